// nbk_tables.hpp -- host only: what nbk_model_create derives from a descriptor before anything touches a device.
//   desc_check      validates the table groups of a nbk_model_desc a caller is about to read;
//   compile_tables  turns a checked descriptor into ModelTables: every table of the device blob, the host mirrors of nbk_model and the
//                   Spec text of the per-robot broadphase, stage by stage (compile_geometry is its first half).
// No kernel and no HIP runtime call in this file: the host-only entry points run it on machines without a device.  nbk.hip includes it
// after what it uses: the K_* kinds, MotionTab and world_reach_bound (nbk_device.hpp), the LDS layouts (nbk_lds.hpp), JK_*, NSUB
// and g_err.  Every expression here feeds a table the kernels and the oracle agree on bit for bit.
#pragma once

namespace nbk {

// ---- descriptor checks ------------------------------------------------------------------------------------------------------------
// the table groups of a descriptor; a caller names the ones it is going to read
enum : unsigned {
    D_JOINTS = 1,        // joint_parent / type / qidx / trans / slide: parents first, q columns and types in range
    D_CHAIN = 2,         // joint_rot, joint_axis, base_pose (what FK reads on top of D_JOINTS)
    D_RSHAPES = 4,       // rshape_frame / type / local / param: frames, types and hull indices in range
    D_WSHAPES = 8,       // wshape_type / param / pose: types and hull indices in range
    D_HULL_VERTS = 16,   // hull_vert_begin, hull_verts: lists start at 0 and none is empty
    D_HULL_PLANES = 32,  // hull_face_begin, hull_planes: finite vertices, unit normals that bound the vertex set (implies D_HULL_VERTS)
    D_PAIRS = 64,        // pair_a / pair_b in range
    D_MOTION = D_JOINTS | D_RSHAPES | D_HULL_VERTS | D_PAIRS,      // what MotionTab is made from
    D_ALL = 127
};

static int32_t desc_check(const nbk_model_desc* d, unsigned parts) {
    if (d == nullptr) return NBK_ERR_INVALID;
    const int J = d->n_joints, S = d->n_rshapes, W = d->n_wshapes, P = d->n_pairs, H = d->n_hulls;
    if (d->n_q < 0 || J < 0 || S < 0 || W < 0 || P < 0 || H < 0) return NBK_ERR_INVALID;
    if (J > NBK_MAX_JOINTS || d->n_q > NBK_MAX_DOF) return NBK_ERR_UNSUPPORTED;
    if (parts & D_HULL_PLANES) parts |= D_HULL_VERTS;
    if ((parts & D_HULL_VERTS) && H > 0) {
        if (d->hull_vert_begin == nullptr || d->hull_verts == nullptr || d->hull_vert_begin[0] != 0) return NBK_ERR_INVALID;
        for (int h = 0; h < H; ++h) if (d->hull_vert_begin[h + 1] <= d->hull_vert_begin[h]) return NBK_ERR_INVALID;
    }
    if ((parts & D_HULL_PLANES) && H > 0) {
        if (d->hull_face_begin == nullptr || d->hull_face_begin[0] != 0) return NBK_ERR_INVALID;
        for (int h = 0; h < H; ++h) if (d->hull_face_begin[h + 1] < d->hull_face_begin[h]) return NBK_ERR_INVALID;
        if (d->hull_face_begin[H] > 0 && d->hull_planes == nullptr) return NBK_ERR_INVALID;
        // face planes: unit outward normals that bound the vertex set (n.v <= d for every vertex).  The float32 broadphase certifies
        // hits from the ball the planes inscribe and the overlap depth walks them: planes that are not what nbk.h asks for would
        // produce verdicts neither the narrowphase nor the oracle ever re-examines.
        for (int h = 0; h < H; ++h) {
            const double* v = d->hull_verts + 3 * (size_t)d->hull_vert_begin[h];
            const int nv = d->hull_vert_begin[h + 1] - d->hull_vert_begin[h];
            double vmax = 0.0;
            for (int i = 0; i < 3 * nv; ++i) { if (!(fabs(v[i]) <= 1e300)) return NBK_ERR_INVALID; vmax = std::max(vmax, fabs(v[i])); }
            for (int f = d->hull_face_begin[h]; f < d->hull_face_begin[h + 1]; ++f) {
                const double* pl = d->hull_planes + 4 * (size_t)f;
                const double n2 = pl[0] * pl[0] + pl[1] * pl[1] + pl[2] * pl[2];
                if (!(fabs(n2 - 1.0) <= 1e-9) || !(fabs(pl[3]) <= 1e300)) {
                    snprintf(g_err, sizeof(g_err), "hull %d, plane %d: the normal must have unit length (|n|^2 = %.17g)", h, f - d->hull_face_begin[h], n2);
                    return NBK_ERR_INVALID;
                }
                const double tol = 1e-9 * (1.0 + fabs(pl[3]) + vmax);
                for (int i = 0; i < nv; ++i)
                    if (pl[0] * v[3 * i] + pl[1] * v[3 * i + 1] + pl[2] * v[3 * i + 2] > pl[3] + tol) {
                        snprintf(g_err, sizeof(g_err), "hull %d, plane %d does not bound vertex %d (n.v - d = %.3g)", h, f - d->hull_face_begin[h], i,
                                 pl[0] * v[3 * i] + pl[1] * v[3 * i + 1] + pl[2] * v[3 * i + 2] - pl[3]);
                        return NBK_ERR_INVALID;
                    }
            }
        }
    }
    auto hull_ok = [&](double idx) { return idx >= 0.0 && idx < (double)H && idx == (double)(int)idx; };
    if (parts & D_JOINTS) {
        if (J > 0 && (!d->joint_parent || !d->joint_type || !d->joint_qidx || !d->joint_trans || !d->joint_slide)) return NBK_ERR_INVALID;
        for (int k = 0; k < J; ++k) {
            if (d->joint_parent[k] >= k || d->joint_parent[k] < -1) return NBK_ERR_INVALID;   // parents first
            if (d->joint_qidx[k] < 0 || d->joint_qidx[k] >= d->n_q) return NBK_ERR_INVALID;
            if (d->joint_type[k] != NBK_REVOLUTE && d->joint_type[k] != NBK_PRISMATIC) return NBK_ERR_INVALID;
        }
    }
    if ((parts & D_CHAIN) && (d->base_pose == nullptr || (J > 0 && (d->joint_rot == nullptr || d->joint_axis == nullptr)))) return NBK_ERR_INVALID;
    if (parts & D_RSHAPES) {
        if (S > 0 && (!d->rshape_frame || !d->rshape_type || !d->rshape_local || !d->rshape_param)) return NBK_ERR_INVALID;
        for (int s = 0; s < S; ++s) {
            if (d->rshape_frame[s] < -1 || d->rshape_frame[s] >= J) return NBK_ERR_INVALID;
            const int t = d->rshape_type[s];
            if (!((t >= NBK_SPHERE && t <= NBK_CYLINDER) || t == NBK_HULL)) return NBK_ERR_INVALID;
            if (t == NBK_HULL && !hull_ok(d->rshape_param[4 * s])) return NBK_ERR_INVALID;
        }
    }
    if (parts & D_WSHAPES) {
        if (W > 0 && (d->wshape_type == nullptr || d->wshape_param == nullptr || d->wshape_pose == nullptr)) return NBK_ERR_INVALID;
        for (int w = 0; w < W; ++w) {
            const int t = d->wshape_type[w];
            if (t < NBK_SPHERE || t > NBK_HULL || (t == NBK_HULL && !hull_ok(d->wshape_param[4 * w]))) return NBK_ERR_INVALID;
        }
    }
    if (parts & D_PAIRS) {
        if (P > 0 && (d->pair_a == nullptr || d->pair_b == nullptr)) return NBK_ERR_INVALID;
        for (int p = 0; p < P; ++p)
            if (d->pair_a[p] < 0 || d->pair_a[p] >= S || d->pair_b[p] < 0 || d->pair_b[p] >= S + W) return NBK_ERR_INVALID;
    }
    return NBK_OK;
}

// ---- shape cores ------------------------------------------------------------------------------------------------------------------
static void core_params(int type, const double* param, int& kind, double* cc) {
    cc[0] = cc[1] = cc[2] = cc[3] = cc[4] = 0.0;
    switch (type) {
        case NBK_SPHERE: kind = K_POINT; cc[4] = param[0]; break;
        case NBK_CAPSULE: kind = K_SEG; cc[4] = param[0]; cc[0] = param[1]; break;
        case NBK_BOX:
            kind = K_BOX; cc[4] = param[3];
            cc[0] = param[0] - param[3]; cc[1] = param[1] - param[3]; cc[2] = param[2] - param[3];
            break;
        case NBK_CYLINDER: kind = K_CYL; cc[4] = param[3]; cc[3] = param[0] - param[3]; cc[0] = param[1] - param[3]; break;
        case NBK_HULL: kind = K_HULL; cc[4] = param[3]; break;      // cc[0..2] (the HullRef) and the radius are filled in by the caller
        default: kind = K_PLANE; break;
    }
}

static double host_bound_radius(int kind, const double* cc) {
    // must round exactly like the oracle's core_bound_radius
    switch (kind) {
        case K_POINT: return 0.0;
        case K_SEG: return cc[0];
        case K_CYL: return sqrt(fma(cc[3], cc[3], cc[0] * cc[0]));
        case K_BOX: return sqrt(fma(cc[2], cc[2], fma(cc[1], cc[1], cc[0] * cc[0])));
        case K_HULL: return cc[5];                 // stored: hull_bound_radius of its vertices
        default: return HUGE_VAL;
    }
}

// largest vertex norm of a hull; must round exactly like the oracle's hull_bound_radius
static double hull_bound_radius(const double* v, int n) {
    double best = 0.0;
    for (int k = 0; k < n; ++k) {
        const double r2 = fma(v[3 * k + 2], v[3 * k + 2], fma(v[3 * k + 1], v[3 * k + 1], v[3 * k] * v[3 * k]));
        if (r2 > best) best = r2;
    }
    return sqrt(best);
}

// local bounding box of a hull's n vertices (centre, half extents rounded outwards): the six values in front of its vertex list
// (the scene's hull blob and a held object's)
static void hull_local_box(const double* v, int n, double* box) {
    double lo[3] = {v[0], v[1], v[2]}, hi[3] = {v[0], v[1], v[2]};
    for (int k = 1; k < n; ++k)
        for (int j = 0; j < 3; ++j) { lo[j] = std::min(lo[j], v[3 * k + j]); hi[j] = std::max(hi[j], v[3 * k + j]); }
    for (int j = 0; j < 3; ++j) { box[j] = 0.5 * (lo[j] + hi[j]); box[3 + j] = 0.5 * (hi[j] - lo[j]) * (1.0 + 1e-12) + 1e-300; }
}

static int host_core_rows(int kind) { return kind == K_POINT ? 3 : ((kind == K_BOX || kind == K_HULL) ? 12 : 6); }
// core parameters of robot shape s as the descriptor stores them: h0 h1 h2 rad margin rho (rho: bounding radius about the centre)
static void robot_core_host(const nbk_model_desc* d, int s, int& kind, double* cc) {
    core_params(d->rshape_type[s], d->rshape_param + 4 * s, kind, cc);
    if (kind == K_HULL) {
        const int h = (int)d->rshape_param[4 * s];
        cc[5] = hull_bound_radius(d->hull_verts + 3 * (size_t)d->hull_vert_begin[h], d->hull_vert_begin[h + 1] - d->hull_vert_begin[h]);
    }
    cc[5] = host_bound_radius(kind, cc);
}

static double norm3_host(const double* v) { return sqrt(fma(v[2], v[2], fma(v[1], v[1], v[0] * v[0]))); }
// per joint frame: the joints on the path from the base to it (bit k = joint k)
static std::vector<unsigned> frame_masks(const nbk_model_desc* d) {
    std::vector<unsigned> m(d->n_joints > 0 ? d->n_joints : 1, 0u);
    for (int k = 0; k < d->n_joints; ++k) m[k] = (d->joint_parent[k] >= 0 ? m[d->joint_parent[k]] : 0u) | (1u << k);
    return m;
}

// host copies of the MotionTab tables (nbk_model_create uploads them; nbk_edge_motion_bounds_host uses them in place)
struct MotionHost {
    std::vector<int> jtype, jqidx, pa, pb;
    std::vector<double> jtn, jsn, sloc, sbnd;
    std::vector<unsigned> smask;
    MotionTab view(int J, int S) const {
        return MotionTab{J, S, jtype.data(), jqidx.data(), jtn.data(), jsn.data(), smask.data(), sloc.data(), sbnd.data(), pa.data(), pb.data()};
    }
};

// fills h from a descriptor that passed desc_check(d, D_MOTION)
static void motion_tables(const nbk_model_desc* d, const std::vector<unsigned>& fmask, MotionHost& h) {
    const int J = d->n_joints, S = d->n_rshapes, P = d->n_pairs;
    const size_t J1 = J > 0 ? J : 1, S1 = S > 0 ? S : 1, P1 = P > 0 ? P : 1;
    h.jtype.assign(J1, 0); h.jqidx.assign(J1, 0); h.jtn.assign(J1, 0.0); h.jsn.assign(J1, 0.0);
    for (int k = 0; k < J; ++k) {
        h.jtype[k] = d->joint_type[k];
        h.jqidx[k] = d->joint_qidx[k];
        h.jtn[k] = norm3_host(d->joint_trans + 3 * k);
        h.jsn[k] = norm3_host(d->joint_slide + 3 * k);
    }
    h.smask.assign(S1, 0u); h.sloc.assign(S1, 0.0); h.sbnd.assign(S1, 0.0);
    for (int x = 0; x < S; ++x) {
        const int f = d->rshape_frame[x];
        h.smask[x] = f >= 0 ? fmask[f] : 0u;
        const double* L = d->rshape_local + 12 * (size_t)x;
        const double tl[3] = {L[3], L[7], L[11]};
        h.sloc[x] = norm3_host(tl);
        int kind;
        double cc[6];
        robot_core_host(d, x, kind, cc);
        h.sbnd[x] = cc[5] + cc[4];
    }
    h.pa.assign(d->pair_a, d->pair_a + P); h.pa.resize(P1, 0);
    h.pb.assign(d->pair_b, d->pair_b + P); h.pb.resize(P1, 0);
}

// ---- the compiled tables ----------------------------------------------------------------------------------------------------------
// Everything nbk_model_create derives from a descriptor, by the stage that makes it (tables sized "n > 0 ? n : 1": data() is never null)
struct ModelTables {
    // frame load/save plan
    std::vector<int> load, save;  int slots = 0;
    // shape order and cores: robot shapes in frame order (`order[i]` = descriptor index of shape i)
    std::vector<int> order, begin, rs_kind, rs_row, rs_frame, rs_hull, ws_kind, ws_hull;      // *_hull: hull index of K_HULL shapes, else -1
    std::vector<double> rs_local, rs_core, ws_core, ws_center;
    std::vector<unsigned> frame_mask, rs_mask;
    int rows = 0;  bool world_hulls = false;
    // pair classes and the validity tables
    std::vector<int> pa, pb, pu, pdev, vp_tab, vp_canon;
    std::vector<double> vp_cst, gjk_margins;
    int n_plane = 0, n_closed = 0;  bool margins_zero = true, gjk_any_hull = false;
    // broadphase order, static reach; the LDS verdicts of the compiled-in limits
    std::vector<int> bq_tab;  std::vector<double> bq_static, reach;
    bool lds_broad_ok = false, parked_ok = false;
    // joint tables
    std::vector<double> jrot, jtrans, joint_pk;  std::vector<int> joint_kind;  MotionHost mh;
    // queue groups
    std::vector<int> vp_info, vp_cls;
    int cls_count[4] = {0, 0, 0, 0}, cls_groups[4] = {0, 0, 0, 0}, cls_base[4] = {0, 0, 0, 0};
    // float tables and slack
    std::vector<double> hull_obb;  std::vector<float> ftab;
    int f_trans = 0, f_slide = 0, f_base = 0, f_tl = 0, f_wc = 0, f_wobb = 0, f_pk = 0, f_meta = 0, f_chain = 0;
    float f_eps = 0.0f, f_reach = 0.0f, f_e2max = 0.0f;
    std::string spec;             // the `struct Spec` of the per-robot broadphase, "" when the robot does not take it
    // inscribed radii and the hull blob
    std::vector<double> rs_in, ws_in, hull_blob;
    std::vector<size_t> hull_off;           // offset (in doubles) of hull h's first vertex inside hull_blob
    // shape refs of the validity tables: >= 0 robot shape (frame order), < 0 world shape ~ref
    int kind_of(int ref) const { return ref >= 0 ? rs_kind[ref] : ws_kind[~ref]; }
    const double* core_of(int ref) const { return ref >= 0 ? &rs_core[6 * ref] : &ws_core[18 * (~ref) + 12]; }
};

// frame load/save plan: a frame stays in registers when its child is the next joint
static void plan_frames(const nbk_model_desc* d, ModelTables& t) {
    const int J = d->n_joints;
    t.load.assign(J, 0); t.save.assign(J, -1);
    for (int k = 0; k < J; ++k) {
        const int par = d->joint_parent[k];
        if (par == k - 1) t.load[k] = (par < 0) ? -1 : -2;
        else if (par < 0) t.load[k] = -1;
        else {
            if (t.save[par] < 0) t.save[par] = t.slots++;
            t.load[k] = t.save[par];
        }
    }
}

// robot shapes in frame order with their cores and joint masks, world shapes with theirs
static void order_shapes(const nbk_model_desc* d, ModelTables& t) {
    const int J = d->n_joints, S = d->n_rshapes, W = d->n_wshapes;
    t.begin.assign(J + 2, 0);
    for (int f = -1; f < J; ++f) {
        t.begin[f + 1] = (int)t.order.size();
        for (int s = 0; s < S; ++s) if (d->rshape_frame[s] == f) t.order.push_back(s);
    }
    t.begin[J + 1] = (int)t.order.size();
    t.rs_kind.assign(S, 0); t.rs_row.assign(S, 0);
    t.rs_local.assign(12 * (size_t)S, 0.0); t.rs_core.assign(6 * (size_t)S, 0.0);
    t.rs_hull.assign(S > 0 ? S : 1, -1); t.ws_hull.assign(W > 0 ? W : 1, -1);
    t.rs_frame.assign(S > 0 ? S : 1, -1); t.rs_mask.assign(S > 0 ? S : 1, 0u);
    t.frame_mask = frame_masks(d);
    for (int i = 0; i < S; ++i) {
        const int s = t.order[i];
        int kind;
        robot_core_host(d, s, kind, &t.rs_core[6 * i]);
        if (kind == K_HULL) t.rs_hull[i] = (int)d->rshape_param[4 * s];
        t.rs_kind[i] = kind;
        t.rs_row[i] = t.rows;
        t.rows += host_core_rows(kind);
        memcpy(&t.rs_local[12 * i], d->rshape_local + 12 * s, 12 * sizeof(double));
        t.rs_frame[i] = d->rshape_frame[s];
        t.rs_mask[i] = t.rs_frame[i] >= 0 ? t.frame_mask[t.rs_frame[i]] : 0u;
    }
    t.ws_kind.assign(W, 0); t.ws_core.assign(18 * (size_t)W, 0.0); t.ws_center.assign(3 * (size_t)W, 0.0);
    for (int w = 0; w < W; ++w) {
        double cc[6];  int kind;
        core_params(d->wshape_type[w], d->wshape_param + 4 * w, kind, cc);
        cc[5] = 0.0;
        if (kind == K_HULL) {
            const int h = (int)d->wshape_param[4 * w];
            cc[5] = hull_bound_radius(d->hull_verts + 3 * (size_t)d->hull_vert_begin[h], d->hull_vert_begin[h + 1] - d->hull_vert_begin[h]);
            t.ws_hull[w] = h;
        }
        t.ws_kind[w] = kind;
        t.world_hulls = t.world_hulls || kind == K_HULL;
        const double* T = d->wshape_pose + 12 * w;
        double* o = &t.ws_core[18 * w];
        o[0] = T[3]; o[1] = T[7]; o[2] = T[11];
        for (int j = 0; j < 3; ++j) { o[3 + 3 * j] = T[j]; o[4 + 3 * j] = T[4 + j]; o[5 + 3 * j] = T[8 + j]; }
        if (kind == K_PLANE) { o[9] = d->wshape_param[4 * w]; o[10] = d->wshape_param[4 * w + 1]; o[11] = d->wshape_param[4 * w + 2]; }
        o[12] = cc[0]; o[13] = cc[1]; o[14] = cc[2]; o[15] = cc[3]; o[16] = cc[4];
        o[17] = host_bound_radius(kind, cc);
        t.ws_center[3 * w] = o[0]; t.ws_center[3 * w + 1] = o[1]; t.ws_center[3 * w + 2] = o[2];
    }
}

// pairs in frame order, then the validity tables: pairs stably sorted by class (0 plane, 1 closed form, 2 GJK)
static void pair_tables(const nbk_model_desc* d, ModelTables& t) {
    const int S = d->n_rshapes, P = d->n_pairs;
    std::vector<int> new_index(S);
    for (int i = 0; i < S; ++i) new_index[t.order[i]] = i;
    t.pa.assign(P, 0); t.pb.assign(P, 0); t.pu.assign(P, 0); t.pdev.assign(P > 0 ? P : 1, 0);
    std::vector<int> vcls(P), vorder(P), refA(P), refB(P);
    for (int p = 0; p < P; ++p) {
        t.pa[p] = new_index[d->pair_a[p]];
        t.pb[p] = d->pair_b[p] < S ? new_index[d->pair_b[p]] : d->pair_b[p];
        t.pu[p] = p;
        t.pdev[t.pu[p]] = p;
        refA[p] = t.pa[p];
        refB[p] = t.pb[p] < S ? t.pb[p] : ~(t.pb[p] - S);
        const int ka = t.kind_of(refA[p]), kb = t.kind_of(refB[p]);
        const bool a_ps = (ka == K_POINT || ka == K_SEG), b_ps = (kb == K_POINT || kb == K_SEG);
        if (kb == K_PLANE) vcls[p] = 0;
        else if (ka == K_HULL || kb == K_HULL) vcls[p] = 2;           // hulls have no closed forms: GJK, also against a point
        else if ((a_ps && b_ps) || ka == K_POINT || kb == K_POINT) vcls[p] = 1;
        else vcls[p] = 2;
    }
    int cur = 0;
    for (int c = 0; c < 3; ++c)
        for (int p = 0; p < P; ++p)
            if (vcls[p] == c) { vorder[cur++] = p; if (c == 0) ++t.n_plane; if (c == 1) ++t.n_closed; }
    t.vp_tab.assign(4 * (size_t)P, 0); t.vp_canon.assign(2 * (size_t)P, 0); t.vp_cst.assign(4 * (size_t)P, 0.0);
    for (int i = 0; i < P; ++i) {
        const int p = vorder[i];
        const int ka = t.kind_of(refA[p]), kb = t.kind_of(refB[p]);
        t.vp_tab[4 * i] = refA[p]; t.vp_tab[4 * i + 1] = refB[p]; t.vp_tab[4 * i + 2] = vcls[p]; t.vp_tab[4 * i + 3] = p;
        const bool swap = ka > kb;
        t.vp_canon[2 * i] = swap ? refB[p] : refA[p];
        t.vp_canon[2 * i + 1] = swap ? refA[p] : refB[p];
        const double* ca = t.core_of(refA[p]);
        const double* cb = t.core_of(refB[p]);
        t.vp_cst[4 * i] = ca[4]; t.vp_cst[4 * i + 1] = cb[4];
        t.vp_cst[4 * i + 2] = host_bound_radius(ka, ca);
        t.vp_cst[4 * i + 3] = host_bound_radius(kb, cb);
        const int k0 = ka < kb ? ka : kb, k1 = ka < kb ? kb : ka;          // canonical order
        const bool closed = k1 != K_HULL && (k0 == K_POINT || ((k0 == K_POINT || k0 == K_SEG) && (k1 == K_POINT || k1 == K_SEG)));
        if (k1 != K_PLANE && !closed && (ca[4] != 0.0 || cb[4] != 0.0)) t.margins_zero = false;
        if (k1 != K_PLANE && !closed) { t.gjk_margins.push_back(ca[4]); t.gjk_margins.push_back(cb[4]); if (k1 == K_HULL) t.gjk_any_hull = true; }
    }
}

// broadphase order: category-major (0 plane, 1 robot-robot, 2 robot-world, 3 robot-world box), then by pair
static void broad_order(const nbk_model_desc* d, ModelTables& t) {
    const int P = d->n_pairs;
    t.bq_tab.assign(4 * (size_t)(P > 0 ? P : 1), 0);
    int cur_b = 0;
    for (int cat = 0; cat < 4; ++cat)
        for (int i = 0; i < P; ++i) {
            const int ra = t.vp_tab[4 * i], rb = t.vp_tab[4 * i + 1];
            const int c = rb >= 0 ? 1 : (t.ws_kind[~rb] == K_PLANE ? 0 : (t.ws_kind[~rb] == K_BOX ? 3 : 2));
            if (c != cat) continue;
            t.bq_tab[4 * cur_b] = 3 * ra;
            t.bq_tab[4 * cur_b + 1] = rb >= 0 ? 3 * rb : ~rb;
            t.bq_tab[4 * cur_b + 2] = i;
            t.bq_tab[4 * cur_b + 3] = cat;
            ++cur_b;
        }
}

// static reach bound of broadphase pair j with the world shapes at `poses` [W][12]: -inf for a robot-robot pair and behind a prismatic joint
static double pair_reach_bound(const nbk_model_desc* d, const ModelTables& t, int j, const double* poses) {
    const int cat = t.bq_tab[4 * j + 3], a = t.bq_tab[4 * j] / 3, w = t.bq_tab[4 * j + 1], i = t.bq_tab[4 * j + 2];
    if (cat == 1 || !(t.reach[a] < INFINITY)) return -INFINITY;
    const double* T = poses + 12 * (size_t)w;
    const double c[3] = {T[3], T[7], T[11]}, b0[3] = {d->base_pose[3], d->base_pose[7], d->base_pose[11]};
    return world_reach_bound(cat == 0, c, d->wshape_param + 4 * (size_t)w, b0, t.reach[a], t.vp_cst[4 * i + 2], t.vp_cst[4 * i + 3]);
}

// static reach culling: the centre of robot shape a never leaves the ball of radius reach_a around the base origin
// (sum of the joint offsets on its path + its local offset; unbounded when a prismatic joint is on the path), so a world
// shape farther than that from the base, radii included, can never be a candidate.  Rigorous by the triangle inequality.
static void static_reach(const nbk_model_desc* d, ModelTables& t) {
    const int J = d->n_joints, S = d->n_rshapes, P = d->n_pairs;
    t.bq_static.assign((size_t)(P > 0 ? P : 1), -INFINITY);       // (P = 0: one element, never uploaded)
    t.reach.assign(S > 0 ? S : 1, 0.0);          // per robot shape (frame order); k_world_update reads a device copy
    for (int i = 0; i < S; ++i) {
        const int f = t.rs_frame[i];
        double r = 0.0;
        bool unbounded = false;
        if (f >= 0)
            for (int k = 0; k < J; ++k)
                if ((t.frame_mask[f] >> k) & 1u) {
                    if (d->joint_type[k] == NBK_PRISMATIC) unbounded = true;
                    r += std::sqrt(d->joint_trans[3 * k] * d->joint_trans[3 * k] + d->joint_trans[3 * k + 1] * d->joint_trans[3 * k + 1] +
                                   d->joint_trans[3 * k + 2] * d->joint_trans[3 * k + 2]);
                }
        const double lx = t.rs_local[12 * i + 3], ly = t.rs_local[12 * i + 7], lz = t.rs_local[12 * i + 11];
        r += std::sqrt(lx * lx + ly * ly + lz * lz);
        t.reach[i] = unbounded ? INFINITY : r * (1.0 + 1e-12) + 1e-12;
    }
    for (int j = 0; j < P; ++j) t.bq_static[j] = pair_reach_bound(d, t, j, d->wshape_pose);
}

// the geometry half of compile_tables; nbk_world_reach_bounds_host stops here, ahead of the compiled-in limits and the joint tables
static void compile_geometry(const nbk_model_desc* d, ModelTables& t) {
    plan_frames(d, t);
    order_shapes(d, t);
    pair_tables(d, t);
    broad_order(d, t);
    static_reach(d, t);
}

// the compiled-in limits; sets the two LDS verdicts
static int32_t check_limits(const nbk_model_desc* d, ModelTables& t) {
    const int S = d->n_rshapes, W = d->n_wshapes, P = d->n_pairs;
    if (3 * S >= 65536 || W >= 65536 || P >= (1 << 20)) return NBK_ERR_UNSUPPORTED;      // (the layouts below count in int)
    // the LDS broadphase (robots with more than 16 primitives) keeps the pair constants and world cores in LDS; robots the
    // register broadphases serve do not need it, however many world shapes there are
    t.lds_broad_ok = lds_broad_ok(d->n_q, t.slots, S, P, W);
    if (!t.lds_broad_ok && S > 16) return NBK_ERR_UNSUPPORTED;
    // robots whose primitives do not fit the LDS-parked layout (some 25+ shapes) keep validity and edges, through the
    // broadphase + narrowphase kernels at every batch size; the per-pair distance entry points report UNSUPPORTED for them
    t.parked_ok = ValidityLds(d->n_q, t.rows > d->n_q ? t.rows : d->n_q, t.slots).fits();
    if (S <= 16 && !broad_f32_ok(d->n_q, t.slots, S)) return NBK_ERR_UNSUPPORTED;
    if (P >= (1 << 26)) return NBK_ERR_UNSUPPORTED;
    return NBK_OK;
}

// the 15 packed constants of a joint about coordinate axis KZ of its frame (U, V = the two other axes) from its joint_rot block M: the pairs
// (M2[r][U], M2[r][V]) and (M1[r][U], M1[r][V]), r = 0..2, then column KZ of M0; for the double rows of joint_pk and, cast, the float rows at f_pk
template <class T>
static void pack_joint_rot(const double* M, int joint_kind, T* out) {
    const int kz = joint_kind <= 2 ? joint_kind : 0;
    const int u = (kz + 1) % 3, v = (kz + 2) % 3;
    for (int r = 0; r < 3; ++r) {
        out[2 * r] = (T)M[18 + 3 * r + u]; out[2 * r + 1] = (T)M[18 + 3 * r + v];
        out[6 + 2 * r] = (T)M[9 + 3 * r + u]; out[6 + 2 * r + 1] = (T)M[9 + 3 * r + v];
        out[12 + r] = (T)M[3 * r + kz];
    }
}

// joint tables: exact zeros are stored as +0 (so that a literal 0.0 in the axis-aligned fast paths is the same operand), every joint
// is classified (which coordinate axis of the joint frame it turns about, if any) and its packed row made; the MotionTab tables
static int32_t joint_tables(const nbk_model_desc* d, ModelTables& t) {
    const int J = d->n_joints;
    t.jrot.assign(d->joint_rot, d->joint_rot + 27 * (size_t)J); t.jtrans.assign(d->joint_trans, d->joint_trans + 3 * (size_t)J);
    for (double& v : t.jrot) v += 0.0;  for (double& v : t.jtrans) v += 0.0;
    t.joint_kind.assign(J > 0 ? J : 1, JK_GENERIC);
    t.joint_pk.assign(22 * (size_t)(J > 0 ? J : 1), 0.0);
    for (int k = 0; k < J; ++k) {
        const double* Mk = &t.jrot[27 * (size_t)k];
        if (d->joint_type[k] == NBK_PRISMATIC) {
            bool zero = true;
            for (int e = 9; e < 27; ++e) zero = zero && Mk[e] == 0.0;
            if (!zero) { snprintf(g_err, sizeof(g_err), "prismatic joint %d: M1 / M2 of joint_rot must be zero", k); return NBK_ERR_INVALID; }
            t.joint_kind[k] = JK_PRISMATIC;
        } else {
            for (int kz = 0; kz < 3; ++kz) {
                const int u = (kz + 1) % 3, v = (kz + 2) % 3;
                bool ok = d->joint_slide[3 * k] == 0.0 && d->joint_slide[3 * k + 1] == 0.0 && d->joint_slide[3 * k + 2] == 0.0;
                for (int r = 0; r < 3; ++r)
                    ok = ok && Mk[9 + 3 * r + kz] == 0.0 && Mk[18 + 3 * r + kz] == 0.0 && Mk[3 * r + u] == 0.0 && Mk[3 * r + v] == 0.0;
                if (ok) { t.joint_kind[k] = kz; break; }
            }
        }
        double* jp = &t.joint_pk[22 * (size_t)k];
        pack_joint_rot(Mk, t.joint_kind[k], jp);
        for (int r = 0; r < 3; ++r) { jp[15 + r] = t.jtrans[3 * k + r]; jp[18 + r] = d->joint_axis[3 * k + r]; }
    }
    motion_tables(d, t.frame_mask, t.mh);
    return NBK_OK;
}

// queue groups: canonical refs with their joint masks, every pair's kind class, sub-queues per class in proportion to its pairs (at least one)
static void queue_groups(const nbk_model_desc* d, ModelTables& t) {
    const int P = d->n_pairs;
    t.vp_info.assign(4 * (size_t)(P > 0 ? P : 1), 0);
    t.vp_cls.assign((size_t)(P > 0 ? P : 1), 3);
    for (int i = 0; i < P; ++i) {
        const int ra = t.vp_canon[2 * i], rb = t.vp_canon[2 * i + 1];
        t.vp_info[4 * i] = ra; t.vp_info[4 * i + 1] = rb;
        t.vp_info[4 * i + 2] = ra >= 0 ? (int)t.rs_mask[ra] : 0;
        t.vp_info[4 * i + 3] = rb >= 0 ? (int)t.rs_mask[rb] : 0;
        const int ka = t.kind_of(ra), kb = t.kind_of(rb);
        t.vp_cls[i] = (ka == K_BOX && kb == K_BOX) ? 0 : ((ka == K_BOX && kb == K_CYL) ? 1 : ((ka == K_CYL && kb == K_CYL) ? 2 : 3));
        t.cls_count[t.vp_cls[i]] += 1;
    }
    int used = 0, nonempty = 0;
    for (int c = 0; c < 4; ++c) if (t.cls_count[c] > 0) ++nonempty;
    const int spare = NSUB - nonempty;
    for (int c = 0; c < 4; ++c)
        if (t.cls_count[c] > 0) { t.cls_groups[c] = 1 + (int)((long long)spare * t.cls_count[c] / (P > 0 ? P : 1)); used += t.cls_groups[c]; }
    // hand what rounding left over to the largest class
    int big = 0;
    for (int c = 1; c < 4; ++c) if (t.cls_count[c] > t.cls_count[big]) big = c;
    if (P > 0) t.cls_groups[big] += NSUB - used;
    for (int c = 1; c < 4; ++c) t.cls_base[c] = t.cls_base[c - 1] + t.cls_groups[c - 1];
}

// float32 tables + error slack of the conservative broadphase.  Position error of a float32 chain sweep is below
// (joints + 2) * 16 ulp(float) * reach; the slack is 50x that, never below 1e-4 of the reach.
static void float_tables(const nbk_model_desc* d, const double* world_radius, ModelTables& t) {
    const int J = d->n_joints, S = d->n_rshapes, W = d->n_wshapes, H = d->n_hulls;
    // local bounding box of every hull (centre, half extents rounded outwards): the hull midphase culls against it
    t.hull_obb.assign(6 * (size_t)(H > 0 ? H : 1), 0.0);
    for (int h = 0; h < H; ++h)
        hull_local_box(d->hull_verts + 3 * (size_t)d->hull_vert_begin[h], d->hull_vert_begin[h + 1] - d->hull_vert_begin[h], &t.hull_obb[6 * h]);
    std::vector<float>& ftab = t.ftab;
    double freach = 0.0;
    for (int k = 0; k < J; ++k) for (int e = 0; e < 27; ++e) ftab.push_back((float)d->joint_rot[27 * k + e]);
    t.f_trans = (int)ftab.size();
    for (int k = 0; k < J; ++k) {
        double n2 = 0.0;
        for (int e = 0; e < 3; ++e) { ftab.push_back((float)d->joint_trans[3 * k + e]); n2 += d->joint_trans[3 * k + e] * d->joint_trans[3 * k + e]; }
        freach += std::sqrt(n2);
    }
    t.f_slide = (int)ftab.size();
    for (int k = 0; k < J; ++k) for (int e = 0; e < 3; ++e) ftab.push_back((float)d->joint_slide[3 * k + e]);
    t.f_base = (int)ftab.size();
    double b2 = 0.0;
    for (int e = 0; e < 12; ++e) ftab.push_back((float)d->base_pose[e]);
    for (int i = 0; i < 3; ++i) b2 += d->base_pose[4 * i + 3] * d->base_pose[4 * i + 3];
    freach += std::sqrt(b2);
    t.f_tl = (int)ftab.size();
    double lmax = 0.0;
    for (int i = 0; i < S; ++i) {
        double n2 = 0.0;
        for (int r = 0; r < 3; ++r) { const double v = t.rs_local[12 * i + 4 * r + 3]; ftab.push_back((float)v); n2 += v * v; }
        if (std::sqrt(n2) > lmax) lmax = std::sqrt(n2);
    }
    freach += lmax;
    t.f_wc = (int)ftab.size();
    for (int w = 0; w < W; ++w) {
        double n2 = 0.0;
        for (int e = 0; e < 18; ++e) ftab.push_back((float)t.ws_core[18 * w + e]);
        for (int e = 0; e < 3; ++e) n2 += t.ws_core[18 * w + e] * t.ws_core[18 * w + e];
        if (std::sqrt(n2) > freach) freach = std::sqrt(n2);          // world coordinates enter the differences too
    }
    // a movable descriptor: every centre its poses may ever have (the caller's promise, checked by k_world_update)
    if (world_radius != nullptr && *world_radius > freach) freach = *world_radius;
    t.f_wobb = (int)ftab.size();
    for (int w = 0; w < W; ++w)
        for (int e = 0; e < 6; ++e) {
            const double v = t.ws_hull[w] >= 0 ? t.hull_obb[6 * (size_t)t.ws_hull[w] + e] : 0.0;
            ftab.push_back(e < 3 ? (float)v : (float)v * (1.0f + 2.4e-7f));          // half extents rounded up
        }
    // packed sweep of k_broad_f32, 20 floats per joint: the 15 of pack_joint_rot, pad, offset translation, pad; at least 8 rows (it prefetches k + 1 <= 7)
    while (ftab.size() % 4 != 0) ftab.push_back(0.0f);
    t.f_pk = (int)ftab.size();
    ftab.resize(ftab.size() + 20 * (size_t)(J > 8 ? J : 8), 0.0f);
    for (int k = 0; k < J; ++k) {
        float* fp = &ftab[t.f_pk + 20 * (size_t)k];
        pack_joint_rot(d->joint_rot + 27 * (size_t)k, t.joint_kind[k], fp);
        for (int e = 0; e < 3; ++e) fp[16 + e] = (float)d->joint_trans[3 * k + e];
    }
    t.f_meta = (int)ftab.size();
    for (int k = 0; k < 8; ++k) {
        const unsigned v = k < J ? ((unsigned)t.joint_kind[k] | ((unsigned)d->joint_qidx[k] << 8)) : 0u;
        float fv; memcpy(&fv, &v, 4);
        ftab.push_back(fv);
    }
    t.f_chain = (J >= 1 && J <= 8 && S <= 16) ? 1 : 0;
    for (int k = 0; k < J && t.f_chain; ++k) if (t.load[k] != (k == 0 ? -1 : -2) || t.save[k] != -1) t.f_chain = 0;
    // slack constants of the float32 broadphase: 50 x the float32 error bound (joints + 2) * 16 ulp of a chain sweep, relative; the
    // kernel multiplies it by the larger of the static reach and the configuration's own largest coordinate (prismatic travel is
    // unbounded here)
    const double rel = 50.0 * (J + 2) * 16.0 * 5.96e-8;
    t.f_eps = (float)(rel > 1e-4 ? rel : 1e-4);
    t.f_reach = (float)(freach > 1e-3 ? freach : 1e-3);
    t.f_e2max = 2.0f * t.f_reach * (t.f_eps + 2.4e-7f * 64.0f) * (1.0f + 1e-6f);
}

// world shapes with a pair that the specialised kernel unrolls at most: every one is a fully unrolled block with its own queue
// appends (8 cubes made 140 KB of code for a 64 KB instruction cache and an 11 s compile); other scenes keep the generic kernel
constexpr int SPEC_MAX_WORLD = 2;

// Class of a float32 table value for the folded sweep of the specialised kernel (Spec::fc_*): 0 general, 1 zero, 2 exactly +1,
// 3 exactly -1.  Zero covers the residues that multiples of pi / 2 leave in a URDF's origins (cos(pi / 2) = 6.1e-17): a rotation
// entry up to 2^-40, a length up to 2^-40 of the static reach (`zero_below`).  DESIGN.md §3 charges them to the slack.
constexpr float FOLD_ZERO_REL = 0x1p-40f;
static int fold_class(float v, float zero_below) {
    if (std::fabs(v) <= zero_below) return 1;
    return v == 1.0f ? 2 : (v == -1.0f ? 3 : 0);
}

// The `struct Spec` of one descriptor ("" when the robot does not take the specialised kernel: not a serial chain of at most
// 8 joints, more than 16 shapes, no pairs, too many world shapes).  movable: the world cores at f_wc may be rewritten later
// (k_world_update), so nothing about a world shape's pose is built in
static std::string bf32_spec_text(const nbk_model_desc* d, const ModelTables& t, bool movable) {
    const int S = d->n_rshapes, J = d->n_joints, W = d->n_wshapes, P = d->n_pairs;
    if (!t.f_chain || P == 0 || S < 1 || S > 16 || J < 1 || J > 8) return std::string();
    std::vector<int> rrp((size_t)S * S, -1), wlist;
    std::vector<int> wslot_of(W > 0 ? W : 1, -1);
    for (int j = 0; j < P; ++j) {
        const int* bt = &t.bq_tab[4 * j];
        if (bt[3] != 1 && wslot_of[bt[1]] < 0) { wslot_of[bt[1]] = 0; wlist.push_back(bt[1]); }
    }
    std::sort(wlist.begin(), wlist.end());
    if ((int)wlist.size() > SPEC_MAX_WORLD) return std::string();
    const int NW = (int)wlist.size();
    for (int i = 0; i < NW; ++i) wslot_of[wlist[i]] = i;
    std::vector<int> wp((size_t)(NW > 0 ? NW : 1) * S, -1);
    bool rr_any = false;
    for (int j = 0; j < P; ++j) {
        const int* bt = &t.bq_tab[4 * j];
        const int a = bt[0] / 3;
        if (bt[3] == 1) {
            const int b = bt[1] / 3, lo = a < b ? a : b, hi = a < b ? b : a;
            rrp[(size_t)lo * S + hi] = bt[2];
            rr_any = true;
        } else {
            wp[(size_t)wslot_of[bt[1]] * S + a] = bt[2];
        }
    }
    std::string o;
    char buf[512];
    auto add = [&](const char* fmt, auto... v) { snprintf(buf, sizeof(buf), fmt, v...); o += buf; };
    auto arr = [&](const char* name, const std::vector<int>& v) {
        add("    static constexpr int %s[] = {", name);
        for (size_t i = 0; i < v.size(); ++i) add(i ? ", %d" : "%d", v[i]);
        if (v.empty()) o += "-1";
        o += "};\n";
    };
    const int SB = S <= 8 ? 8 : (S <= 12 ? 12 : 16);
    o += "struct Spec {\n";
    add("    static constexpr int S = %d, SB = %d, NQ = %d, J = %d, W = %d, NW = %d;\n", S, SB, d->n_q, J, W, NW);
    arr("jkind", std::vector<int>(t.joint_kind.begin(), t.joint_kind.begin() + J));
    arr("qcol", std::vector<int>(d->joint_qidx, d->joint_qidx + J));
    arr("sh_begin", t.begin);
    add("    static constexpr int f_rot = 0, f_pk = %d, f_tl = %d, f_base = %d, f_wc = %d, f_wobb = %d, f_trans = %d, f_slide = %d;\n",
        t.f_pk, t.f_tl, t.f_base, t.f_wc, t.f_wobb, t.f_trans, t.f_slide);
    add("    static constexpr float f_eps = %af, f_reach = %af, f_e2max = %af;\n", (double)t.f_eps, (double)t.f_reach, (double)t.f_e2max);
    add("    static constexpr bool rr_any = %s;\n", rr_any ? "true" : "false");
    arr("rrp_", rrp);
    std::vector<int> wk;
    for (int w : wlist) wk.push_back(t.ws_kind[w]);
    arr("wl", wlist);
    arr("wk", wk);
    arr("wp_", wp);
    // a world BOX that can never move and whose axes (the nine floats behind its centre at f_wc) are exactly the coordinate
    // axes: the kernel takes the centre differences as its axis projections (box_slot2<true>)
    std::vector<int> aligned;
    for (int w : wlist) {
        bool id = !movable && t.ws_kind[w] == K_BOX;
        for (int e = 0; e < 9 && id; ++e) id = t.ftab[t.f_wc + 18 * (size_t)w + 3 + e] == (e % 4 == 0 ? 1.0f : 0.0f);
        aligned.push_back(id ? 1 : 0);
    }
    arr("wbox_aligned", aligned);
    // Classes of the robot's own float32 table values, which no call ever rewrites (a movable descriptor's neither), for the folded
    // sweep of the kernel: per joint the 18 used floats of its block at f_pk (m2p, m1p, mk, toff), per shape its offset at f_tl.  (The
    // base pose is not classed: folding an identity base was measured and did not pay)  The tables keep their
    // values: the generic kernel and k_prepare_f32 read the same floats.
    // fc_any = 0 (and every class general) when a table value is outside the range FOLD_QMAX's argument in nbk_bf32_spec.hpp
    // assumes -- a rotation-type entry above 2, a length above 2^20 -- or when no value the folded sweep reads has a class.
    bool fold_ok = t.f_reach <= 0x1p20f;
    for (int e = 0; e < 27 * J; ++e) fold_ok = fold_ok && std::fabs(t.ftab[e]) <= 2.0f;
    for (int e = 0; e < 3 * J; ++e) fold_ok = fold_ok && std::fabs(t.ftab[t.f_trans + e]) <= 0x1p20f && std::fabs(t.ftab[t.f_slide + e]) <= 0x1p20f;
    for (int e = 0; e < 12; ++e) fold_ok = fold_ok && std::fabs(t.ftab[t.f_base + e]) <= (e % 4 == 3 ? 0x1p20f : 2.0f);
    for (int e = 0; e < 3 * S; ++e) fold_ok = fold_ok && std::fabs(t.ftab[t.f_tl + e]) <= 0x1p20f;
    const float zr = FOLD_ZERO_REL, zt = FOLD_ZERO_REL * t.f_reach;
    std::vector<int> fc_pk, fc_tl;
    bool fold_any = false;
    for (int k = 0; k < J; ++k)
        for (int e = 0; e < 18; ++e) {
            fc_pk.push_back(fold_ok ? (e < 15 ? fold_class(t.ftab[t.f_pk + 20 * (size_t)k + e], zr) : fold_class(t.ftab[t.f_pk + 20 * (size_t)k + e + 1], zt)) : 0);
            fold_any = fold_any || (t.joint_kind[k] <= 2 && fc_pk.back() != 0);
        }
    for (int e = 0; e < 3 * S; ++e) { fc_tl.push_back(fold_ok ? fold_class(t.ftab[t.f_tl + e], zt) : 0); fold_any = fold_any || fc_tl.back() != 0; }
    add("    static constexpr int fc_any = %d;\n", fold_any ? 1 : 0);
    arr("fc_pk", fc_pk);
    arr("fc_tl", fc_tl);
    arr("cls_base", std::vector<int>(t.cls_base, t.cls_base + 4));
    std::vector<int> groups(t.cls_groups, t.cls_groups + 4);
    for (int& g : groups) g = g > 0 ? g : 1;             // as DevModel::cls_groups: a divisor, also for a class without pairs
    arr("cls_groups", groups);
    o += "    static constexpr int rr_p(int a, int b) { return a >= 0 && b < S && a < b ? rrp_[a * S + b] : -1; }\n"
         "    static constexpr int wpair(int wi, int a) { return a < S ? wp_[wi * S + a] : -1; }\n"
         "    static constexpr bool rr_group(int a, int i) { return rr_p(a, 2 * i) >= 0 || rr_p(a, 2 * i + 1) >= 0; }\n"
         "    static constexpr int row_slots(int a) { int n = 0; for (int b = a + 1; b < S; ++b) n += rr_p(a, b) >= 0 ? 1 : 0; return n; }\n"
         "};\n";
    return o;
}

// inscribed radii and the hull blob
static void hull_tables(const nbk_model_desc* d, ModelTables& t) {
    const int S = d->n_rshapes, W = d->n_wshapes, H = d->n_hulls;
    // radius of a ball around each shape's centre that lies inside the shape (the float32 broadphase certifies a collision when two
    // such balls overlap): margin + the smallest half extent of the core; hulls: the smallest face offset (0 without planes)
    auto inscribed = [&](int kind, const double* cc, int hull) {
        double r = 0.0;
        if (kind == K_BOX) r = std::min(cc[0], std::min(cc[1], cc[2]));
        else if (kind == K_CYL) r = std::min(cc[3], cc[0]);
        else if (kind == K_HULL) {
            const int f0 = d->hull_face_begin[hull], f1 = d->hull_face_begin[hull + 1];
            r = f1 > f0 ? INFINITY : 0.0;
            for (int f = f0; f < f1; ++f) r = std::min(r, d->hull_planes[4 * (size_t)f + 3]);
            r *= (1.0 - 1e-9);             // the planes come from a float64 hull computation: stay inside them
        } else if (kind == K_PLANE) return 0.0;
        if (!(r > 0.0)) r = 0.0;
        return r + cc[4];
    };
    t.rs_in.assign(S > 0 ? S : 1, 0.0); t.ws_in.assign(W > 0 ? W : 1, 0.0);
    for (int i = 0; i < S; ++i) t.rs_in[i] = inscribed(t.rs_kind[i], &t.rs_core[6 * (size_t)i], t.rs_hull[i]);
    for (int w = 0; w < W; ++w) t.ws_in[w] = inscribed(t.ws_kind[w], &t.ws_core[18 * (size_t)w + 12], t.ws_hull[w]);
    // hull vertices, each hull's list preceded by its local bounding box (centre, half extents): 6 + 3 n doubles per hull
    t.hull_off.assign(H > 0 ? H : 1, 0);
    for (int h = 0; h < H; ++h) {
        const double* v = d->hull_verts + 3 * (size_t)d->hull_vert_begin[h];
        const int n = d->hull_vert_begin[h + 1] - d->hull_vert_begin[h];
        t.hull_blob.insert(t.hull_blob.end(), &t.hull_obb[6 * h], &t.hull_obb[6 * h] + 6);
        t.hull_off[h] = t.hull_blob.size();
        t.hull_blob.insert(t.hull_blob.end(), v, v + 3 * (size_t)n);
    }
}

// every table of a descriptor that passed desc_check(d, D_ALL); world_radius: non-null for a movable descriptor.  NBK_OK,
// NBK_ERR_UNSUPPORTED beyond a compiled-in limit, NBK_ERR_INVALID (with g_err) for a prismatic joint whose joint_rot is no constant
static int32_t compile_tables(const nbk_model_desc* d, const double* world_radius, ModelTables& t) {
    compile_geometry(d, t);
    { const int32_t rc = check_limits(d, t); if (rc != NBK_OK) return rc; }
    { const int32_t rc = joint_tables(d, t); if (rc != NBK_OK) return rc; }
    queue_groups(d, t);
    float_tables(d, world_radius, t);
    t.spec = bf32_spec_text(d, t, world_radius != nullptr);
    hull_tables(d, t);
    return NBK_OK;
}

}  // namespace nbk
