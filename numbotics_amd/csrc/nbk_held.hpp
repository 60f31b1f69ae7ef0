// nbk_held.hpp -- held objects: a body of 1..8 primitive shapes riding on one link, checked on the device.  Included by nbk.hip after
// nbk_cloud.hpp; DESIGN.md 3, "Held objects".
//
// The world pose of held shape h at configuration q is  F(q) . ((A . G) . L_h):  F(q) the moving frame of the holding link's joint
// (the replay of cloud_shape_frame for the frame's joint mask), A the link's constant pose in that frame, G the grasp (the object in
// the link frame; the stored one, or one per row of the call), L_h the shape in the object's frame.  The two constant products are
// formed per lane by held_locals, xf_mul's expression; nbk_held_locals_host runs the same routine on the host.
//
// A held object is a device object of its own (nbk_held), made against a descriptor like nbk_cloud against nothing: its kernels sit
// beside the validity pipeline and touch none of it.  Its verdict is the held object's ALONE -- held shape h against the world shapes
// of its list and the robot shapes of its set, each pair by the scene's own predicate in the operand order of a descriptor that holds
// the held shapes as robot shapes S .. S+H-1 of the holding frame with the pairs (s, S+h) and (S+h, world w):
//   world w   tc = (thr + margin_h) + margin_w, rs = (tc + rho_h) + rho_w; free unless rs > 0 and |c_h - c_w|^2 < rs^2; a plane is
//             always a candidate and decided by plane_collides(held, plane, thr, rho_h)
//   robot s   tc = (thr + margin_s) + margin_h, rs = (tc + rho_s) + rho_h; free unless rs > 0 and |c_s - c_h|^2 < rs^2
//   then cores_collide_exact with the cores in canonical order (kind ascending; on a tie the descriptor's first operand first).
// The world loop is linear in the list: a grid over many world shapes is a later step.
#pragma once

namespace nbk {

constexpr int HELD_MAX_SHAPES = 8;
constexpr int HELD_SHAPE_LEN = 18;              // per shape: L_h [12] | h0 h1 h2 rad margin rho

struct HeldDev {                                // what the kernels read (by value)
    unsigned mask;                              // joints on the path from the base to the holding frame
    int n_shapes, n_world;
    const double* tab;                          // A [12] | G [12] | n_shapes x HELD_SHAPE_LEN
    const int* kind;                            // [n_shapes] core kinds
    const int* world;                           // [n_world] allowed world shapes, ascending
    CloudSel robot;                             // allowed robot shapes, device order (all == 0)
    int n_items;                                // K: the (held shape, other shape) items of the distance and certified entries
    const int* items;                           // [K][4] held shape | 0 robot, 1 world | device index of the robot shape, or the world
                                                // shape | the robot shape's caller's index (MotionTab's order), or the world shape
};
constexpr int HELD_ITEM_LEN = 4;

// o = a * b for 3x4 poses stored [12] row-major (rows of a 4x4 work as well: only [4 i + j], j < 4, i < 3 is read): xf_mul's
// expression, term for term
__host__ __device__ inline void held_mul12(const double* a, const double* b, double* o) {
    for (int i = 0; i < 3; ++i) {
        const double a0 = a[4 * i], a1 = a[4 * i + 1], a2 = a[4 * i + 2];
        for (int j = 0; j < 3; ++j) o[4 * i + j] = NBK_FMA(a2, b[8 + j], NBK_FMA(a1, b[4 + j], a0 * b[j]));
        o[4 * i + 3] = NBK_FMA(a2, b[11], NBK_FMA(a1, b[7], NBK_FMA(a0, b[3], a[4 * i + 3])));
    }
}
// the local pose of held shape h in the holding frame: (A . G) . L_h
__host__ __device__ inline void held_locals(const double* AG, const double* L, double* out) { held_mul12(AG, L, out); }

// F(q): the joints of `mask`, base first (cloud_shape_frame for a mask instead of a shape).  rows (optional): the lane's column of the
// [J][6][64] joint rows, written through joint_frame_rows for every joint of the mask (what prox_row_masks reads)
NBK_DEV void held_frame(const DevModel& m, unsigned mask, const double* myq, Xf& T, double* rows = nullptr) {
    xf_from12(m.base_pose, T);
    for (int k = 0; k < m.n_joints; ++k) {
        if (((mask >> k) & 1u) == 0u) continue;
        Xf nxt;
        joint_apply(m, k, T, myq[m.joint_qidx[k]], nxt);
        if (rows != nullptr) joint_frame_rows(m, k, nxt, rows + 6 * k * WAVE);
        T = nxt;
    }
}

// core of held shape h from the holding frame F and A . G: build_core's robot branch with the local pose formed here.  A held hull
// has its three axes like a box and the HullRef of its tables (in the held blob) in h[].  HULLS = false leaves the hull case out:
// the hull-free instances of the held-versus-cloud verdict kernels, which are never given a held hull (their entries pick the
// other instance for one), keep the code they had.
template <bool HULLS = true>
NBK_DEV void held_core(const HeldDev& hd, int h, const Xf& F, const double* AG, Core& o) {
    const double* rec = hd.tab + 24 + HELD_SHAPE_LEN * h;
    double loc[12];
    held_locals(AG, rec, loc);
    const double* cc = rec + 12;
    o.kind = hd.kind[h];
    o.h[0] = cc[0]; o.h[1] = cc[1]; o.h[2] = cc[2]; o.rad = cc[3]; o.margin = cc[4]; o.rho = cc[5];
    double Rl[9], tl[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { Rl[3 * i] = loc[4 * i]; Rl[3 * i + 1] = loc[4 * i + 1]; Rl[3 * i + 2] = loc[4 * i + 2]; tl[i] = loc[4 * i + 3]; }
    xf_mul_pos(F, tl, o.c);
    if (o.kind == K_SEG || o.kind == K_CYL) {
        xf_mul_col(F, Rl, 2, o.ax[2]);
    } else if (o.kind == K_BOX || (HULLS && o.kind == K_HULL)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) xf_mul_col(F, Rl, j, o.ax[j]);
    }
}

// o = first ? a : b, member by member (registers stay registers: no core is addressed through a lane-varying pointer)
NBK_DEV void held_pick(bool first, const Core& a, const Core& b, Core& o) {
    o.kind = first ? a.kind : b.kind;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        o.c[e] = first ? a.c[e] : b.c[e];
        o.h[e] = first ? a.h[e] : b.h[e];
#pragma unroll
        for (int j = 0; j < 3; ++j) o.ax[j][e] = first ? a.ax[j][e] : b.ax[j][e];
    }
    o.rad = first ? a.rad : b.rad;
    o.margin = first ? a.margin : b.margin;
    o.rho = first ? a.rho : b.rho;
}

// the pair predicate past the bounding spheres for (P, Q) in the descriptor's operand order, neither a plane
NBK_DEV bool held_collides(const Core& P, const Core& Q, double tc) {
    const bool keep = !(P.kind > Q.kind);
    Core A, Bc;
    held_pick(keep, P, Q, A);
    held_pick(keep, Q, P, Bc);
    return cores_collide_exact(A, Bc, tc);
}

// The walk: does the held object at the lane's staged row `myq` with the grasp `grasp_row` (12 values of a 3x4, or the first three rows
// of a 4x4) touch an allowed world or robot shape?  Called by every lane of the wave (`active`: this lane has a row; `hit`: its
// verdict so far, raised here -- a lane that comes in with a hit, or without a row, only keeps the ballots company).  Two stages per
// held shape and list, as cloud_row_hits: each lane runs ahead to its next candidate that passes the bounding spheres, then the lanes
// that hold one decide theirs side by side.
NBK_DEV void held_row_hits(const DevModel& m, const HeldDev& hd, const double* grasp_row, double thr, const double* myq, bool active,
                           bool& hit) {
    if (__builtin_amdgcn_ballot_w64(active && !hit) == 0ull) return;
    Xf F;
    double AG[12];
    if (active && !hit) {
        held_frame(m, hd.mask, myq, F);
        double G[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) G[e] = grasp_row[e];
        held_mul12(hd.tab, G, AG);
    }
    Xf T;
    int cur_frame = -2;                                  // per lane: the frame T holds
    for (int h = 0; h < hd.n_shapes; ++h) {
        const bool work = active && !hit;
        if (__builtin_amdgcn_ballot_w64(work) == 0ull) break;
        Core Hc;
        cloud_core_init(Hc);
        if (work) held_core(hd, h, F, AG, Hc);
        // ---- the world list
        int i = 0;
        while (true) {
            bool cand = false;
            int w = 0;
            double tc = 0.0;
            while (work && !hit && !cand && i < hd.n_world) {
                w = hd.world[i++];
                if (m.ws_kind[w] == K_PLANE) { cand = true; break; }
                const double* wc = m.ws_core + 18 * (size_t)w;
                tc = (thr + Hc.margin) + wc[16];
                const double rs = (tc + Hc.rho) + wc[17];
                double dl[3];
                sub3(Hc.c, wc, dl);
                cand = rs > 0.0 && dot3(dl, dl) < rs * rs;
            }
            if (__builtin_amdgcn_ballot_w64(cand) == 0ull) break;
            if (cand) {
                Core Wc;
                cloud_core_init(Wc);
                load_wcore(m, w, Wc);
                if (Wc.kind == K_PLANE) { if (plane_collides(Hc, Wc, thr, Hc.rho)) hit = true; }
                else if (held_collides(Hc, Wc, tc)) hit = true;
            }
        }
        // ---- the robot set (device order)
        int s = 0;
        while (true) {
            bool cand = false;
            double tc = 0.0;
            Core A;
            cloud_core_init(A);
            while (work && !hit && !cand && s < m.n_rshapes) {
                const int sc = s++;
                if (!cloud_selected(hd.robot, sc)) continue;
                if (m.rs_frame[sc] != cur_frame) { cloud_shape_frame(m, sc, myq, T); cur_frame = m.rs_frame[sc]; }
                build_core(m, sc, T, A);
                tc = (thr + A.margin) + Hc.margin;
                const double rs = (tc + A.rho) + Hc.rho;
                double dl[3];
                sub3(A.c, Hc.c, dl);
                cand = rs > 0.0 && dot3(dl, dl) < rs * rs;
            }
            if (__builtin_amdgcn_ballot_w64(cand) == 0ull) break;
            if (cand && held_collides(A, Hc, tc)) hit = true;
        }
    }
}

// the lane's grasp row: the stored one (rows == 0), the call's one row (1) or row b of B; `fin`: every value read is finite
NBK_DEV const double* held_grasp_row(const HeldDev& hd, const double* __restrict__ grasp, int grasp_rows, int64_t b, bool& fin) {
    const double* g = grasp_rows == 0 ? hd.tab + 12 : (grasp_rows == 1 ? grasp : grasp + 16 * b);
    fin = true;
#pragma unroll
    for (int e = 0; e < 12; ++e) fin = fin && (g[e] - g[e] == 0.0);
    return g;
}

// verdict of row b = the walk's, or 1 for a non-finite q or grasp row or a set world status (wstatus: the movable descriptor's, else
// null).  A workgroup owns one mask word, so the word and the bytes have one writer each.
__global__ __launch_bounds__(64) void k_held_validity(DevModel m, HeldDev hd, const int* __restrict__ wstatus, const double* __restrict__ q,
                                                      int64_t B, const double* __restrict__ grasp, int grasp_rows, double thr,
                                                      int accumulate, unsigned long long* __restrict__ mask_bits,
                                                      uint8_t* __restrict__ mask_bytes) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * WAVE + lane;
    const bool active = b < B;
    double* myq = lds + lane * m.n_q;
    const bool wbad = wstatus != nullptr && *wstatus != 0;
    bool hit = false;
    const double* grow = hd.tab + 12;
    if (active) {
        bool gfin = true;
        grow = held_grasp_row(hd, grasp, grasp_rows, b, gfin);
        hit = !cloud_stage_q(q, b, m.n_q, myq) || !gfin || wbad;
    }
    if (!wbad) held_row_hits(m, hd, grow, thr, myq, active, hit);
    const unsigned long long word = __builtin_amdgcn_ballot_w64(active && hit);
    if (mask_bits != nullptr && lane == 0) {
        if (accumulate) { if (word != 0ull) mask_bits[blockIdx.x] |= word; }
        else mask_bits[blockIdx.x] = word;
    }
    if (mask_bytes != nullptr && active) {
        if (!accumulate) mask_bytes[b] = hit ? 1 : 0;
        else if (hit) mask_bytes[b] = 1;
    }
}

// ---- sampled edges with the held object (nbk_edge_held_validity_batch): k_cloud_edges with the held walk in the cloud walk's place.
// valid[e] before the walk is k_cloud_edges_init's; one grasp per call; a non-finite grasp or a set world status makes every
// non-degenerate edge invalid.
__global__ __launch_bounds__(64) void k_held_edges(DevModel m, HeldDev hd, const int* __restrict__ wstatus, EdgeSrc es,
                                                   const unsigned long long* __restrict__ offs, int64_t E,
                                                   const double* __restrict__ grasp, int grasp_rows, double thr, uint8_t* valid) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    double* myq = lds + lane * m.n_q;
    const unsigned long long total = offs[E];
    bool gfin = true;
    const double* grow = held_grasp_row(hd, grasp, grasp_rows, 0, gfin);
    const bool bad = !gfin || (wstatus != nullptr && *wstatus != 0);
    for (unsigned long long base = (unsigned long long)blockIdx.x * WAVE; base < total; base += (unsigned long long)gridDim.x * WAVE) {
        const unsigned long long f = base + (unsigned long long)lane;
        int64_t e = 0;
        bool work = false;
        if (f < total) {
            e = cloud_flat_owner(offs, E, f);
            if (__hip_atomic_load(valid + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                edge_sample_row(es, ((unsigned long long)e << 32) | (f - offs[e]), m.n_q, myq, 1);
                work = !row_nonfinite(myq, m.n_q, 1) && !bad;
                if (!work) __hip_atomic_store(valid + e, (uint8_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        bool hit = false;
        if (!bad) held_row_hits(m, hd, grow, thr, myq, work, hit);
        if (hit) __hip_atomic_store(valid + e, (uint8_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- sampled B-spline trajectories with the held object (nbk_spline_held_validity_batch): k_cloud_spline with the held walk in the
// cloud walk's place -- the same plan, scan, first-hit key (SPC_*) and accumulate rules; k_cloud_spline_init (hold: the world status
// of a movable descriptor, else null) and k_cloud_spline_final are the cloud's.  One grasp per call; a non-finite one hits every
// sample that is looked at, so every trajectory that has samples is hit at its first.
template <int K>
__global__ __launch_bounds__(64) void k_held_spline(DevModel m, HeldDev hd, const double* __restrict__ ctrl, int n,
                                                    const double* __restrict__ knots, const double* __restrict__ plan,
                                                    const unsigned long long* __restrict__ offs, int64_t S,
                                                    const double* __restrict__ grasp, int grasp_rows, double thr,
                                                    const double* __restrict__ t_prev, unsigned long long* first) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    double* myq = lds + lane * m.n_q;
    const unsigned long long total = offs[S];
    bool gfin = true;
    const double* grow = held_grasp_row(hd, grasp, grasp_rows, 0, gfin);
    for (unsigned long long base = (unsigned long long)blockIdx.x * WAVE; base < total; base += (unsigned long long)gridDim.x * WAVE) {
        const unsigned long long f = base + (unsigned long long)lane;
        int64_t s = 0;
        unsigned long long j = 0ull;
        bool work = false, hit = false;
        if (f < total) {
            s = cloud_flat_owner(offs, S, f);
            j = f - offs[s];
            const unsigned long long key = __hip_atomic_load(first + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (key <= SPC_NONE && j + 1ull < key) {
                const double jd = (double)j;
                const double t = jd < plan[2 * s + 1] ? jd * plan[2 * s] : 1.0;
                if (t_prev == nullptr || !(t >= t_prev[s])) {
                    const int ell = spline_span<K>(knots, n, t);
                    const double* cp = ctrl + ((size_t)s * (size_t)n + (size_t)(ell - K)) * m.n_q;
                    de_boor<K>(m.n_q, cp, knots, ell, t, [&](int c, double v) { myq[c] = v; });
                    work = gfin && !row_nonfinite(myq, m.n_q, 1);
                    hit = !work;                             // a non-finite sample, or grasp, collides
                }
            }
        }
        if (gfin) held_row_hits(m, hd, grow, thr, myq, work, hit);
        if (hit) atomicMin(first + s, j + 1ull);
    }
}

// ---- the held object against a point cloud (nbk_held_cloud_*): the held shapes in the robot shapes' place of the cloud's kernels.
// The verdict is the OR over (held shape h, point i) of the pair predicate for (robot shape, sphere world shape of the cloud's radius
// at p_i) in cloud_row_hits' operand order: tc = (thr + margin_h) + radius, rs = (tc + rho_h) + 0, free unless rs > 0 and
// |c_h - p|^2 < rs^2, then cloud_collides(P, Hc, tc) with the point core first -- the bits of a descriptor that holds the held shapes
// as robot shapes S + h of the holding frame and the points as sphere world shapes, with the pairs (S + h, p_i).  This is the
// held-versus-cloud term ALONE: no world shape and no link takes part, the world status is not read, and the attachment's world
// list and robot set play no part.

// cloud_collides(P, Hc, tc) for a point core P and a held core Hc that is NO hull.  There cloud_collides is
// cores_collide_exact, and for a point core first and a second core that is no hull cores_collide_pre decides EVERY pair -- box
// cores in its midphase or, like cylinder cores, in its last statement (point_solid), point and segment cores in ps_closest -- and never
// answers -1: cores_collide_exact returns `pre != 0` there, bit for bit.  Calling the routine that decides keeps the three GJK
// walks behind it out of these kernels (their scratch arrays and spills with them).  (-1 cannot come; it would read "collides".)
NBK_DEV bool held_cloud_collides(const Core& P, const Core& Hc, double tc) { return cores_collide_pre(P, Hc, tc) != 0; }

// The walk: cloud_row_hits with held_core in build_core's place.  Called by every lane of the wave (`active`, `hit` as in
// held_row_hits); the caller has checked that the cloud holds points and that its status is clear.  HULLS = false is the walk of an
// attachment without a hull, statement for statement what it was before hulls were served: held_cloud_collides decides every
// pair and no GJK walk is compiled in.  HULLS = true serves an attachment that holds a hull: the loop over h is wave-uniform, so
// every working lane holds THIS held shape -- a hull core takes the scalar-cache path (rad = -1.0, as in cloud_row_hits) and is
// decided by cloud_collides (which, for a hull at tc <= 0, goes straight to gjk_collides: hull_box_far's deviation there does not
// apply), a primitive shape of the same attachment by held_cloud_collides as before; hd.kind[h] is a uniform load, the branch a
// uniform one.
template <bool HULLS>
NBK_DEV void held_cloud_row_hits(const DevModel& m, const HeldDev& hd, const CloudDev& cd, const double* grasp_row, double radius,
                                 double thr, const double* myq, bool active, bool& hit) {
    if (__builtin_amdgcn_ballot_w64(active && !hit) == 0ull) return;
    Core P;
    cloud_point_core(radius, P);
    Xf F;
    double AG[12];
    if (active && !hit) {
        held_frame(m, hd.mask, myq, F);
        double G[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) G[e] = grasp_row[e];
        held_mul12(hd.tab, G, AG);
    }
    for (int h = 0; h < hd.n_shapes; ++h) {
        const bool work = active && !hit;
        if (__builtin_amdgcn_ballot_w64(work) == 0ull) break;
        Core Hc;
        cloud_core_init(Hc);
        double tc = 0.0, rs = 0.0;
        if (work) {
            held_core<HULLS>(hd, h, F, AG, Hc);
            if (HULLS && Hc.kind == K_HULL) Hc.rad = -1.0;      // every working lane holds this hull: the scalar cache serves its vertices
            tc = (thr + Hc.margin) + radius;
            rs = (tc + Hc.rho) + 0.0;
        }
        CloudWalk w;
        cloud_walk_begin(cd, work, Hc.c, rs, w);
        const double rs2 = rs * rs;
        while (true) {
            // (cloud_row_hits' two stages: run ahead to the next point inside the bounding sphere, decide side by side)
            bool cand = false;
            while (!hit && !cand && cloud_walk_next(cd, w)) {
                const double* p = cd.pts + 3 * (size_t)w.cur;
                ++w.cur;
                P.c[0] = p[0]; P.c[1] = p[1]; P.c[2] = p[2];
                double dc[3];
                sub3(Hc.c, P.c, dc);
                cand = dot3(dc, dc) < rs2;
            }
            if (__builtin_amdgcn_ballot_w64(cand) == 0ull) break;
            if constexpr (HULLS) {
                if (hd.kind[h] == K_HULL) { if (cand && cloud_collides(P, Hc, tc)) hit = true; }
                else if (cand && held_cloud_collides(P, Hc, tc)) hit = true;
            } else {
                if (cand && held_cloud_collides(P, Hc, tc)) hit = true;
            }
        }
    }
}

// verdict of row b = the walk's, or 1 for a non-finite q or grasp row or a set cloud status; an empty cloud is free.  k_held_validity's
// frame: a workgroup owns one mask word, so the word and the bytes have one writer each.  HULLS: the walk's instance (the entry picks
// it by nbk_held.has_hull).
template <bool HULLS>
__global__ __launch_bounds__(64) void k_held_cloud_validity(DevModel m, HeldDev hd, CloudDev cd, const double* __restrict__ q, int64_t B,
                                                            const double* __restrict__ grasp, int grasp_rows, double thr, int accumulate,
                                                            unsigned long long* __restrict__ mask_bits, uint8_t* __restrict__ mask_bytes) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * WAVE + lane;
    const bool active = b < B;
    double* myq = lds + lane * m.n_q;
    const int status = cd.hdr->status;
    const int n = cd.hdr->n;
    const double radius = cd.hdr->radius;
    bool hit = false;
    const double* grow = hd.tab + 12;
    if (active) {
        bool gfin = true;
        grow = held_grasp_row(hd, grasp, grasp_rows, b, gfin);
        hit = !cloud_stage_q(q, b, m.n_q, myq) || !gfin || status != 0;
    }
    if (n > 0 && status == 0) held_cloud_row_hits<HULLS>(m, hd, cd, grow, radius, thr, myq, active, hit);
    const unsigned long long word = __builtin_amdgcn_ballot_w64(active && hit);
    if (mask_bits != nullptr && lane == 0) {
        if (accumulate) { if (word != 0ull) mask_bits[blockIdx.x] |= word; }
        else mask_bits[blockIdx.x] = word;
    }
    if (mask_bytes != nullptr && active) {
        if (!accumulate) mask_bytes[b] = hit ? 1 : 0;
        else if (hit) mask_bytes[b] = 1;
    }
}

// k_cloud_clearance with the held shapes in the robot shapes' place: per row the minimum over (h, i) of the signed distance, reported
// below d_max with the held shape index and the original point index (ties: the smallest h, then the smallest point); NaN, -1, -1
// for a non-finite q or grasp row or a set status; +inf, -1, -1 when nothing is nearer than d_max.
__global__ __launch_bounds__(64) void k_held_cloud_clearance(DevModel m, HeldDev hd, CloudDev cd, const double* __restrict__ q, int64_t B,
                                                             const double* __restrict__ grasp, int grasp_rows, double d_max,
                                                             double* __restrict__ out_d, int32_t* __restrict__ out_s,
                                                             int32_t* __restrict__ out_p) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * WAVE + lane;
    const bool active = b < B;
    double* myq = lds + lane * m.n_q;
    const int status = cd.hdr->status;
    const int n = cd.hdr->n;
    const double radius = cd.hdr->radius;
    bool ok = false;
    const double* grow = hd.tab + 12;
    if (active) {
        bool gfin = true;
        grow = held_grasp_row(hd, grasp, grasp_rows, b, gfin);
        ok = cloud_stage_q(q, b, m.n_q, myq) && gfin && status == 0;
    }
    double best = NBK_INF;
    int bs = -1, bi = -1;
    if (n > 0 && status == 0 && __builtin_amdgcn_ballot_w64(ok) != 0ull) {
        Core P;
        cloud_point_core(radius, P);
        Xf F;
        double AG[12];
        if (ok) {
            held_frame(m, hd.mask, myq, F);
            double G[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) G[e] = grow[e];
            held_mul12(hd.tab, G, AG);
        }
        for (int h = 0; h < hd.n_shapes; ++h) {
            Core Hc;
            cloud_core_init(Hc);
            if (ok) {
                held_core(hd, h, F, AG, Hc);
                if (Hc.kind == K_HULL) Hc.rad = -1.0;      // h is wave-uniform: every working lane holds this hull (k_cloud_clearance's rule)
            }
            cloud_core_clearance(cd, Hc, P, radius, ok, h, d_max, best, bs, bi);
        }
    }
    if (active) {
        out_d[b] = ok ? best : __builtin_nan("");
        if (out_s != nullptr) out_s[b] = ok ? bs : -1;
        if (out_p != nullptr) out_p[b] = ok ? bi : -1;
    }
}

// ---- proximity records of the held object against the cloud (nbk_held_cloud_records_batch): k_cloud_records with the held shapes in
// the robot shapes' place, in its two phases.
//   1. the winner: k_held_cloud_clearance's loop, cloud_core_clearance keeping the winner's slot in the sorted arrays.  PER_SHAPE =
//      true has the grid (ceil(B / 64), H) with blockIdx.y = h -- a wave holds ONE held shape, every item starts from a fresh `best`
//      -- and writes column h of [B][H].
//   2. the record, for the lanes that hold a winner and only when a witness or a row is asked for: the holding frame once more (the
//      same joint_apply sequence, so the same frame bits), with joint_frame_rows into the [J][6][64] LDS rows when rows are asked
//      for; held_core of the winning shape (a hull through per-lane loads: the lanes' winners may differ); cores_distance<true, true> and epa_refine<true> on (held core, point core) --
//      item_distance's statements for a (robot shape, sphere world shape) pair; prox_row_masks with the holding frame's mask and 0.
//      The distance this phase finds is the one reported where it runs: the bits of phase 1.
// Nothing nearer than d_max: +inf, -1, -1, NaN witness, a row of +0.0.  A non-finite q or grasp row or a set status: NaN, -1, -1, NaN,
// NaN.  LDS: PairItemsLds -- [64][n_q] q rows | [J][6][64] joint rows when rows are asked for.
template <bool PER_SHAPE>
__global__ __launch_bounds__(64) void k_held_cloud_records(DevModel m, HeldDev hd, CloudDev cd, const double* __restrict__ q, int64_t B,
                                                           const double* __restrict__ grasp, int grasp_rows, double d_max,
                                                           double* __restrict__ out_d, int32_t* __restrict__ out_s,
                                                           int32_t* __restrict__ out_p, double* __restrict__ out_w,
                                                           double* __restrict__ out_j) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * WAVE + lane;
    const bool active = b < B;
    const PairItemsLds L(m.n_q);
    double* myq = L.q(lds) + lane * m.n_q;
    const int h0 = PER_SHAPE ? (int)blockIdx.y : 0, h1 = PER_SHAPE ? h0 + 1 : hd.n_shapes;
    if (h0 >= hd.n_shapes) return;
    const int status = cd.hdr->status;
    const int n = cd.hdr->n;
    const double radius = cd.hdr->radius;
    bool ok = false;
    const double* grow = hd.tab + 12;
    if (active) {
        bool gfin = true;
        grow = held_grasp_row(hd, grasp, grasp_rows, b, gfin);
        ok = cloud_stage_q(q, b, m.n_q, myq) && gfin && status == 0;
    }
    double best = NBK_INF;
    int bs = -1, bi = -1;
    unsigned slot = 0u;
    Core P;
    cloud_point_core(radius, P);
    double AG[12];
    if (n > 0 && status == 0 && __builtin_amdgcn_ballot_w64(ok) != 0ull) {
        Xf F;
        if (ok) {
            held_frame(m, hd.mask, myq, F);
            double G[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) G[e] = grow[e];
            held_mul12(hd.tab, G, AG);
        }
        for (int h = h0; h < h1; ++h) {
            Core Hc;
            cloud_core_init(Hc);
            if (ok) {
                held_core(hd, h, F, AG, Hc);
                if (Hc.kind == K_HULL) Hc.rad = -1.0;      // h is wave-uniform here, in the dense loop and with blockIdx.y = h
            }
            cloud_core_clearance(cd, Hc, P, radius, ok, h, d_max, best, bs, bi, &slot);
        }
    }
    const bool win = ok && bs >= 0;
    double wit[9];
    if ((out_w != nullptr || out_j != nullptr) && win) {
        Xf F;
        held_frame(m, hd.mask, myq, F, out_j != nullptr ? L.jz(lds) + lane : nullptr);
        Core Hc;
        cloud_core_init(Hc);
        // (each lane builds the core of its OWN winner and the lanes may differ: a hull keeps its per-lane vertex loads here, rad
        // stays as the tables have it; the comparisons and the vertex are those of the scalar-cache path, so the bits are phase 1's)
        held_core(hd, bs, F, AG, Hc);
        const double* p = cd.pts + 3 * (size_t)slot;
        P.c[0] = p[0]; P.c[1] = p[1]; P.c[2] = p[2];
        double fam = -1.0;
        double d = cores_distance<true, true>(Hc, P, wit, &fam);
        if (fam >= 0.0) epa_refine<true>(Hc, P, fam, d, wit);
        best = d;
    }
    if (!active) return;
    const int64_t o = PER_SHAPE ? b * hd.n_shapes + h0 : b;
    const double nan = __builtin_nan("");
    out_d[o] = ok ? best : nan;
    if (out_s != nullptr) out_s[o] = ok ? bs : -1;
    if (out_p != nullptr) out_p[o] = ok ? bi : -1;
    if (out_w != nullptr) {
#pragma unroll
        for (int e = 0; e < 9; ++e) out_w[o * 9 + e] = win ? wit[e] : nan;
    }
    if (out_j != nullptr) {
        if (win) prox_row_masks(m, L.jz(lds), lane, hd.mask, 0u, wit, out_j + o * m.n_q);
        else for (int c = 0; c < m.n_q; ++c) out_j[o * m.n_q + c] = ok ? 0.0 : nan;
    }
}

// k_cloud_edges with the held walk against the cloud (nbk_edge_held_cloud_validity_batch): the plan, the scan and k_cloud_edges_init
// are the cloud's.  One grasp per call; a non-finite grasp or a set cloud status makes every non-degenerate edge invalid.
template <bool HULLS>
__global__ __launch_bounds__(64) void k_held_cloud_edges(DevModel m, HeldDev hd, CloudDev cd, EdgeSrc es,
                                                         const unsigned long long* __restrict__ offs, int64_t E,
                                                         const double* __restrict__ grasp, int grasp_rows, double thr, uint8_t* valid) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    double* myq = lds + lane * m.n_q;
    const unsigned long long total = offs[E];
    const int status = cd.hdr->status;
    const int n = cd.hdr->n;
    const double radius = cd.hdr->radius;
    bool gfin = true;
    const double* grow = held_grasp_row(hd, grasp, grasp_rows, 0, gfin);
    const bool bad = !gfin || status != 0;
    for (unsigned long long base = (unsigned long long)blockIdx.x * WAVE; base < total; base += (unsigned long long)gridDim.x * WAVE) {
        const unsigned long long f = base + (unsigned long long)lane;
        int64_t e = 0;
        bool work = false;
        if (f < total) {
            e = cloud_flat_owner(offs, E, f);
            if (__hip_atomic_load(valid + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                edge_sample_row(es, ((unsigned long long)e << 32) | (f - offs[e]), m.n_q, myq, 1);
                work = !row_nonfinite(myq, m.n_q, 1) && !bad;
                if (!work) __hip_atomic_store(valid + e, (uint8_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        bool hit = false;
        if (n > 0 && !bad) held_cloud_row_hits<HULLS>(m, hd, cd, grow, radius, thr, myq, work, hit);
        if (hit) __hip_atomic_store(valid + e, (uint8_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// k_cloud_spline with the held walk against the cloud and the call's grasp (nbk_spline_held_cloud_validity_batch): the same plan,
// scan, first-hit key (SPC_*) and accumulate rules; k_cloud_spline_init (hold: the cloud's status) and k_cloud_spline_final are the
// cloud's.  A non-finite grasp hits every sample that is looked at, as in k_held_spline.
template <int K, bool HULLS>
__global__ __launch_bounds__(64) void k_held_cloud_spline(DevModel m, HeldDev hd, CloudDev cd, const double* __restrict__ ctrl, int n,
                                                          const double* __restrict__ knots, const double* __restrict__ plan,
                                                          const unsigned long long* __restrict__ offs, int64_t S,
                                                          const double* __restrict__ grasp, int grasp_rows, double thr,
                                                          const double* __restrict__ t_prev, unsigned long long* first) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    double* myq = lds + lane * m.n_q;
    const unsigned long long total = offs[S];
    const int ncl = cd.hdr->n;
    const double radius = cd.hdr->radius;
    bool gfin = true;
    const double* grow = held_grasp_row(hd, grasp, grasp_rows, 0, gfin);
    for (unsigned long long base = (unsigned long long)blockIdx.x * WAVE; base < total; base += (unsigned long long)gridDim.x * WAVE) {
        const unsigned long long f = base + (unsigned long long)lane;
        int64_t s = 0;
        unsigned long long j = 0ull;
        bool work = false, hit = false;
        if (f < total) {
            s = cloud_flat_owner(offs, S, f);
            j = f - offs[s];
            const unsigned long long key = __hip_atomic_load(first + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (key <= SPC_NONE && j + 1ull < key) {
                const double jd = (double)j;
                const double t = jd < plan[2 * s + 1] ? jd * plan[2 * s] : 1.0;
                if (t_prev == nullptr || !(t >= t_prev[s])) {
                    const int ell = spline_span<K>(knots, n, t);
                    const double* cp = ctrl + ((size_t)s * (size_t)n + (size_t)(ell - K)) * m.n_q;
                    de_boor<K>(m.n_q, cp, knots, ell, t, [&](int c, double v) { myq[c] = v; });
                    work = gfin && !row_nonfinite(myq, m.n_q, 1);
                    hit = !work;                             // a non-finite sample, or grasp, collides
                }
            }
        }
        if (ncl > 0 && gfin) held_cloud_row_hits<HULLS>(m, hd, cd, grow, radius, thr, myq, work, hit);
        if (hit) atomicMin(first + s, j + 1ull);
    }
}

// ---- held items: one (held shape h, other shape) pair each, in the order of the pair list of a descriptor that holds the held
// shapes as robot shapes S + h: (s, S + h) for the allowed robot shapes s in the caller's order, then h; then (S + h, world w) for h,
// then the allowed world shapes.  HeldDev.items holds them (held_item_list, made once by nbk_held_create).

// The record of item `it` at the lane's staged row `myq` with the grasp `grasp_row`: item_distance's statements on the held core and
// the other shape's, in the descriptor's operand order (robot shape first, held shape second; held shape first, world shape
// second) -- the signed distance, and in wit[9] the point on the first, the point on the second and the unit normal from the second
// to the first.  Every lane of the wave calls it; lanes with ok == false replay nothing, get NaN and leave wit alone.  The two
// frames are replayed from the base, each along its own mask: common ancestors give the same bits on either path.  rows (optional):
// the lane's column of the [J][6][64] joint rows; every joint of either mask is written (a common ancestor twice, the same bits),
// which is what prox_row_masks reads for this item.
NBK_DEV double held_item_record(const DevModel& m, const HeldDev& hd, const double* grasp_row, const double* myq, bool ok, int it,
                                double* rows, double* wit) {
    // the hull support's scalar-cache path (rad < 0) needs every running lane to hold the same hull: only for item-uniform waves
    const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok);
    const int it0 = __shfl(it, okm != 0ull ? __builtin_ctzll(okm) : 0);
    const bool uniform = __builtin_amdgcn_ballot_w64(ok && it != it0) == 0ull;
    if (!ok) return __builtin_nan("");
    const int* rec = hd.items + HELD_ITEM_LEN * it;
    const int h = rec[0], idx = rec[2];
    const bool robot = rec[1] == 0;
    Xf F;
    held_frame(m, hd.mask, myq, F, rows);
    double G[12], AG[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) G[e] = grasp_row[e];
    held_mul12(hd.tab, G, AG);
    Core Hc, Oc;
    cloud_core_init(Hc);
    cloud_core_init(Oc);
    held_core(hd, h, F, AG, Hc);
    if (robot) {
        Xf T;
        held_frame(m, m.rs_mask[idx], myq, T, rows);      // (cloud_shape_frame's statements)
        build_core(m, idx, T, Oc);
    } else {
        load_wcore(m, idx, Oc);
    }
    Core A, Bc;
    held_pick(robot, Oc, Hc, A);
    held_pick(robot, Hc, Oc, Bc);
    if (uniform && A.kind == K_HULL) A.rad = -1.0;
    if (uniform && Bc.kind == K_HULL) Bc.rad = -1.0;
    double fam = -1.0;
    double d = cores_distance<true, true>(A, Bc, wit, &fam);
    if (fam >= 0.0) epa_refine<true>(A, Bc, fam, d, wit);
    return d;
}

// the signed distance alone (k_held_distances, the certified lanes)
NBK_DEV double held_item_distance(const DevModel& m, const HeldDev& hd, const double* grasp_row, const double* myq, bool ok, int it) {
    double wit[9];
    return held_item_record(m, hd, grasp_row, myq, ok, it, nullptr, wit);
}

// one (row, item) per lane, item-major (a wave holds one item unless it straddles two): out_d[b][it], NaN where the q row or the
// grasp row is not finite or the world status is set
__global__ __launch_bounds__(64) void k_held_distances(DevModel m, HeldDev hd, const int* __restrict__ wstatus, const double* __restrict__ q,
                                                       int64_t B, const double* __restrict__ grasp, int grasp_rows,
                                                       double* __restrict__ out_d) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * WAVE + lane;
    const bool live = i < B * (int64_t)hd.n_items;
    const int it = live ? (int)(i / B) : 0;
    const int64_t b = live ? i - (int64_t)it * B : 0;
    double* myq = lds + lane * m.n_q;
    const bool wbad = wstatus != nullptr && *wstatus != 0;
    bool ok = false;
    const double* grow = hd.tab + 12;
    if (live) {
        bool gfin = true;
        grow = held_grasp_row(hd, grasp, grasp_rows, b, gfin);
        ok = cloud_stage_q(q, b, m.n_q, myq) && gfin && !wbad;
    }
    const double d = held_item_distance(m, hd, grow, myq, ok, it);
    if (live) out_d[b * hd.n_items + it] = d;
}

// ---- records of held items (nbk_held_records_batch, nbk_held_records_items): the distance of k_held_distances with the witness and
// the gradient row -- what k_distances<3> / k_pair_items give for the pair of the item on a descriptor that holds the held shapes as
// robot shapes S + h.  One (row, item) per lane.  LISTED = false: the item-major dense index of k_held_distances, outputs [B][K],
// [B][K][9], [B][K][n_q].  LISTED = true: items [N][2] = (row of q, item), outputs [N], [N][9], [N][n_q]; an entry outside
// [0, B) x [0, K) reads nothing and writes NaN to every field.  The row is prox_row_masks over the joint rows the replay leaves in
// LDS: a robot item (s, S + h) has the link shape as subject (rs_mask[s]) and the held shape as target (hd.mask); a world item
// (S + h, w) the held shape as subject and no target mask.  Every field is NaN where the q row or the grasp row is not finite or the
// world status is set.  LDS: PairItemsLds -- [64][n_q] q rows | [J][6][64] joint rows when rows are asked for.
template <bool LISTED>
__global__ __launch_bounds__(64) void k_held_records(DevModel m, HeldDev hd, const int* __restrict__ wstatus, const double* __restrict__ q,
                                                     int64_t B, const int32_t* __restrict__ items, int64_t N,
                                                     const double* __restrict__ grasp, int grasp_rows, double* __restrict__ out_d,
                                                     double* __restrict__ out_w, double* __restrict__ out_j) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * WAVE + lane;
    const int64_t K = hd.n_items;
    const bool live = i < (LISTED ? N : B * K);
    bool in = false;
    int it = 0;
    int64_t b = 0;
    if (live) {
        if constexpr (LISTED) {
            const long long bl = items[2 * i];
            const int il = items[2 * i + 1];
            in = bl >= 0 && bl < B && il >= 0 && il < K;
            if (in) { b = bl; it = il; }
        } else {
            it = (int)(i / B);
            b = i - (int64_t)it * B;
            in = true;
        }
    }
    const PairItemsLds L(m.n_q);
    double* myq = L.q(lds) + lane * m.n_q;
    double* rows = out_j != nullptr ? L.jz(lds) + lane : nullptr;
    const bool wbad = wstatus != nullptr && *wstatus != 0;
    bool ok = false;
    const double* grow = hd.tab + 12;
    if (in) {
        bool gfin = true;
        grow = held_grasp_row(hd, grasp, grasp_rows, b, gfin);
        ok = cloud_stage_q(q, b, m.n_q, myq) && gfin && !wbad;
    }
    double wit[9];
    const double d = held_item_record(m, hd, grow, myq, ok, it, rows, wit);
    if (!live) return;
    const int64_t o = LISTED ? i : b * K + it;
    if (!ok) {
        const double nan = __builtin_nan("");
        out_d[o] = nan;
        if (out_w != nullptr) for (int e = 0; e < 9; ++e) out_w[o * 9 + e] = nan;
        if (out_j != nullptr) for (int c = 0; c < m.n_q; ++c) out_j[o * m.n_q + c] = nan;
        return;
    }
    out_d[o] = d;
    if (out_w != nullptr) {
#pragma unroll
        for (int e = 0; e < 9; ++e) out_w[o * 9 + e] = wit[e];
    }
    if (out_j != nullptr) {
        const int* rec = hd.items + HELD_ITEM_LEN * it;
        const bool robot = rec[1] == 0;
        prox_row_masks(m, L.jz(lds), lane, robot ? m.rs_mask[rec[2]] : hd.mask, robot ? hd.mask : 0u, wit, out_j + o * m.n_q);
    }
}

// ---- the motion bound of a held item: pair_motion_bound's bits for that pair on a descriptor whose shape tables hold, for S + h,
// the holding frame's joint mask, the norm of the translation of (A . G) . L_h and rho + margin
__host__ __device__ inline MotionShape held_motion_shape(unsigned mask, const double* tab, const double* grasp_row, int h) {
    const double* rec = tab + 24 + HELD_SHAPE_LEN * h;
    double G[12], AG[12], loc[12];
    for (int e = 0; e < 12; ++e) G[e] = grasp_row[e];
    held_mul12(tab, G, AG);
    held_locals(AG, rec, loc);
    const double n = __builtin_sqrt(NBK_FMA(loc[11], loc[11], NBK_FMA(loc[7], loc[7], loc[3] * loc[3])));      // (norm3_host's expression)
    return MotionShape{mask, n, rec[17] + rec[16]};
}

// mu of the item `rec` on the trajectory tr.  A robot item counts the joints on one path and not on the other, the robot shape's
// terms first; a world item counts every joint of the holding path.
template <class TR>
__host__ __device__ inline double held_item_motion_bound(const MotionTab& t, unsigned mask, const double* tab, const double* grasp_row,
                                                         const int* rec, const TR& tr) {
    const MotionShape hs = held_motion_shape(mask, tab, grasp_row, rec[0]);
    if (rec[1] != 0) return motion_terms(t, hs, hs.mask, tr, 0.0);
    const int a = rec[3];
    const unsigned ma = t.smask[a];
    const double mu = motion_terms(t, a, ma & ~hs.mask, tr, 0.0);
    return motion_terms(t, hs, hs.mask & ~ma, tr, mu);
}

// ---- certified continuous checks with the held object (nbk_edge_held_continuous_batch, nbk_spline_held_continuous_batch): ca_walk on
// one (trajectory, held item) per lane, item-major.  The init kernels are the scene's; k_held_ca_hold (nbk.hip), behind them, gives
// CA_KEEP_KEY to every non-degenerate trajectory when the world status is set or the call's grasp is not finite (device data both),
// and the walks leave such trajectories alone.

// the linear edge of EdgeLane for one held item (ca_walk's pu and p are both the item)
struct HeldEdgeLane {
    const double* s;
    const double* g;
    double Tf;
    const HeldDev& hd;
    const double* grow;       // the call's grasp row
    double* myq;              // the lane's LDS row
    NBK_DEV double end() const { return Tf; }
    NBK_DEV double span_end() const { return Tf; }
    NBK_DEV double enter(const DevModel& m, int it, double) const {
        return held_item_motion_bound(m.mt, hd.mask, hd.tab, grow, hd.items + HELD_ITEM_LEN * it, EdgeMotion{s, g});
    }
    NBK_DEV double distance(const DevModel& m, bool run, int it, int, double t, double*) const {
        bool ok = false;
        if (run) {
            const double omt = 1.0 - t;
            for (int c = 0; c < m.n_q; ++c) { const double a = omt * s[c]; const double b = t * g[c]; myq[c] = a + b; }
            ok = !row_nonfinite(myq, m.n_q, 1);      // (a non-finite q(t) is answered NaN without a walk: the item stops UNDECIDED there)
        }
        return held_item_distance(m, hd, grow, myq, ok, it);
    }
};

__global__ __launch_bounds__(64) void k_held_edge_ca(DevModel m, HeldDev hd, const double* __restrict__ starts, const double* __restrict__ goals,
                                                     const double* __restrict__ dist, int64_t E, double max_distance, int mode,
                                                     const double* __restrict__ grasp, double thr, int max_iter, double slack,
                                                     unsigned long long* __restrict__ key) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * WAVE + lane;
    const bool live = i < E * (int64_t)hd.n_items;
    const int it = live ? (int)(i / E) : 0;
    const int64_t e = live ? i - (int64_t)it * E : 0;
    HeldEdgeLane tr{starts + e * m.n_q, goals + e * m.n_q, 0.0, hd, grasp != nullptr ? grasp : hd.tab + 12, lds + lane * m.n_q};
    double d_edge = 0.0;
    const bool run = live && edge_span(m.n_q, tr.s, tr.g, dist, e, max_distance, mode, d_edge, tr.Tf) &&
                     __hip_atomic_load(key + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != CA_KEEP_KEY;
    ca_walk(m, tr, run, it, it, lane, thr, max_iter, slack, key + e);
}

// trajectory s of SplineLane<K> for one held item: the trajectory half is SplineLane's
template <int K>
struct HeldSplineLane {
    const double* c;            // control points of the trajectory, [n][nq]
    const double* knots;
    double* row;                // LDS [nq]
    int n, nq, ell;
    const HeldDev& hd;
    const double* grow;
    NBK_DEV double end() const { return 1.0; }
    NBK_DEV double span_end() const { return knots[ell + 1]; }
    NBK_DEV double enter(const DevModel& m, int it, double t) {
        ell = spline_span<K>(knots, n, t);
        return held_item_motion_bound(m.mt, hd.mask, hd.tab, grow, hd.items + HELD_ITEM_LEN * it,
                                      SplineSpanMotion{c + (size_t)(ell - K) * nq, knots + (ell - K + 1), nq, K});
    }
    NBK_DEV double distance(const DevModel& m, bool run, int it, int, double t, double*) const {
        bool ok = false;
        if (run) {
            double* r = row;
            de_boor<K>(nq, c + (size_t)(ell - K) * nq, knots, ell, t, [&](int j, double v) { r[j] = v; });
            ok = !row_nonfinite(row, nq, 1);
        }
        return held_item_distance(m, hd, grow, row, ok, it);
    }
};

template <int K>
__global__ __launch_bounds__(64) void k_held_spline_ca(DevModel m, HeldDev hd, const double* __restrict__ ctrl, int64_t S, int n,
                                                       const double* __restrict__ knots, const double* __restrict__ grasp, double thr,
                                                       int max_iter, double slack, unsigned long long* __restrict__ key) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * WAVE + lane;
    const bool live = i < S * (int64_t)hd.n_items;
    const int it = live ? (int)(i / S) : 0;
    const int64_t s = live ? i - (int64_t)it * S : 0;
    HeldSplineLane<K> tr{ctrl + (size_t)s * (size_t)n * m.n_q, knots, lds + lane * m.n_q, n, m.n_q, K, hd, grasp != nullptr ? grasp : hd.tab + 12};
    const unsigned long long k0 = __hip_atomic_load(key + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool run = live && k0 != CA_DEGENERATE_KEY && k0 != CA_KEEP_KEY;
    ca_walk(m, tr, run, it, it, lane, thr, max_iter, slack, key + s);
}

// ---- certified continuous checks of the held object against a point cloud (nbk_edge_held_cloud_continuous_batch,
// nbk_spline_held_cloud_continuous_batch): ca_walk as it is, on one (trajectory, held shape h) item per lane (ca_walk's pu and p are
// both h).  The grid is (ceil(E / 64), H) with blockIdx.y = h: a wave holds ONE held shape, so Core.kind is wave-uniform as
// cloud_core_clearance needs it (a flat item-major index, as in k_held_edge_ca, would straddle shapes).  LDS: [64][n_q] q rows and
// nothing else.  The init and final kernels are the scene's (hold = the cloud's status, prev when accumulating); k_held_ca_hold,
// behind the init, gives CA_KEEP_KEY to every non-degenerate trajectory when the call's grasp is not finite -- the world status is
// not read.  This is the held-versus-cloud term ALONE, as for the sampled kernels above: no world shape and no link takes part.
//
// The distance half is CloudEdgeLane's with held_core in build_core's place, the frame and core construction k_held_cloud_clearance's.
// The item's motion bound is mu_h = motion_terms over every joint of the holding path (the cloud stands still: the world-item branch
// of held_item_motion_bound, per held shape), and its distance at t the clearance of held shape h ALONE against the cloud at q(t),
// cut at
//     D = min(D_end, D_cap),   D_end = (thr + slack) + mu_h (T_f - t),   D_cap = (thr + slack) + look_ahead:
// the smallest distance below D where there is one; else +inf when D == D_end, else D_cap.  Soundness:
//   * every point of held shape h moves at most mu_h |t' - t| between q(t) and q(t'), and the points of the cloud stand still;
//   * so no point within D_end at t means that the distance stays above thr + slack up to T_f: the item may stop FREE at T_f, which
//     is what ca_walk makes of +inf (gap is infinite, the advance reaches hi = T_f) -- no new branch;
//   * a distance >= D_cap reported as D_cap is a lower bound of it, and advancing on a lower bound is conservative.
// look_ahead bounds the ball a step walks, and so the points a lane meets: without it the first step of a long edge walks the whole
// cloud.  k_edge_ca_init gives CA_KEEP_KEY to the edges whose items do not run and whose result is 0 / UNDECIDED / NaN: every
// non-degenerate edge while the cloud's status is set, and -- accumulating -- those that come in with a NaN t_free.

// the distance of held shape h from the cloud at the lane's staged row, cut at D (D_end: the cut that reaches the stop point); the
// frame, A . G and the core are formed here, only where ok, and die here: none of them is carried round ca_walk's loop
NBK_DEV double held_cloud_cut_distance(const DevModel& m, const HeldDev& hd, const CloudDev& cd, const double* grow, double radius,
                                       const double* myq, bool ok, int h, double D_end, double d_cap) {
    Core P;
    cloud_point_core(radius, P);
    Core Hc;
    cloud_core_init(Hc);
    double D = 0.0;
    if (ok) {
        Xf F;
        held_frame(m, hd.mask, myq, F);
        double G[12], AG[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) G[e] = grow[e];
        held_mul12(hd.tab, G, AG);
        held_core(hd, h, F, AG, Hc);
        if (Hc.kind == K_HULL) Hc.rad = -1.0;      // the certified grids have blockIdx.y = h: every working lane holds this hull
        D = D_end < d_cap ? D_end : d_cap;
    }
    double best = NBK_INF;
    int bs = -1, bi = -1;
    cloud_core_clearance(cd, Hc, P, radius, ok, 0, D, best, bs, bi);
    if (!ok) return __builtin_nan("");
    if (best < D) return best;
    return D == D_end ? NBK_INF : d_cap;
}

// the linear edge of EdgeLane for one held shape against the cloud
struct HeldCloudEdgeLane {
    const double* s;
    const double* g;
    double Tf;
    const HeldDev& hd;
    const CloudDev& cd;
    const double* grow;       // the call's grasp row
    double radius;            // of the cloud's points
    double* myq;              // the lane's LDS row
    double d_base, d_cap;     // thr + slack; (thr + slack) + look_ahead
    double mu;
    NBK_DEV double end() const { return Tf; }
    NBK_DEV double span_end() const { return Tf; }
    NBK_DEV double enter(const DevModel& m, int h, double) {
        const MotionShape hs = held_motion_shape(hd.mask, hd.tab, grow, h);
        mu = motion_terms(m.mt, hs, hs.mask, EdgeMotion{s, g}, 0.0);
        return mu;
    }
    NBK_DEV double distance(const DevModel& m, bool run, int h, int, double t, double*) {
        bool ok = false;
        if (run) {
            const double omt = 1.0 - t;
            for (int c = 0; c < m.n_q; ++c) { const double a = omt * s[c]; const double b = t * g[c]; myq[c] = a + b; }
            ok = !row_nonfinite(myq, m.n_q, 1);      // (a non-finite q(t) is answered NaN without a walk: the item stops UNDECIDED there)
        }
        return held_cloud_cut_distance(m, hd, cd, grow, radius, myq, ok, h, ok ? d_base + mu * (Tf - t) : 0.0, d_cap);
    }
};

__global__ __launch_bounds__(64) void k_held_cloud_edge_ca(DevModel m, HeldDev hd, CloudDev cd, const double* __restrict__ starts,
                                                           const double* __restrict__ goals, const double* __restrict__ dist, int64_t E,
                                                           double max_distance, int mode, const double* __restrict__ grasp, double thr,
                                                           int max_iter, double slack, double look_ahead,
                                                           unsigned long long* __restrict__ key) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int h = (int)blockIdx.y;
    if (h >= hd.n_shapes) return;
    const int n = cd.hdr->n;
    const int64_t i = (int64_t)blockIdx.x * WAVE + lane;
    const bool live = i < E;
    const int64_t e = live ? i : 0;
    const double base = thr + slack;
    HeldCloudEdgeLane tr{starts + e * m.n_q, goals + e * m.n_q, 0.0, hd, cd, grasp != nullptr ? grasp : hd.tab + 12, cd.hdr->radius,
                         lds + lane * m.n_q, base, base + look_ahead, 0.0};
    double d_edge = 0.0;
    // (an empty cloud stops every item FREE at T_f, which is where its key stands; the keys of a cloud whose status is set, or of a
    // grasp that is not finite, are all reserved)
    const bool run = live && n > 0 && edge_span(m.n_q, tr.s, tr.g, dist, e, max_distance, mode, d_edge, tr.Tf) &&
                     __hip_atomic_load(key + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != CA_KEEP_KEY;
    ca_walk(m, tr, run, h, h, lane, thr, max_iter, slack, key + e);
}

// SplineLane's trajectory with HeldCloudEdgeLane's distance: entering a span gives mu_h on that span, q(t) goes by de_boor into the
// lane's LDS row, and the distance is the held shape's clearance from the cloud cut at
//     D = min(D_end, D_cap),   D_end = (thr + slack) + mu_max (1 - t),   D_cap = (thr + slack) + look_ahead,
// the smallest distance below D where there is one; else +inf when D == D_end; else D_cap.  mu_max is the LARGEST span bound of the
// trajectory over its non-empty spans, formed once per lane before the walk (bound_all), not the current span's.  Soundness of the
// +inf, as at CloudSplineLane:
//   * ca_walk carries an infinite gap across ALL remaining spans without another evaluation (gap - mu (hi - t) stays infinite), so
//     +inf at t stops the item FREE at 1: it may only be reported when no point can be reached on the whole remainder [t, 1];
//   * each span's mu bounds the speed of every point of the held shape on that span, so mu_max bounds it on every span, and no point
//     of the shape travels further than mu_max (1 - t) between q(t) and any q(t'), t' in [t, 1]; the cloud stands still;
//   * so no point within D_end at t means that the distance stays above thr + slack up to 1;
//   * D_cap is a lower bound of a distance that is not below it, and advancing on a lower bound is conservative, span by span with
//     each span's own mu.
// With n = 2, K = 1 and the knots [0, 0, 1, 1] there is one span, mu_max = mu and T_f = 1: HeldCloudEdgeLane's bits in connect mode.
template <int K>
struct HeldCloudSplineLane {
    const double* c;          // control points of the trajectory, [n][nq]
    const double* knots;
    int n, nq, ell;
    const HeldDev& hd;
    const CloudDev& cd;
    const double* grow;       // the call's grasp row
    double radius;            // of the cloud's points
    double* myq;              // the lane's LDS row
    double d_base, d_cap;     // thr + slack; (thr + slack) + look_ahead
    double mu_max;
    NBK_DEV double end() const { return 1.0; }
    NBK_DEV double span_end() const { return knots[ell + 1]; }
    NBK_DEV double span_bound(const DevModel& m, int h, int span) const {
        const MotionShape hs = held_motion_shape(hd.mask, hd.tab, grow, h);
        return motion_terms(m.mt, hs, hs.mask, SplineSpanMotion{c + (size_t)(span - K) * nq, knots + (span - K + 1), nq, K}, 0.0);
    }
    NBK_DEV double enter(const DevModel& m, int h, double t) {
        ell = spline_span<K>(knots, n, t);
        return span_bound(m, h, ell);
    }
    // the largest bound over the non-empty spans: what D_end may use (see above)
    NBK_DEV void bound_all(const DevModel& m, int h) {
        mu_max = 0.0;
        for (int span = K; span < n; ++span) {
            if (!(knots[span] < knots[span + 1])) continue;
            const double mu = span_bound(m, h, span);
            mu_max = mu > mu_max ? mu : mu_max;
        }
    }
    NBK_DEV double distance(const DevModel& m, bool run, int h, int, double t, double*) {
        bool ok = false;
        if (run) {
            double* r = myq;
            de_boor<K>(nq, c + (size_t)(ell - K) * nq, knots, ell, t, [&](int j, double v) { r[j] = v; });
            ok = !row_nonfinite(myq, nq, 1);
        }
        // mu_max, NOT the current span's mu: +inf frees the item up to 1 across every later span (ca_walk evaluates nothing there),
        // and a later span may be faster than this one
        return held_cloud_cut_distance(m, hd, cd, grow, radius, myq, ok, h, ok ? d_base + mu_max * (1.0 - t) : 0.0, d_cap);
    }
};

template <int K>
__global__ __launch_bounds__(64) void k_held_cloud_spline_ca(DevModel m, HeldDev hd, CloudDev cd, const double* __restrict__ ctrl, int64_t S,
                                                             int n, const double* __restrict__ knots, const double* __restrict__ grasp,
                                                             double thr, int max_iter, double slack, double look_ahead,
                                                             unsigned long long* __restrict__ key) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int h = (int)blockIdx.y;
    if (h >= hd.n_shapes) return;
    const int ncl = cd.hdr->n;
    const int64_t i = (int64_t)blockIdx.x * WAVE + lane;
    const bool live = i < S;
    const int64_t s = live ? i : 0;
    const double base = thr + slack;
    HeldCloudSplineLane<K> tr{ctrl + (size_t)s * (size_t)n * m.n_q, knots, n, m.n_q, K, hd, cd, grasp != nullptr ? grasp : hd.tab + 12,
                              cd.hdr->radius, lds + lane * m.n_q, base, base + look_ahead, 0.0};
    // (an empty cloud stops every item FREE at 1, which is where its key stands)
    bool run = false;
    if (live && ncl > 0) {
        const unsigned long long k0 = __hip_atomic_load(key + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        run = k0 != CA_DEGENERATE_KEY && k0 != CA_KEEP_KEY;
    }
    if (run) tr.bound_all(m, h);
    ca_walk(m, tr, run, h, h, lane, thr, max_iter, slack, key + s);
}

}  // namespace nbk

struct nbk_held {
    nbk::HeldDev d;
    const nbk_model* model;        // the descriptor it was made against: its calls take no other
    int device;
    void* blob;
    std::vector<int> h_items;      // the host copy of d.items
    bool has_hull;                 // a held shape is a hull (nbk_held_create_hulls)
    bool cloud_hulls;              // nbk_held_set_cloud_hulls: the held-versus-cloud entries serve the hulls (host side only: no kernel
                                   // reads it); cleared by the creators, and without it those entries refuse an object that has a hull
};

namespace nbk {

static int32_t held_call_begin(const nbk_model* m, const nbk_held* h) {
    if (h->model != m) { snprintf(g_err, sizeof(g_err), "the held object was made against another descriptor"); return NBK_ERR_INVALID; }
    NBK_DEVICE(m);
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != h->device) {
        snprintf(g_err, sizeof(g_err), "held object belongs to device %d, the current device is %d", h->device, dev);
        return NBK_ERR_INVALID;
    }
    return NBK_OK;
}

// the status word that holds a held call: the world status of a movable descriptor, else none
static const int* world_status_word(const nbk_model* m) { return m->movable ? (const int*)m->world_status : (const int*)nullptr; }

// The grasp rule of the row entries, answered without a device: grasp_rows is 0 (the stored grasp), 1 (the call's one row) or B (a row
// each), and -- where there are rows of q at all -- a grasp is passed exactly when it has rows -> held_grasp_row's code 0 / 1 / 2, or
// -1 where the rule is broken
static int held_grasp_rows(const double* grasp, int64_t grasp_rows, int64_t B) {
    if (grasp_rows != 0 && grasp_rows != 1 && grasp_rows != B) return -1;
    if ((grasp_rows != 0) != (grasp != nullptr) && B > 0) return -1;
    return grasp_rows == 0 ? 0 : (grasp_rows == 1 ? 1 : 2);
}

static bool held_pose_finite(const double* p) {
    for (int e = 0; e < 12; ++e) if (!(p[e] - p[e] == 0.0)) return false;
    return true;
}

// the hull tables of a held object, in the layout and with the rules of nbk_model_desc's hull fields (nbk_held_create_hulls and the
// *_hulls_host twins); the entries without them pass null and refuse a hull shape
struct HeldHulls {
    int32_t n;
    const int32_t* vert_begin;
    const double* verts;
    const int32_t* face_begin;
    const double* planes;
    int nv(int h) const { return vert_begin[h + 1] - vert_begin[h]; }
    int nf(int h) const { return face_begin[h + 1] - face_begin[h]; }
};

// the argument rules of the held shapes, their poses and the world list (the two creators and the host twins of the motion bound).
// hl == null: a hull shape is NBK_ERR_UNSUPPORTED; else the tables pass desc_check's hull rules (a descriptor of nothing but them)
// and a hull shape names one of them in param[0]
static int32_t held_args_check(int32_t frame, int32_t n_joints, int32_t n_wshapes, const double* A, const double* G, int32_t H,
                               const int32_t* shape_type, const double* shape_local, const double* shape_param, int32_t n_world,
                               const int32_t* world_shapes, const HeldHulls* hl = nullptr) {
    if (A == nullptr || G == nullptr || H < 1 || shape_type == nullptr || shape_local == nullptr || shape_param == nullptr ||
        n_world < 0 || (n_world > 0 && world_shapes == nullptr))
        return NBK_ERR_INVALID;
    if (frame < -1 || frame >= n_joints || n_world > n_wshapes) return NBK_ERR_INVALID;
    if (!held_pose_finite(A) || !held_pose_finite(G)) return NBK_ERR_INVALID;
    if (H > HELD_MAX_SHAPES) return NBK_ERR_UNSUPPORTED;
    if (hl != nullptr) {
        nbk_model_desc hd{};
        hd.n_hulls = hl->n; hd.hull_vert_begin = hl->vert_begin; hd.hull_verts = hl->verts;
        hd.hull_face_begin = hl->face_begin; hd.hull_planes = hl->planes;
        if (desc_check(&hd, D_HULL_PLANES) != NBK_OK) return NBK_ERR_INVALID;
    }
    for (int32_t h = 0; h < H; ++h) {
        if (shape_type[h] == NBK_HULL && hl == nullptr) return NBK_ERR_UNSUPPORTED;
        if (shape_type[h] != NBK_SPHERE && shape_type[h] != NBK_CAPSULE && shape_type[h] != NBK_BOX && shape_type[h] != NBK_CYLINDER &&
            shape_type[h] != NBK_HULL) return NBK_ERR_INVALID;
        if (!held_pose_finite(shape_local + 12 * (size_t)h)) return NBK_ERR_INVALID;
        for (int e = 0; e < 4; ++e) if (!(shape_param[4 * h + e] - shape_param[4 * h + e] == 0.0)) return NBK_ERR_INVALID;
        const double idx = shape_param[4 * h];
        if (shape_type[h] == NBK_HULL && !(idx >= 0.0 && idx < (double)hl->n && idx == (double)(int)idx)) return NBK_ERR_INVALID;
    }
    for (int32_t i = 0; i < n_world; ++i) {
        if (world_shapes[i] < 0 || world_shapes[i] >= n_wshapes) return NBK_ERR_INVALID;
        if (i > 0 && world_shapes[i] <= world_shapes[i - 1]) return NBK_ERR_INVALID;
    }
    return NBK_OK;
}

// A | G | the shape records (HeldDev.tab) and the core kinds
// (a hull's h0 h1 h2 slot stays zero here: nbk_held_create_hulls patches the HullRef in once the blob's address is known)
static void held_tab(const double* A, const double* G, int32_t H, const int32_t* shape_type, const double* shape_local,
                     const double* shape_param, std::vector<double>& tab, std::vector<int>& kind, const HeldHulls* hl = nullptr) {
    tab.assign(24 + HELD_SHAPE_LEN * (size_t)H, 0.0);
    kind.assign(H, 0);
    memcpy(&tab[0], A, 12 * sizeof(double));
    memcpy(&tab[12], G, 12 * sizeof(double));
    for (int32_t h = 0; h < H; ++h) {
        double* rec = &tab[24 + HELD_SHAPE_LEN * (size_t)h];
        memcpy(rec, shape_local + 12 * (size_t)h, 12 * sizeof(double));
        core_params(shape_type[h], shape_param + 4 * (size_t)h, kind[h], rec + 12);
        if (kind[h] == K_HULL) {             // (robot_core_host's statements)
            const int x = (int)shape_param[4 * (size_t)h];
            rec[17] = hull_bound_radius(hl->verts + 3 * (size_t)hl->vert_begin[x], hl->nv(x));
        }
        rec[17] = host_bound_radius(kind[h], rec + 12);
    }
}

// f(std::true_type / std::false_type) for a run-time flag (with_degree's form): the verdict entries pick their walk's instance
template <class F>
static void with_flag(bool on, F&& f) {
    if (on) f(std::integral_constant<bool, true>{});
    else f(std::integral_constant<bool, false>{});
}

// the items (HeldDev.items): robot_bits in the caller's order over S shapes (null: none); dev_of_user (nullable): the device index
// of each of the caller's shapes, else the caller's index stands in
static std::vector<int> held_item_list(int S, const int* dev_of_user, const uint64_t* robot_bits, int H, int n_world, const int32_t* world) {
    std::vector<int> it;
    if (robot_bits != nullptr)
        for (int s = 0; s < S; ++s) {
            if (((robot_bits[s >> 6] >> (s & 63)) & 1ull) == 0ull) continue;
            for (int h = 0; h < H; ++h) { it.push_back(h); it.push_back(0); it.push_back(dev_of_user != nullptr ? dev_of_user[s] : s); it.push_back(s); }
        }
    for (int h = 0; h < H; ++h)
        for (int i = 0; i < n_world; ++i) { it.push_back(h); it.push_back(1); it.push_back(world[i]); it.push_back(world[i]); }
    return it;
}

}  // namespace nbk

extern "C" {

int32_t nbk_held_locals_host(const double* A, const double* G, const double* L, int32_t H, double* out) {
    if (A == nullptr || G == nullptr || H < 0 || (H > 0 && (L == nullptr || out == nullptr))) return NBK_ERR_INVALID;
    double AG[12];
    held_mul12(A, G, AG);
    for (int32_t h = 0; h < H; ++h) held_locals(AG, L + 12 * (size_t)h, out + 12 * (size_t)h);
    return NBK_OK;
}

// the body of the two creators (hl: the hull tables of nbk_held_create_hulls, null for nbk_held_create).  The blob: the tables, the
// kinds, the world list, the items, then -- as the scene's hull_blob -- each hull's [local bounding box (6) | vertices], then every
// hull's planes; the h0 h1 h2 slot of a hull shape's record holds its HullRef into them (patch_hulls' statements)
static int32_t held_create(const nbk_model* m, int32_t frame, const double* A, const double* G, int32_t H, const int32_t* shape_type,
                           const double* shape_local, const double* shape_param, int32_t n_world, const int32_t* world_shapes,
                           const uint64_t* robot_bits, const HeldHulls* hl, nbk_held** out) {
    if (out == nullptr) return NBK_ERR_INVALID;
    *out = nullptr;
    if (m == nullptr) return NBK_ERR_INVALID;
    { const int32_t rc = held_args_check(frame, m->n_joints, m->d.n_wshapes, A, G, H, shape_type, shape_local, shape_param, n_world, world_shapes, hl);
      if (rc != NBK_OK) return rc; }
    if (robot_bits != nullptr && m->d.n_rshapes > 256) return NBK_ERR_UNSUPPORTED;
    NBK_DEVICE(m);
    // the tables, then one allocation and one copy
    std::vector<double> tab;
    std::vector<int> kind, world(n_world > 0 ? n_world : 1, 0);
    held_tab(A, G, H, shape_type, shape_local, shape_param, tab, kind, hl);
    for (int32_t i = 0; i < n_world; ++i) world[i] = world_shapes[i];
    const int NH = hl != nullptr ? hl->n : 0;
    std::vector<double> hverts;
    std::vector<size_t> hoff(NH > 0 ? NH : 1, 0);      // offset (in doubles) of hull x's first vertex inside hverts
    for (int x = 0; x < NH; ++x) {
        const double* v = hl->verts + 3 * (size_t)hl->vert_begin[x];
        double box[6];
        hull_local_box(v, hl->nv(x), box);
        hverts.insert(hverts.end(), box, box + 6);
        hoff[x] = hverts.size();
        hverts.insert(hverts.end(), v, v + 3 * (size_t)hl->nv(x));
    }
    const size_t n_planes = NH > 0 ? 4 * (size_t)hl->face_begin[NH] : 0;
    const int S = m->d.n_rshapes;
    std::vector<int> dev_of_user(S > 0 ? S : 1, 0);
    for (int i = 0; i < S; ++i) dev_of_user[m->h_rs_user[i]] = i;
    std::vector<int> items = held_item_list(S, dev_of_user.data(), robot_bits, H, n_world, world_shapes);
    const int n_items = (int)(items.size() / HELD_ITEM_LEN);
    auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
    const size_t o_kind = up(sizeof(double) * tab.size());
    const size_t o_world = up(o_kind + sizeof(int) * kind.size());
    const size_t o_items = up(o_world + sizeof(int) * world.size());
    const size_t o_verts = up(o_items + sizeof(int) * (items.size() > 0 ? items.size() : 1));
    const size_t o_planes = up(o_verts + sizeof(double) * hverts.size());
    const size_t bytes = up(o_planes + sizeof(double) * n_planes);
    std::vector<char> host(bytes, 0);
    memcpy(host.data(), tab.data(), sizeof(double) * tab.size());
    memcpy(host.data() + o_kind, kind.data(), sizeof(int) * kind.size());
    memcpy(host.data() + o_world, world.data(), sizeof(int) * world.size());
    if (!items.empty()) memcpy(host.data() + o_items, items.data(), sizeof(int) * items.size());
    if (!hverts.empty()) memcpy(host.data() + o_verts, hverts.data(), sizeof(double) * hverts.size());
    if (n_planes > 0) memcpy(host.data() + o_planes, hl->planes, sizeof(double) * n_planes);
    std::unique_ptr<nbk_held> hd(new nbk_held());
    hipError_t e = hipMalloc(&hd->blob, bytes);
    if (e != hipSuccess) { hip_fail(e, "hipMalloc(held)"); return NBK_ERR_ALLOC; }
    hd->has_hull = false;
    hd->cloud_hulls = false;
    for (int32_t h = 0; h < H; ++h) {
        if (kind[h] != K_HULL) continue;
        const int x = (int)shape_param[4 * (size_t)h];
        HullRef r;
        r.hv = reinterpret_cast<const double*>(static_cast<const char*>(hd->blob) + o_verts) + hoff[x];
        r.hp = reinterpret_cast<const double*>(static_cast<const char*>(hd->blob) + o_planes) + 4 * (size_t)hl->face_begin[x];
        r.hn = hl->nv(x);
        r.hf = hl->nf(x);
        static_assert(sizeof(HullRef) == 24, "HullRef must overlay h[3]");
        memcpy(host.data() + sizeof(double) * (24 + HELD_SHAPE_LEN * (size_t)h + 12), &r, sizeof(r));
        hd->has_hull = true;
    }
    e = hipMemcpy(hd->blob, host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(hd->blob); return hip_fail(e, "hipMemcpy(held)"); }
    const char* base = static_cast<const char*>(hd->blob);
    hd->d.mask = frame >= 0 ? m->h_frame_mask[frame] : 0u;
    hd->d.n_shapes = H;
    hd->d.n_world = n_world;
    hd->d.tab = reinterpret_cast<const double*>(base);
    hd->d.kind = reinterpret_cast<const int*>(base + o_kind);
    hd->d.world = reinterpret_cast<const int*>(base + o_world);
    hd->d.robot = robot_bits == nullptr ? CloudSel{{0ull, 0ull, 0ull, 0ull}, 0} : cloud_selection(m, robot_bits);
    hd->d.n_items = n_items;
    hd->d.items = reinterpret_cast<const int*>(base + o_items);
    hd->h_items = std::move(items);
    hd->model = m;
    (void)hipGetDevice(&hd->device);
    *out = hd.release();
    return NBK_OK;
}

int32_t nbk_held_create(const nbk_model* m, int32_t frame, const double* A, const double* G, int32_t H, const int32_t* shape_type,
                        const double* shape_local, const double* shape_param, int32_t n_world, const int32_t* world_shapes,
                        const uint64_t* robot_bits, nbk_held** out) {
    return held_create(m, frame, A, G, H, shape_type, shape_local, shape_param, n_world, world_shapes, robot_bits, nullptr, out);
}

int32_t nbk_held_create_hulls(const nbk_model* m, int32_t frame, const double* A, const double* G, int32_t H, const int32_t* shape_type,
                              const double* shape_local, const double* shape_param, int32_t n_world, const int32_t* world_shapes,
                              const uint64_t* robot_bits, int32_t n_hulls, const int32_t* hull_vert_begin, const double* hull_verts,
                              const int32_t* hull_face_begin, const double* hull_planes, nbk_held** out) {
    const HeldHulls hl{n_hulls, hull_vert_begin, hull_verts, hull_face_begin, hull_planes};
    return held_create(m, frame, A, G, H, shape_type, shape_local, shape_param, n_world, world_shapes, robot_bits, &hl, out);
}

int32_t nbk_held_set_cloud_hulls(nbk_held* held, int32_t on) {
    if (held == nullptr) return NBK_ERR_INVALID;
    held->cloud_hulls = on != 0;
    return NBK_OK;
}

void nbk_held_destroy(nbk_held* h) {
    if (h == nullptr) return;
    if (h->blob) (void)hipFree(h->blob);
    delete h;
}

int32_t nbk_held_validity_batch(const nbk_model* m, const nbk_held* held, const double* q, int64_t B, const double* grasp,
                                int64_t grasp_rows, double threshold, int32_t accumulate, uint64_t* mask_bits, uint8_t* mask_bytes,
                                void* stream) {
    if (m == nullptr || held == nullptr || B < 0 || threshold != threshold) return NBK_ERR_INVALID;
    const int rows = held_grasp_rows(grasp, grasp_rows, B);
    if (rows < 0) return NBK_ERR_INVALID;
    if (B > 0 && (q == nullptr || (mask_bits == nullptr && mask_bytes == nullptr))) return NBK_ERR_INVALID;
    { const int32_t rc = held_call_begin(m, held); if (rc != NBK_OK) return rc; }
    if (B == 0) return NBK_OK;
    if ((B + WAVE - 1) / WAVE > 0x7fffffffLL) return NBK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_held_validity, dim3(blocks_for(B)), dim3(WAVE), QSlabLds(m->n_q).bytes(), (hipStream_t)stream, m->d, held->d,
                       world_status_word(m), q, B, grasp, rows, threshold, (int)accumulate,
                       reinterpret_cast<unsigned long long*>(mask_bits), mask_bytes);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int64_t nbk_edge_held_workspace_bytes(int64_t E) { return edge_workspace_bytes(E); }

int32_t nbk_edge_held_validity_batch(const nbk_model* m, const nbk_held* held, const double* starts, const double* goals, const double* dist,
                                     int64_t E, double resolution, double max_distance, int32_t mode, double threshold,
                                     const double* grasp, int32_t accumulate, uint8_t* valid, double* end, int32_t* n_samples,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
    if (m == nullptr || held == nullptr) return NBK_ERR_INVALID;
    return sampled_edges_call(
        m, starts, goals, dist, E, resolution, max_distance, mode, threshold, accumulate, valid, end, n_samples, workspace, workspace_bytes,
        stream, [&] { return held_call_begin(m, held); },
        [&](dim3 grid, size_t lds, hipStream_t st, const EdgeSrc& es, const unsigned long long* offs) {
            hipLaunchKernelGGL(k_held_edges, grid, dim3(WAVE), lds, st, m->d, held->d, world_status_word(m), es, offs, E, grasp,
                               grasp != nullptr ? 1 : 0, threshold, valid);
        });
}

int32_t nbk_held_item_count(const nbk_held* held) { return held == nullptr ? NBK_ERR_INVALID : held->d.n_items; }

int32_t nbk_held_items(const nbk_held* held, int32_t* out) {
    if (held == nullptr || (held->d.n_items > 0 && out == nullptr)) return NBK_ERR_INVALID;
    for (int i = 0; i < held->d.n_items; ++i) {
        const int* rec = &held->h_items[HELD_ITEM_LEN * (size_t)i];
        out[3 * i] = rec[0]; out[3 * i + 1] = rec[1]; out[3 * i + 2] = rec[3];
    }
    return NBK_OK;
}

int32_t nbk_held_distances_batch(const nbk_model* m, const nbk_held* held, const double* q, int64_t B, const double* grasp,
                                 int64_t grasp_rows, double* out_d, void* stream) {
    if (m == nullptr || held == nullptr || B < 0) return NBK_ERR_INVALID;
    const int rows = held_grasp_rows(grasp, grasp_rows, B);
    if (rows < 0) return NBK_ERR_INVALID;
    const int64_t K = held->d.n_items;
    if (B > 0 && (q == nullptr || (K > 0 && out_d == nullptr))) return NBK_ERR_INVALID;
    { const int32_t rc = held_call_begin(m, held); if (rc != NBK_OK) return rc; }
    if (B == 0 || K == 0) return NBK_OK;
    if (B > 0x7fffffffLL || (B * K + WAVE - 1) / WAVE > 0x7fffffffLL) return NBK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_held_distances, dim3((unsigned)((B * K + WAVE - 1) / WAVE)), dim3(WAVE), QSlabLds(m->n_q).bytes(), (hipStream_t)stream,
                       m->d, held->d, world_status_word(m), q, B, grasp, rows, out_d);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int32_t nbk_held_records_batch(const nbk_model* m, const nbk_held* held, const double* q, int64_t B, const double* grasp,
                               int64_t grasp_rows, double* dist, double* witness, double* jrows, void* stream) {
    if (m == nullptr || held == nullptr || B < 0) return NBK_ERR_INVALID;
    const int rows = held_grasp_rows(grasp, grasp_rows, B);
    if (rows < 0) return NBK_ERR_INVALID;
    if (B > 0 && (q == nullptr || dist == nullptr)) return NBK_ERR_INVALID;
    { const int32_t rc = held_call_begin(m, held); if (rc != NBK_OK) return rc; }
    const int64_t K = held->d.n_items;
    if (B == 0 || K == 0) return NBK_OK;
    if (B > 0x7fffffffLL || (B * K + WAVE - 1) / WAVE > 0x7fffffffLL) return NBK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_held_records<false>, dim3((unsigned)((B * K + WAVE - 1) / WAVE)), dim3(WAVE),
                       PairItemsLds(m->n_q, jrows != nullptr ? m->n_joints : 0).bytes(), (hipStream_t)stream, m->d, held->d,
                       world_status_word(m), q, B, (const int32_t*)nullptr, (int64_t)0, grasp, rows, dist, witness, jrows);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int32_t nbk_held_records_items(const nbk_model* m, const nbk_held* held, const double* q, int64_t B, const int32_t* items, int64_t N,
                               const double* grasp, int64_t grasp_rows, double* dist, double* witness, double* jrows, void* stream) {
    if (m == nullptr || held == nullptr || B < 0) return NBK_ERR_INVALID;
    const int rows = held_grasp_rows(grasp, grasp_rows, B);
    if (rows < 0) return NBK_ERR_INVALID;
    if (N < 0 || (N > 0 && (items == nullptr || dist == nullptr || (B > 0 && q == nullptr)))) return NBK_ERR_INVALID;
    { const int32_t rc = held_call_begin(m, held); if (rc != NBK_OK) return rc; }
    if (N == 0) return NBK_OK;
    if (B > 0x7fffffffLL || (N + WAVE - 1) / WAVE > 0x7fffffffLL) return NBK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_held_records<true>, dim3((unsigned)((N + WAVE - 1) / WAVE)), dim3(WAVE),
                       PairItemsLds(m->n_q, jrows != nullptr ? m->n_joints : 0).bytes(), (hipStream_t)stream, m->d, held->d,
                       world_status_word(m), q, B, items, N, grasp, rows, dist, witness, jrows);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

// (the certified entries of the held object alone: a flat grid of n x K lanes, K = the object's items, read for the size limit before
// the handles are looked at; no status holds the init kernel -- the world status and the call's grasp go through the grasp hold)
int32_t nbk_edge_held_continuous_batch(const nbk_model* m, const nbk_held* held, const double* starts, const double* goals, const double* dist,
                                       int64_t E, double max_distance, int32_t mode, double threshold, int32_t max_iter, double slack,
                                       const double* grasp, int32_t accumulate, uint8_t* valid, double* end, double* t_free, int32_t* status,
                                       void* stream) {
    if (m == nullptr || held == nullptr) return NBK_ERR_INVALID;
    return certified_edges_call(
        m, starts, goals, dist, E, max_distance, mode, threshold, max_iter, slack, nullptr, &held->d.n_items, true, nullptr,
        world_status_word(m), grasp, accumulate, valid, end, t_free, status, stream, [&] { return held_call_begin(m, held); },
        [&](hipStream_t st) {
            const int64_t N = E * (int64_t)held->d.n_items;
            hipLaunchKernelGGL(k_held_edge_ca, dim3((unsigned)((N + WAVE - 1) / WAVE)), dim3(WAVE), QSlabLds(m->n_q).bytes(), st, m->d, held->d,
                               starts, goals, dist, E, max_distance, (int)mode, grasp, threshold, (int)max_iter, slack, ca_keys(t_free));
        });
}

int32_t nbk_spline_held_continuous_batch(const nbk_model* m, const nbk_held* held, const double* ctrl, int64_t S, int32_t n_ctrl,
                                         int32_t degree, const double* knots, double threshold, int32_t max_iter, double slack,
                                         const double* grasp, int32_t accumulate, uint8_t* valid, double* t_free, int32_t* status,
                                         void* stream) {
    if (m == nullptr || held == nullptr) return NBK_ERR_INVALID;
    return certified_splines_call(
        m, ctrl, S, n_ctrl, degree, knots, threshold, max_iter, slack, nullptr, &held->d.n_items, true, nullptr, world_status_word(m), grasp,
        accumulate, valid, t_free, status, stream, [&] { return held_call_begin(m, held); },
        [&](auto K, size_t lds, hipStream_t st) {
            const int64_t N = S * (int64_t)held->d.n_items;
            hipLaunchKernelGGL(k_held_spline_ca<decltype(K)::value>, dim3((unsigned)((N + WAVE - 1) / WAVE)), dim3(WAVE), lds, st, m->d,
                               held->d, ctrl, S, (int)n_ctrl, knots, grasp, threshold, (int)max_iter, slack, ca_keys(t_free));
        });
}

int64_t nbk_spline_held_workspace_bytes(int64_t S) { return spline_workspace_bytes(S); }

int32_t nbk_spline_held_validity_batch(const nbk_model* m, const nbk_held* held, const double* ctrl, int64_t S, int32_t n_ctrl, int32_t degree,
                                       const double* knots, double resolution, double threshold, const double* grasp,
                                       int32_t accumulate, uint8_t* valid, double* t_hit, int32_t* n_samples, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
    if (m == nullptr || held == nullptr) return NBK_ERR_INVALID;
    return sampled_splines_call(
        m, ctrl, S, n_ctrl, degree, knots, resolution, threshold, world_status_word(m), accumulate, valid, t_hit, n_samples, workspace,
        workspace_bytes, stream, [&] { return held_call_begin(m, held); },
        [&](auto K, dim3 grid, size_t lds, hipStream_t st, const SplineCloudLayout::View& v, const double* t_prev) {
            hipLaunchKernelGGL(k_held_spline<decltype(K)::value>, grid, dim3(WAVE), lds, st, m->d, held->d, ctrl, (int)n_ctrl, knots,
                               (const double*)v.plan, (const unsigned long long*)v.offs, S, grasp, grasp != nullptr ? 1 : 0, threshold, t_prev,
                               v.first);
        });
}

// ---- the held object against a point cloud.  What every entry answers once its own argument rules are through: the held object's
// descriptor and device (held_call_begin), then the cloud's device.
static int32_t held_cloud_call_begin(const nbk_model* m, const nbk_held* held, const nbk_cloud* c) {
    // (hulls against a cloud are opt-in, nbk_held_set_cloud_hulls: without the flag refused before a device is touched)
    if (held->has_hull && !held->cloud_hulls) { snprintf(g_err, sizeof(g_err), "a held object with a hull is not served against point clouds"); return NBK_ERR_UNSUPPORTED; }
    { const int32_t rc = held_call_begin(m, held); if (rc != NBK_OK) return rc; }
    return cloud_check_device(c);
}

int32_t nbk_held_cloud_validity_batch(const nbk_model* m, const nbk_held* held, const nbk_cloud* c, const double* q, int64_t B,
                                      const double* grasp, int64_t grasp_rows, double threshold, int32_t accumulate, uint64_t* mask_bits,
                                      uint8_t* mask_bytes, void* stream) {
    if (m == nullptr || held == nullptr || c == nullptr || B < 0 || threshold != threshold) return NBK_ERR_INVALID;
    const int rows = held_grasp_rows(grasp, grasp_rows, B);
    if (rows < 0) return NBK_ERR_INVALID;
    if (B > 0 && (q == nullptr || (mask_bits == nullptr && mask_bytes == nullptr))) return NBK_ERR_INVALID;
    { const int32_t rc = held_cloud_call_begin(m, held, c); if (rc != NBK_OK) return rc; }
    if (B == 0) return NBK_OK;
    if ((B + WAVE - 1) / WAVE > 0x7fffffffLL) return NBK_ERR_UNSUPPORTED;
    with_flag(held->has_hull, [&](auto HULLS) {
        hipLaunchKernelGGL(k_held_cloud_validity<decltype(HULLS)::value>, dim3(blocks_for(B)), dim3(WAVE), QSlabLds(m->n_q).bytes(),
                           (hipStream_t)stream, m->d, held->d, cloud_dev(c), q, B, grasp, rows, threshold, (int)accumulate,
                           reinterpret_cast<unsigned long long*>(mask_bits), mask_bytes);
    });
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int32_t nbk_held_cloud_clearance_batch(const nbk_model* m, const nbk_held* held, const nbk_cloud* c, const double* q, int64_t B,
                                       const double* grasp, int64_t grasp_rows, double d_max, double* min_dist, int32_t* shape,
                                       int32_t* point, void* stream) {
    if (m == nullptr || held == nullptr || c == nullptr || B < 0 || !(d_max - d_max == 0.0)) return NBK_ERR_INVALID;
    const int rows = held_grasp_rows(grasp, grasp_rows, B);
    if (rows < 0) return NBK_ERR_INVALID;
    if (B > 0 && (q == nullptr || min_dist == nullptr)) return NBK_ERR_INVALID;
    { const int32_t rc = held_cloud_call_begin(m, held, c); if (rc != NBK_OK) return rc; }
    if (B == 0) return NBK_OK;
    if ((B + WAVE - 1) / WAVE > 0x7fffffffLL) return NBK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_held_cloud_clearance, dim3(blocks_for(B)), dim3(WAVE), QSlabLds(m->n_q).bytes(), (hipStream_t)stream, m->d,
                       held->d, cloud_dev(c), q, B, grasp, rows, d_max, min_dist, shape, point);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int32_t nbk_held_cloud_records_batch(const nbk_model* m, const nbk_held* held, const nbk_cloud* c, const double* q, int64_t B,
                                     const double* grasp, int64_t grasp_rows, double d_max, int32_t per_shape, double* dist,
                                     int32_t* shape, int32_t* point, double* witness, double* jrows, void* stream) {
    if (m == nullptr || held == nullptr || c == nullptr || B < 0 || !(d_max - d_max == 0.0)) return NBK_ERR_INVALID;
    const int rows = held_grasp_rows(grasp, grasp_rows, B);
    if (rows < 0) return NBK_ERR_INVALID;
    if (B > 0 && (q == nullptr || dist == nullptr)) return NBK_ERR_INVALID;
    { const int32_t rc = held_cloud_call_begin(m, held, c); if (rc != NBK_OK) return rc; }
    if (B == 0) return NBK_OK;
    if ((B + WAVE - 1) / WAVE > 0x7fffffffLL) return NBK_ERR_UNSUPPORTED;
    const size_t lds = PairItemsLds(m->n_q, jrows != nullptr ? m->n_joints : 0).bytes();
    if (per_shape)
        hipLaunchKernelGGL(k_held_cloud_records<true>, dim3(blocks_for(B), (unsigned)held->d.n_shapes), dim3(WAVE), lds, (hipStream_t)stream,
                           m->d, held->d, cloud_dev(c), q, B, grasp, rows, d_max, dist, shape, point, witness, jrows);
    else
        hipLaunchKernelGGL(k_held_cloud_records<false>, dim3(blocks_for(B)), dim3(WAVE), lds, (hipStream_t)stream, m->d, held->d,
                           cloud_dev(c), q, B, grasp, rows, d_max, dist, shape, point, witness, jrows);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int64_t nbk_edge_held_cloud_workspace_bytes(int64_t E) { return edge_workspace_bytes(E); }

int32_t nbk_edge_held_cloud_validity_batch(const nbk_model* m, const nbk_held* held, const nbk_cloud* c, const double* starts,
                                           const double* goals, const double* dist, int64_t E, double resolution, double max_distance,
                                           int32_t mode, double threshold, const double* grasp, int32_t accumulate, uint8_t* valid,
                                           double* end, int32_t* n_samples, void* workspace, int64_t workspace_bytes, void* stream) {
    if (m == nullptr || held == nullptr || c == nullptr) return NBK_ERR_INVALID;
    return sampled_edges_call(
        m, starts, goals, dist, E, resolution, max_distance, mode, threshold, accumulate, valid, end, n_samples, workspace, workspace_bytes,
        stream, [&] { return held_cloud_call_begin(m, held, c); },
        [&](dim3 grid, size_t lds, hipStream_t st, const EdgeSrc& es, const unsigned long long* offs) {
            with_flag(held->has_hull, [&](auto HULLS) {
                hipLaunchKernelGGL(k_held_cloud_edges<decltype(HULLS)::value>, grid, dim3(WAVE), lds, st, m->d, held->d, cloud_dev(c), es, offs,
                                   E, grasp, grasp != nullptr ? 1 : 0, threshold, valid);
            });
        });
}

int64_t nbk_spline_held_cloud_workspace_bytes(int64_t S) { return spline_workspace_bytes(S); }

int32_t nbk_spline_held_cloud_validity_batch(const nbk_model* m, const nbk_held* held, const nbk_cloud* c, const double* ctrl, int64_t S,
                                             int32_t n_ctrl, int32_t degree, const double* knots, double resolution, double threshold,
                                             const double* grasp, int32_t accumulate, uint8_t* valid, double* t_hit, int32_t* n_samples,
                                             void* workspace, int64_t workspace_bytes, void* stream) {
    if (m == nullptr || held == nullptr || c == nullptr) return NBK_ERR_INVALID;
    return sampled_splines_call(
        m, ctrl, S, n_ctrl, degree, knots, resolution, threshold, cloud_status_word(c), accumulate, valid, t_hit, n_samples, workspace,
        workspace_bytes, stream, [&] { return held_cloud_call_begin(m, held, c); },
        [&](auto K, dim3 grid, size_t lds, hipStream_t st, const SplineCloudLayout::View& v, const double* t_prev) {
            with_flag(held->has_hull, [&](auto HULLS) {
                hipLaunchKernelGGL((k_held_cloud_spline<decltype(K)::value, decltype(HULLS)::value>), grid, dim3(WAVE), lds, st, m->d, held->d,
                                   cloud_dev(c), ctrl, (int)n_ctrl, knots, (const double*)v.plan, (const unsigned long long*)v.offs, S, grasp,
                                   grasp != nullptr ? 1 : 0, threshold, t_prev, v.first);
            });
        });
}

// (the certified entries against a cloud: one row of workgroups per held shape -- an object holds at least one --; the cloud's status
// holds the init kernel, and the grasp hold takes the call's grasp alone: the stored one is finite by nbk_held_create's rules, and
// the world status is not read)
int32_t nbk_edge_held_cloud_continuous_batch(const nbk_model* m, const nbk_held* held, const nbk_cloud* c, const double* starts,
                                             const double* goals, const double* dist, int64_t E, double max_distance, int32_t mode,
                                             double threshold, int32_t max_iter, double slack, double look_ahead, const double* grasp,
                                             int32_t accumulate, uint8_t* valid, double* end, double* t_free, int32_t* status,
                                             void* stream) {
    if (m == nullptr || held == nullptr || c == nullptr) return NBK_ERR_INVALID;
    return certified_edges_call(
        m, starts, goals, dist, E, max_distance, mode, threshold, max_iter, slack, &look_ahead, &held->d.n_shapes, false,
        cloud_status_word(c), nullptr, grasp, accumulate, valid, end, t_free, status, stream,
        [&] { return held_cloud_call_begin(m, held, c); },
        [&](hipStream_t st) {
            hipLaunchKernelGGL(k_held_cloud_edge_ca, dim3(blocks_for(E), (unsigned)held->d.n_shapes), dim3(WAVE), QSlabLds(m->n_q).bytes(), st,
                               m->d, held->d, cloud_dev(c), starts, goals, dist, E, max_distance, (int)mode, grasp, threshold, (int)max_iter,
                               slack, look_ahead, ca_keys(t_free));
        });
}

int32_t nbk_spline_held_cloud_continuous_batch(const nbk_model* m, const nbk_held* held, const nbk_cloud* c, const double* ctrl, int64_t S,
                                               int32_t n_ctrl, int32_t degree, const double* knots, double threshold, int32_t max_iter,
                                               double slack, double look_ahead, const double* grasp, int32_t accumulate, uint8_t* valid,
                                               double* t_free, int32_t* status, void* stream) {
    if (m == nullptr || held == nullptr || c == nullptr) return NBK_ERR_INVALID;
    return certified_splines_call(
        m, ctrl, S, n_ctrl, degree, knots, threshold, max_iter, slack, &look_ahead, &held->d.n_shapes, false, cloud_status_word(c), nullptr,
        grasp, accumulate, valid, t_free, status, stream, [&] { return held_cloud_call_begin(m, held, c); },
        [&](auto K, size_t lds, hipStream_t st) {
            hipLaunchKernelGGL(k_held_cloud_spline_ca<decltype(K)::value>, dim3(blocks_for(S), (unsigned)held->d.n_shapes), dim3(WAVE), lds,
                               st, m->d, held->d, cloud_dev(c), ctrl, S, (int)n_ctrl, knots, grasp, threshold, (int)max_iter, slack,
                               look_ahead, ca_keys(t_free));
        });
}

// ---- the host twins of the held motion bound: held_item_motion_bound on the tables motion_tables makes of the descriptor, the
// items in held_item_list's order (robot_bits in the descriptor's numbering); no GPU
static int32_t held_motion_host_begin(const nbk_model_desc* d, int32_t frame, const double* A, const double* G, int32_t H,
                                      const int32_t* shape_type, const double* shape_local, const double* shape_param, int32_t n_world,
                                      const int32_t* world_shapes, const uint64_t* robot_bits, MotionHost& mh, unsigned& mask,
                                      std::vector<double>& tab, std::vector<int>& items, const HeldHulls* hl = nullptr) {
    if (d == nullptr) return NBK_ERR_INVALID;
    { const int32_t rc = desc_check(d, D_MOTION); if (rc != NBK_OK) return rc; }
    { const int32_t rc = held_args_check(frame, d->n_joints, d->n_wshapes, A, G, H, shape_type, shape_local, shape_param, n_world, world_shapes, hl);
      if (rc != NBK_OK) return rc; }
    const std::vector<unsigned> fm = frame_masks(d);
    motion_tables(d, fm, mh);
    mask = frame >= 0 ? fm[frame] : 0u;
    std::vector<int> kind;
    held_tab(A, G, H, shape_type, shape_local, shape_param, tab, kind, hl);
    items = held_item_list(d->n_rshapes, nullptr, robot_bits, H, n_world, world_shapes);
    return NBK_OK;
}

static int32_t edge_held_motion_bounds(const nbk_model_desc* d, int32_t frame, const double* A, const double* G, int32_t H,
                                       const int32_t* shape_type, const double* shape_local, const double* shape_param, int32_t n_world,
                                       const int32_t* world_shapes, const uint64_t* robot_bits, const HeldHulls* hl, const double* starts,
                                       const double* goals, int64_t E, double* mu) {
    if (E < 0) return NBK_ERR_INVALID;
    MotionHost mh;
    unsigned mask = 0u;
    std::vector<double> tab;
    std::vector<int> items;
    { const int32_t rc = held_motion_host_begin(d, frame, A, G, H, shape_type, shape_local, shape_param, n_world, world_shapes, robot_bits, mh, mask, tab, items, hl);
      if (rc != NBK_OK) return rc; }
    const int64_t K = (int64_t)(items.size() / HELD_ITEM_LEN);
    if (E == 0 || K == 0) return NBK_OK;
    if (starts == nullptr || goals == nullptr || mu == nullptr) return NBK_ERR_INVALID;
    const MotionTab t = mh.view(d->n_joints, d->n_rshapes);
    for (int64_t e = 0; e < E; ++e)
        for (int64_t i = 0; i < K; ++i)
            mu[e * K + i] = held_item_motion_bound(t, mask, tab.data(), tab.data() + 12, &items[HELD_ITEM_LEN * (size_t)i],
                                                   EdgeMotion{starts + e * d->n_q, goals + e * d->n_q});
    return NBK_OK;
}

int32_t nbk_edge_held_motion_bounds_host(const nbk_model_desc* d, int32_t frame, const double* A, const double* G, int32_t H,
                                         const int32_t* shape_type, const double* shape_local, const double* shape_param, int32_t n_world,
                                         const int32_t* world_shapes, const uint64_t* robot_bits, const double* starts, const double* goals,
                                         int64_t E, double* mu) {
    return edge_held_motion_bounds(d, frame, A, G, H, shape_type, shape_local, shape_param, n_world, world_shapes, robot_bits, nullptr, starts,
                                   goals, E, mu);
}

int32_t nbk_edge_held_motion_bounds_hulls_host(const nbk_model_desc* d, int32_t frame, const double* A, const double* G, int32_t H,
                                               const int32_t* shape_type, const double* shape_local, const double* shape_param,
                                               int32_t n_world, const int32_t* world_shapes, const uint64_t* robot_bits, int32_t n_hulls,
                                               const int32_t* hull_vert_begin, const double* hull_verts, const int32_t* hull_face_begin,
                                               const double* hull_planes, const double* starts, const double* goals, int64_t E, double* mu) {
    const HeldHulls hl{n_hulls, hull_vert_begin, hull_verts, hull_face_begin, hull_planes};
    return edge_held_motion_bounds(d, frame, A, G, H, shape_type, shape_local, shape_param, n_world, world_shapes, robot_bits, &hl, starts,
                                   goals, E, mu);
}

static int32_t spline_held_motion_bounds(const nbk_model_desc* d, int32_t frame, const double* A, const double* G, int32_t H,
                                         const int32_t* shape_type, const double* shape_local, const double* shape_param,
                                         int32_t n_world, const int32_t* world_shapes, const uint64_t* robot_bits, const HeldHulls* hl,
                                         const double* ctrl, int64_t S, int32_t n_ctrl, int32_t degree, const double* knots, double* mu) {
    if (S < 0 || !spline_args_ok(n_ctrl, degree, nullptr)) return NBK_ERR_INVALID;
    MotionHost mh;
    unsigned mask = 0u;
    std::vector<double> tab;
    std::vector<int> items;
    { const int32_t rc = held_motion_host_begin(d, frame, A, G, H, shape_type, shape_local, shape_param, n_world, world_shapes, robot_bits, mh, mask, tab, items, hl);
      if (rc != NBK_OK) return rc; }
    const int64_t K = (int64_t)(items.size() / HELD_ITEM_LEN);
    const int nq = d->n_q, k = degree, L = n_ctrl - degree;
    if (S == 0 || K == 0) return NBK_OK;
    if (ctrl == nullptr || knots == nullptr || mu == nullptr || !spline_args_ok(n_ctrl, degree, knots)) return NBK_ERR_INVALID;
    const MotionTab t = mh.view(d->n_joints, d->n_rshapes);
    for (int64_t s = 0; s < S; ++s) {
        const double* c = ctrl + (size_t)s * (size_t)n_ctrl * nq;
        for (int ell = k; ell < n_ctrl; ++ell) {
            double* out = mu + ((size_t)s * L + (size_t)(ell - k)) * K;
            const bool span = knots[ell] < knots[ell + 1];
            const SplineSpanMotion tr{c + (size_t)(ell - k) * nq, knots + (ell - k + 1), nq, k};
            for (int64_t i = 0; i < K; ++i)
                out[i] = span ? held_item_motion_bound(t, mask, tab.data(), tab.data() + 12, &items[HELD_ITEM_LEN * (size_t)i], tr) : 0.0;
        }
    }
    return NBK_OK;
}

int32_t nbk_spline_held_motion_bounds_host(const nbk_model_desc* d, int32_t frame, const double* A, const double* G, int32_t H,
                                           const int32_t* shape_type, const double* shape_local, const double* shape_param,
                                           int32_t n_world, const int32_t* world_shapes, const uint64_t* robot_bits, const double* ctrl,
                                           int64_t S, int32_t n_ctrl, int32_t degree, const double* knots, double* mu) {
    return spline_held_motion_bounds(d, frame, A, G, H, shape_type, shape_local, shape_param, n_world, world_shapes, robot_bits, nullptr, ctrl,
                                     S, n_ctrl, degree, knots, mu);
}

int32_t nbk_spline_held_motion_bounds_hulls_host(const nbk_model_desc* d, int32_t frame, const double* A, const double* G, int32_t H,
                                                 const int32_t* shape_type, const double* shape_local, const double* shape_param,
                                                 int32_t n_world, const int32_t* world_shapes, const uint64_t* robot_bits, int32_t n_hulls,
                                                 const int32_t* hull_vert_begin, const double* hull_verts, const int32_t* hull_face_begin,
                                                 const double* hull_planes, const double* ctrl, int64_t S, int32_t n_ctrl, int32_t degree,
                                                 const double* knots, double* mu) {
    const HeldHulls hl{n_hulls, hull_vert_begin, hull_verts, hull_face_begin, hull_planes};
    return spline_held_motion_bounds(d, frame, A, G, H, shape_type, shape_local, shape_param, n_world, world_shapes, robot_bits, &hl, ctrl,
                                     S, n_ctrl, degree, knots, mu);
}

// ---- the host twins of the per-shape bound the held-versus-cloud lanes advance with: motion_terms over the whole holding path for
// each held shape (HeldCloudEdgeLane::enter, HeldCloudSplineLane::span_bound), with the stored grasp G; no item list, no GPU.  One body
// per trajectory kind: the *_hulls_host names pass the hull tables (held_args_check puts them through desc_check's hull rules),
// the names without them pass none and refuse a hull shape
static int32_t edge_held_shape_motion_bounds(const nbk_model_desc* d, int32_t frame, const double* A, const double* G, int32_t H,
                                             const int32_t* shape_type, const double* shape_local, const double* shape_param,
                                             const HeldHulls* hl, const double* starts, const double* goals, int64_t E, double* mu) {
    if (E < 0) return NBK_ERR_INVALID;
    MotionHost mh;
    unsigned mask = 0u;
    std::vector<double> tab;
    std::vector<int> items;
    { const int32_t rc = held_motion_host_begin(d, frame, A, G, H, shape_type, shape_local, shape_param, 0, nullptr, nullptr, mh, mask, tab, items, hl);
      if (rc != NBK_OK) return rc; }
    if (E == 0) return NBK_OK;
    if (starts == nullptr || goals == nullptr || mu == nullptr) return NBK_ERR_INVALID;
    const MotionTab t = mh.view(d->n_joints, d->n_rshapes);
    for (int64_t e = 0; e < E; ++e)
        for (int32_t h = 0; h < H; ++h) {
            const MotionShape hs = held_motion_shape(mask, tab.data(), tab.data() + 12, h);
            mu[e * H + h] = motion_terms(t, hs, hs.mask, EdgeMotion{starts + e * d->n_q, goals + e * d->n_q}, 0.0);
        }
    return NBK_OK;
}

int32_t nbk_edge_held_shape_motion_bounds_host(const nbk_model_desc* d, int32_t frame, const double* A, const double* G, int32_t H,
                                               const int32_t* shape_type, const double* shape_local, const double* shape_param,
                                               const double* starts, const double* goals, int64_t E, double* mu) {
    return edge_held_shape_motion_bounds(d, frame, A, G, H, shape_type, shape_local, shape_param, nullptr, starts, goals, E, mu);
}

int32_t nbk_edge_held_shape_motion_bounds_hulls_host(const nbk_model_desc* d, int32_t frame, const double* A, const double* G, int32_t H,
                                                     const int32_t* shape_type, const double* shape_local, const double* shape_param,
                                                     int32_t n_hulls, const int32_t* hull_vert_begin, const double* hull_verts,
                                                     const int32_t* hull_face_begin, const double* hull_planes, const double* starts,
                                                     const double* goals, int64_t E, double* mu) {
    const HeldHulls hl{n_hulls, hull_vert_begin, hull_verts, hull_face_begin, hull_planes};
    return edge_held_shape_motion_bounds(d, frame, A, G, H, shape_type, shape_local, shape_param, &hl, starts, goals, E, mu);
}

static int32_t spline_held_shape_motion_bounds(const nbk_model_desc* d, int32_t frame, const double* A, const double* G, int32_t H,
                                               const int32_t* shape_type, const double* shape_local, const double* shape_param,
                                               const HeldHulls* hl, const double* ctrl, int64_t S, int32_t n_ctrl, int32_t degree,
                                               const double* knots, double* mu) {
    if (S < 0 || !spline_args_ok(n_ctrl, degree, nullptr)) return NBK_ERR_INVALID;
    MotionHost mh;
    unsigned mask = 0u;
    std::vector<double> tab;
    std::vector<int> items;
    { const int32_t rc = held_motion_host_begin(d, frame, A, G, H, shape_type, shape_local, shape_param, 0, nullptr, nullptr, mh, mask, tab, items, hl);
      if (rc != NBK_OK) return rc; }
    const int nq = d->n_q, k = degree, L = n_ctrl - degree;
    if (S == 0) return NBK_OK;
    if (ctrl == nullptr || knots == nullptr || mu == nullptr || !spline_args_ok(n_ctrl, degree, knots)) return NBK_ERR_INVALID;
    const MotionTab t = mh.view(d->n_joints, d->n_rshapes);
    for (int64_t s = 0; s < S; ++s) {
        const double* c = ctrl + (size_t)s * (size_t)n_ctrl * nq;
        for (int ell = k; ell < n_ctrl; ++ell) {
            double* out = mu + ((size_t)s * L + (size_t)(ell - k)) * H;
            const bool span = knots[ell] < knots[ell + 1];
            const SplineSpanMotion tr{c + (size_t)(ell - k) * nq, knots + (ell - k + 1), nq, k};
            for (int32_t h = 0; h < H; ++h) {
                const MotionShape hs = held_motion_shape(mask, tab.data(), tab.data() + 12, h);
                out[h] = span ? motion_terms(t, hs, hs.mask, tr, 0.0) : 0.0;
            }
        }
    }
    return NBK_OK;
}

int32_t nbk_spline_held_shape_motion_bounds_host(const nbk_model_desc* d, int32_t frame, const double* A, const double* G, int32_t H,
                                                 const int32_t* shape_type, const double* shape_local, const double* shape_param,
                                                 const double* ctrl, int64_t S, int32_t n_ctrl, int32_t degree, const double* knots,
                                                 double* mu) {
    return spline_held_shape_motion_bounds(d, frame, A, G, H, shape_type, shape_local, shape_param, nullptr, ctrl, S, n_ctrl, degree, knots, mu);
}

int32_t nbk_spline_held_shape_motion_bounds_hulls_host(const nbk_model_desc* d, int32_t frame, const double* A, const double* G, int32_t H,
                                                       const int32_t* shape_type, const double* shape_local, const double* shape_param,
                                                       int32_t n_hulls, const int32_t* hull_vert_begin, const double* hull_verts,
                                                       const int32_t* hull_face_begin, const double* hull_planes, const double* ctrl,
                                                       int64_t S, int32_t n_ctrl, int32_t degree, const double* knots, double* mu) {
    const HeldHulls hl{n_hulls, hull_vert_begin, hull_verts, hull_face_begin, hull_planes};
    return spline_held_shape_motion_bounds(d, frame, A, G, H, shape_type, shape_local, shape_param, &hl, ctrl, S, n_ctrl, degree, knots, mu);
}

}  // extern "C"
