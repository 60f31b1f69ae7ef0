// Pieces of the float32 broadphase that the ahead-of-time k_broad_f32<S, WH> (nbk.hip) and the per-robot k_broad_f32_spec
// (nbk_bf32_spec.hpp, compiled with hipRTC) share: ONE definition of the slot-table layout k_prepare_f32 writes (ftab_offsets),
// of the packed chain-sweep joints, of sincos_f, of slot_e2, of the plain-row q staging, of the queue appends (enqueue_lanes,
// queue_room, drain_bits), of the queue flush and of the mask epilogue -- both kernels compile these.  The float64 broadphases
// of nbk.hip (k_broad, k_broad_reg) take drain_bits and write_mask from here as well.
//
// The per-slot tests below (box_slot2 ... robot_slot_gen) are the specialised kernel's; k_broad_f32 keeps the same statements
// inline.  Calling them from k_broad_f32 changes its register allocation at the 5-waves-per-SIMD bound: with the general stage
// through them every instance spills more (scratch bytes <12, false> 108 -> 124, <16, false> 176 -> 224, <16, true> 176 -> 208;
// with the fast stage alone 108 -> 116) and <12, false> runs 0.9-2.3 us of 121 us slower on 1e6 plain rows of c2, also with the
// results returned by value (the same code) or the stages apart (profiles/r11_a_broad_dedupe.log).  So a change to a slot test
// is made here AND in k_broad_f32, and tests/test_broad_spec.py compares the two kernels' masks over both stages.
//
// Self-contained for hipRTC: no includes, nothing beyond what hiprtc supplies.  nbk.hip includes it at file scope; build.py
// embeds it into libnbk.so next to nbk_bf32_spec.hpp, and source_digest() covers it.
#ifndef NBK_BF32_COMMON_HPP
#define NBK_BF32_COMMON_HPP

#define NBK_BF32_DEV __device__ __forceinline__

namespace nbk {

constexpr int WAVE = 64;
constexpr int BQ_CAP = 512;             // per-wave LDS staging of queue items before one global append
constexpr int CNT_STRIDE = 16;          // one 128-byte line per queue counter

typedef float V2f __attribute__((ext_vector_type(2)));
typedef int V2i __attribute__((ext_vector_type(2)));
struct alignas(64) Row16f { float v[16]; };     // one row of a [.][16] slot table: a single s_load_dwordx16

// ---- the per-call slot tables (k_prepare_f32 writes them, both broadphases read them; float offsets from the table start) ---------
// every [.][16] table starts on a multiple of 16 floats from the table (itself 64-byte aligned): a row is one s_load_dwordx16
struct FTabOffsets { int rkey, rp, rcert, rptri, rneg, rnd, wkey, wtc, wp, wcert, wcin, wkey2, rho, n_reach, wlist, wbx; };
__host__ __device__ constexpr FTabOffsets ftab_offsets(int W) {
    const int w16 = W * 16;
    const int wkey = 1408, wtc = wkey + w16, rho = wtc + 5 * w16, n_reach = rho + 32, wlist = n_reach + 16;
    return FTabOffsets{0, 256, 512, 768, 896, 1152, wkey, wtc, wtc + w16, wtc + 2 * w16, wtc + 3 * w16, wtc + 4 * w16, rho, n_reach, wlist,
                       wlist + ((W + 15) & ~15)};
}

NBK_BF32_DEV V2f splat2(float x) { return V2f{x, x}; }
NBK_BF32_DEV V2f fma2(V2f a, V2f b, V2f c) { return __builtin_elementwise_fma(a, b, c); }

// sin / cos for the conservative float32 sweep: the hardware's v_sin_f32 / v_cos_f32 on the fractional part of x / 2 pi (five
// instructions where the Cody-Waite + Taylor form took 22).  Measured on the device over |x| <= 64 (tools: profiles/r03_hw_sincos.log):
// absolute error <= 2.7e-7 for |x| <= 3.2 and <= 2.7e-7 + 4e-8 |x| beyond (the rounding of x / 2 pi) -- inside what the slack
// charges per joint (16 ulp = 9.5e-7 for the sweep, 2.4e-7 |q| for the angle, both times 50)
NBK_BF32_DEV void sincos_f(float x, float& s, float& c) {
    const float r = x * 0.15915494309189535f;
    const float f = r - __builtin_rintf(r);
    s = __builtin_amdgcn_sinf(f);
    c = __builtin_amdgcn_cosf(f);
}

// |d|^2 + nk as one fma chain, for two slots at a time (v_pk_fma_f32) and for one: the same operations in the same order, so the
// one-slot form reproduces the pair form's value bit for bit (the rare enqueue path re-evaluates what the row's sign bits flagged)
NBK_BF32_DEV V2f slot_e2(V2f dx, V2f dy, V2f dz, V2f nk) {
    return __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, __builtin_elementwise_fma(dx, dx, nk)));
}
NBK_BF32_DEV float slot_e1(float dx, float dy, float dz, float nk) { return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, nk))); }

// ---- the packed float32 sweep --------------------------------------------------------------------------------------------------
// A frame as rows 0 and 1 of every column in one register PAIR (Rc[k] = (R[0][k], R[1][k]), tc = (t[0], t[1])) and row 2 apart:
// R x L and R x v then run rows 0 and 1 together on v_pk_fma_f32 (one issue slot for two multiply-adds; plain float32 and packed
// float32 instructions issue at the same rate on this SIMD, profiles/r03_valu_issue_rate.log): 27 instructions per axis-aligned
// joint instead of 48, 6 per shape centre instead of 9.
struct XfP { V2f Rc[3]; float R2[3]; V2f tc; float t2; };
// host-made constants of one joint (f_tab + f_pk + 20 k): for a joint about coordinate axis KZ of its frame, U = KZ + 1, V = KZ + 2
struct alignas(16) JPk { float m2p[6]; float m1p[6]; float mk[3]; float pad0; float toff[3]; float pad1; };

template <int KZ>
NBK_BF32_DEV void joint_apply_axis_p(const JPk& jp, const XfP& P, float s, float c, XfP& o) {
    constexpr int U = (KZ + 1) % 3, V = (KZ + 2) % 3;
    const V2f s2 = splat2(s), c2 = splat2(c);
    V2f Lp[3];                                                     // (L[r][U], L[r][V]) = s M2 - c M1
#pragma unroll
    for (int r = 0; r < 3; ++r) Lp[r] = fma2(s2, V2f{jp.m2p[2 * r], jp.m2p[2 * r + 1]}, -(c2 * V2f{jp.m1p[2 * r], jp.m1p[2 * r + 1]}));
    const V2f cu = fma2(P.Rc[2], splat2(Lp[2].x), fma2(P.Rc[1], splat2(Lp[1].x), P.Rc[0] * splat2(Lp[0].x)));
    const V2f cv = fma2(P.Rc[2], splat2(Lp[2].y), fma2(P.Rc[1], splat2(Lp[1].y), P.Rc[0] * splat2(Lp[0].y)));
    const V2f ck = fma2(P.Rc[2], splat2(jp.mk[2]), fma2(P.Rc[1], splat2(jp.mk[1]), P.Rc[0] * splat2(jp.mk[0])));
    const V2f r2 = fma2(splat2(P.R2[2]), Lp[2], fma2(splat2(P.R2[1]), Lp[1], splat2(P.R2[0]) * Lp[0]));        // row 2, columns U and V
    const float r2k = __builtin_fmaf(P.R2[2], jp.mk[2], __builtin_fmaf(P.R2[1], jp.mk[1], P.R2[0] * jp.mk[0]));
    const V2f tc = fma2(P.Rc[2], splat2(jp.toff[2]), fma2(P.Rc[1], splat2(jp.toff[1]), fma2(P.Rc[0], splat2(jp.toff[0]), P.tc)));
    const float t2 = __builtin_fmaf(P.R2[2], jp.toff[2], __builtin_fmaf(P.R2[1], jp.toff[1], __builtin_fmaf(P.R2[0], jp.toff[0], P.t2)));
    o.Rc[U] = cu; o.Rc[V] = cv; o.Rc[KZ] = ck;
    o.R2[U] = r2.x; o.R2[V] = r2.y; o.R2[KZ] = r2k;
    o.tc = tc; o.t2 = t2;
}

// joints that are not about a coordinate axis (general revolute, prismatic): M = f_tab + 27 k, toff / sl their translation / slide
NBK_BF32_DEV void joint_apply_gen_p(const float* M, const float* toff, const float* sl, const XfP& P, float qk, float s, float c, XfP& o) {
    float L[9], tl[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) L[e] = __builtin_fmaf(s, M[18 + e], __builtin_fmaf(-c, M[9 + e], M[e]));
#pragma unroll
    for (int i = 0; i < 3; ++i) tl[i] = __builtin_fmaf(qk, sl[i], toff[i]);
    XfP n;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        n.Rc[j] = fma2(P.Rc[2], splat2(L[6 + j]), fma2(P.Rc[1], splat2(L[3 + j]), P.Rc[0] * splat2(L[j])));
        n.R2[j] = __builtin_fmaf(P.R2[2], L[6 + j], __builtin_fmaf(P.R2[1], L[3 + j], P.R2[0] * L[j]));
    }
    n.tc = fma2(P.Rc[2], splat2(tl[2]), fma2(P.Rc[1], splat2(tl[1]), fma2(P.Rc[0], splat2(tl[0]), P.tc)));
    n.t2 = __builtin_fmaf(P.R2[2], tl[2], __builtin_fmaf(P.R2[1], tl[1], __builtin_fmaf(P.R2[0], tl[0], P.t2)));
    o = n;
}

// ---- fast-stage slot tests (every lane within the static slack bound: all thresholds are scalars) -------------------------------
// World BOX, two robot shapes (2i, 2i + 1) per call, no branch and no lane mask per slot: the centre's squared distance dd to the
// box centre and ex2 to the (core) box itself -- ex_j = |d . axis_j| - h_j, clamped at 0, squared and summed -- and mx = max_j ex_j
// (< 0: the centre is inside).  Every verdict is the sign of a difference with a per-slot scalar of wbx (tb = wbx + w * 96 + 12 i):
//   candidate  dd < wkey2 (bounding spheres) and ex2 < cull2 (closer to the box than tc+ + rho + slack)
//   certain hit, outside  candidate, ex2 > 0 and ex2 < cin (inside the ball inscribed in the shape, slack taken off)
//   certain hit, inside   candidate, mx < 0, mx < -g (deeper than -tc + slack) and dd < kin
// ALIGNED: the box's axes at wc[3..11] are exactly (1,0,0), (0,1,0), (0,0,1) and can never change (an immovable descriptor; the
// generated Spec says so), and the projections are the differences themselves.  For finite differences that is the value of the
// fma chain -- dx * 1 = dx, fma(dy, 0, dx) and fma(dz, 0, .) round to their addend -- up to the sign of a zero, which fabs
// removes; a row with a non-finite q is `hit` before any slot.
template <bool ALIGNED = false>
NBK_BF32_DEV void box_slot2(V2f dx, V2f dy, V2f dz, const float* wc, const float* tb, V2i& cand, V2i& certh) {
    const V2f dd = fma2(dz, dz, fma2(dy, dy, dx * dx));
    V2f ex[3], ex2 = V2f{0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        V2f pj;
        if constexpr (ALIGNED) pj = j == 0 ? dx : (j == 1 ? dy : dz);
        else pj = fma2(dz, splat2(wc[5 + 3 * j]), fma2(dy, splat2(wc[4 + 3 * j]), dx * splat2(wc[3 + 3 * j])));
        ex[j] = V2f{__builtin_fabsf(pj.x) - wc[12 + j], __builtin_fabsf(pj.y) - wc[12 + j]};
        const V2f cl = V2f{__builtin_fmaxf(ex[j].x, 0.0f), __builtin_fmaxf(ex[j].y, 0.0f)};
        ex2 = fma2(cl, cl, ex2);
    }
    const V2f mx = V2f{__builtin_fmaxf(ex[0].x, __builtin_fmaxf(ex[1].x, ex[2].x)), __builtin_fmaxf(ex[0].y, __builtin_fmaxf(ex[1].y, ex[2].y))};
    const V2i s1 = __builtin_bit_cast(V2i, dd - V2f{tb[0], tb[1]});
    const V2i s2 = __builtin_bit_cast(V2i, ex2 - V2f{tb[2], tb[3]});
    const V2i s3 = __builtin_bit_cast(V2i, ex2 - V2f{tb[4], tb[5]});
    const V2i s4 = __builtin_bit_cast(V2i, dd - V2f{tb[6], tb[7]});
    const V2i s5 = __builtin_bit_cast(V2i, mx + V2f{tb[8], tb[9]});
    const V2i nz = __builtin_bit_cast(V2i, V2f{0.0f, 0.0f} - ex2);         // sign set <=> ex2 > 0 (a true subtraction: +0 - +0 = +0)
    const V2i mi = __builtin_bit_cast(V2i, mx);
    cand = s1 & s2;
    certh = cand & ((s3 & nz) | (mi & s5 & s4));
}

// World HULL, the box slot's form with the hull's local bounding box ob (centre, half extents): candidate = bounding spheres (dd <
// wkey2) and the centre closer to that box than tc+ + rho + slack (a cull only: the box contains the hull); certain hit = the
// inscribed balls (dd < cert)
NBK_BF32_DEV void hull_slot2(V2f dx, V2f dy, V2f dz, const float* wc, const float* ob, const float* tb, V2i& cand, V2i& certh) {
    const V2f dd = fma2(dz, dz, fma2(dy, dy, dx * dx));
    V2f ex2 = V2f{0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const V2f pj = fma2(dz, splat2(wc[5 + 3 * j]), fma2(dy, splat2(wc[4 + 3 * j]), dx * splat2(wc[3 + 3 * j]))) - splat2(ob[j]);
        const V2f cl = V2f{__builtin_fmaxf(__builtin_fabsf(pj.x) - ob[3 + j], 0.0f), __builtin_fmaxf(__builtin_fabsf(pj.y) - ob[3 + j], 0.0f)};
        ex2 = fma2(cl, cl, ex2);
    }
    const V2i s1 = __builtin_bit_cast(V2i, dd - V2f{tb[0], tb[1]});
    const V2i s2 = __builtin_bit_cast(V2i, ex2 - V2f{tb[2], tb[3]});
    certh = __builtin_bit_cast(V2i, dd - V2f{tb[4], tb[5]});
    cand = s1 & s2;
}

// World PLANE / SPHERE-like slot of the fast stage: one compare against the squared (planes: height) candidate threshold and one
// against the certification threshold
NBK_BF32_DEV void plane_slot1(float dx, float dy, float dz, const float* wc, float key2, float cert, bool& cand, bool& certh) {
    const float hc = __builtin_fmaf(dz, wc[11], __builtin_fmaf(dy, wc[10], dx * wc[9]));
    cand = hc < key2;
    certh = certh || (hc < cert);
}
NBK_BF32_DEV void sphere_slot1(float dx, float dy, float dz, float key2, float cert, bool& cand, bool& certh) {
    const float dd = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    cand = dd < key2;
    certh = certh || (dd < cert);
}

// ---- general-stage slot tests (some lane's slack e2 exceeds the static bound) -----------------------------------------------------
// planes: candidate unless hc - rhoA >= key + e2; certain hit when the inscribed ball dips below the plane (hc < cert)
NBK_BF32_DEV bool plane_slot_gen(float dx, float dy, float dz, const float* wc, float key, float rhoA, float e2, float cert, bool& certh) {
    const float hc = __builtin_fmaf(dz, wc[11], __builtin_fmaf(dy, wc[10], dx * wc[9]));
    certh = certh || (hc < cert);
    return !((hc - rhoA) >= key + e2);
}
// boxes: bounding spheres, then -- only when some lane of the wave passed them -- the midphase on the exact box (distance of the
// centre outside, depth inside).  rs = sphere key, tc = contact threshold, cin = squared certification distance to the core box
template <class H>
NBK_BF32_DEV bool box_slot_gen(float dx, float dy, float dz, const float* wc, float rs, float tc, float rho, float e2, float cin,
                               bool& certh, H& hit) {
    const float up = 1.0f + 2.4e-7f;
    const float dd = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    const float r = rs + e2;
    bool cand = rs >= 0.0f && dd < r * r * up;
    if (__builtin_amdgcn_ballot_w64(cand) != 0ull) {
        float ex2 = 0.0f, g = 3.4e38f;
        bool inside = true;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float axj = __builtin_fabsf(__builtin_fmaf(dz, wc[5 + 3 * j], __builtin_fmaf(dy, wc[4 + 3 * j], dx * wc[3 + 3 * j])));
            const float exj = axj - wc[12 + j];
            if (exj > 0.0f) { inside = false; ex2 = __builtin_fmaf(exj, exj, ex2); }
            g = __builtin_fminf(g, wc[12 + j] - axj);
        }
        if (!inside) {
            // outside by more than the slack in every float64 reading: free when far enough (tc >= 0 only)
            const float rr = ((tc > 0.0f ? tc : 0.0f) + rho) + e2;       // tc < 0: disjoint is enough (device-only cull)
            if (ex2 >= rr * rr * up) cand = false;
            // the centre is closer to the box than the radius of the ball inscribed in the shape: certain hit
            if (cand && ex2 < cin) certh = true;
        } else if (cand && g > -tc + e2 && rs > e2 && dd * up < (rs - e2) * (rs - e2)) {
            hit = true;         // inside deeper than -tc, and inside the sphere test, in float64 as well: certain hit
        }
    }
    return cand;
}
// the other kinds: bounding spheres; hulls (ob = local bounding box) add the cull against that box; certain hit = inscribed balls
NBK_BF32_DEV bool other_slot_gen(float dx, float dy, float dz, const float* wc, const float* ob, bool is_hull, float rs, float tc, float rho,
                                 float e2, float cert, bool& certh) {
    const float up = 1.0f + 2.4e-7f;
    const float r = rs + e2;
    const float dd = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    bool cand = rs >= 0.0f && dd < r * r * up;
    if (is_hull && __builtin_amdgcn_ballot_w64(cand) != 0ull) {
        float ex2 = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float xj = __builtin_fmaf(dz, wc[5 + 3 * j], __builtin_fmaf(dy, wc[4 + 3 * j], dx * wc[3 + 3 * j])) - ob[j];
            const float exj = __builtin_fabsf(xj) - ob[3 + j];
            if (exj > 0.0f) ex2 = __builtin_fmaf(exj, exj, ex2);
        }
        const float rr = ((tc > 0.0f ? tc : 0.0f) + rho) + e2;
        if (ex2 >= rr * rr * up) cand = false;
    }
    certh = certh || (dd < cert);           // inscribed balls overlap
    return cand;
}
// robot-robot slot of the general stage: candidate iff the centres are closer than the sphere key + e2; certain hit below rcert
NBK_BF32_DEV bool robot_slot_gen(float dx, float dy, float dz, float rs, float e2, float cert, bool& certh) {
    const float up = 1.0f + 2.4e-7f;
    const float r = rs + e2;
    const float dd = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    certh = certh || (dd < cert);
    return rs >= 0.0f && dd < r * r * up;
}

// ---- plain q rows ---------------------------------------------------------------------------------------------------------------
// rows [base, base + rows_i) of q[.][nq] into the block's row-major slab lds_raw[64][nq] (lane reads lds_raw[lane * nq + j]): 16-byte
// loads where the slab is full, else scalar ones and zeros for the rows past the batch
NBK_BF32_DEV void stage_plain_rows(const double* __restrict__ q, long long base, int rows_i, int nq, double* lds_raw, int lane) {
    const int total = rows_i * nq;
    const double* src = q + base * nq;
    if (rows_i == WAVE && ((reinterpret_cast<unsigned long long>(src) & 15) == 0) && (total % 2 == 0)) {
        const double2* s2 = reinterpret_cast<const double2*>(src);
        double2* d2 = reinterpret_cast<double2*>(lds_raw);
        for (int i = lane; i < total / 2; i += WAVE) d2[i] = s2[i];
    } else {
        for (int i = lane; i < total; i += WAVE) lds_raw[i] = src[i];
        for (int i = total + lane; i < WAVE * nq; i += WAVE) lds_raw[i] = 0.0;
    }
}

// ---- queue flush ------------------------------------------------------------------------------------------------------------------
// Items are routed by the kind class of their pair (vp_cls: box-box, box-cylinder, cylinder-cylinder, the rest): class c owns
// `groups(c)` (at least 1) of the sub-queues from `base(c)` on, in proportion to its pairs; a block appends to the (block %
// groups)-th.  The chunks k_narrow takes are then kind-homogeneous -- one core layout, one support routine per side -- which is worth
// 10 % of its time; one atomicAdd per class present, issued together by lanes 0-3.  Route: cls(pair) / base(c) / groups(c).
template <class Route>
NBK_BF32_DEV void flush_items_r(const Route& rt, unsigned* lds_queue, int qn, long long base_cfg, unsigned long long* q_count,
                                unsigned long long* q_items, unsigned long long cap_sub, int lane, unsigned char* ovf) {
    __syncthreads();
    for (int i0 = 0; i0 < qn; i0 += WAVE) {
        const int i = i0 + lane;
        const bool has = i < qn;
        const unsigned it = has ? lds_queue[i] : 0u;
        const int cls = has ? rt.cls(it >> 6) : 0;
        unsigned long long bc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) bc[c] = __builtin_amdgcn_ballot_w64(has && cls == c);
        const unsigned long long mine_cnt = lane == 0 ? bc[0] : (lane == 1 ? bc[1] : (lane == 2 ? bc[2] : bc[3]));
        unsigned long long off = 0;
        if (lane < 4 && mine_cnt != 0ull)
            off = atomicAdd(q_count + (unsigned long long)(rt.base(lane) + (int)(blockIdx.x % (unsigned)rt.groups(lane))) * CNT_STRIDE,
                            (unsigned long long)__builtin_popcountll(mine_cnt));
        const unsigned olo = (unsigned)__builtin_amdgcn_ds_bpermute(cls * 4, (int)(unsigned)off);
        const unsigned ohi = (unsigned)__builtin_amdgcn_ds_bpermute(cls * 4, (int)(unsigned)(off >> 32));
        if (has) {
            const unsigned long long mb_ = cls == 0 ? bc[0] : (cls == 1 ? bc[1] : (cls == 2 ? bc[2] : bc[3]));
            const unsigned long long slot = (((unsigned long long)ohi << 32) | olo) +
                                            __builtin_amdgcn_mbcnt_hi((unsigned)(mb_ >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mb_, 0u));
            const unsigned sub = (unsigned)(rt.base(cls) + (int)(blockIdx.x % (unsigned)rt.groups(cls)));
            const unsigned long long b = (unsigned long long)(base_cfg + (it & 63u));
            if (slot < cap_sub) q_items[(unsigned long long)sub * cap_sub + slot] = (b << 20) | (unsigned long long)(it >> 6);
            else if (ovf != nullptr) ovf[blockIdx.x] = 1;          // the sub-queue is full: this block is re-decided without a queue
        }
    }
    __syncthreads();
}

// ---- queue appends ----------------------------------------------------------------------------------------------------------------
// One append: the lanes with `cond` get consecutive slots behind the pending items.  No "nearly full" test here: queue_room makes
// room for a whole row of slots before the row's appends start.
NBK_BF32_DEV void enqueue_lanes(bool cond, unsigned pair, unsigned* lds_queue, int& qn, int lane) {
    const unsigned long long cm = __builtin_amdgcn_ballot_w64(cond);
    if (cm != 0ull) {
        if (cond) {
            const int pos = qn + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(cm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)cm, 0u));
            lds_queue[pos] = (pair << 6) | (unsigned)lane;
        }
        qn += __builtin_popcountll(cm);
    }
}
// flush unless `need` more items fit a staging area of `qcap` items
template <class Route>
NBK_BF32_DEV void queue_room(int need, int qcap, const Route& rt, unsigned* lds_queue, int& qn, long long base_cfg, unsigned long long* q_count,
                             unsigned long long* q_items, unsigned long long cap_sub, int lane, unsigned char* ovf) {
    if (qn > qcap - need) { flush_items_r(rt, lds_queue, qn, base_cfg, q_count, q_items, cap_sub, lane, ovf); qn = 0; }
}
// Survivor bits -> items: every lane holds one bit per surviving slot of a row; each trip takes the lowest bit of every lane that
// has one left, so a trip appends at most WAVE items and the staging area (BQ_CAP) is flushed once fewer than WAVE are free.
// pair_of(bit): the pair index of that slot (PairTab: a row of a pair-index table).
struct PairTab {
    const int* t;
    NBK_BF32_DEV unsigned operator()(int bit) const { return (unsigned)t[bit]; }
};
template <class PairOf, class Route>
NBK_BF32_DEV void drain_bits(unsigned long long bits, const PairOf& pair_of, const Route& rt, unsigned* lds_queue, int& qn, long long base_cfg,
                             unsigned long long* q_count, unsigned long long* q_items, unsigned long long cap_sub, int lane, unsigned char* ovf) {
    while (true) {
        const bool has = bits != 0ull;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(has);
        if (bal == 0ull) break;
        if (has) {
            const int bit = __builtin_ctzll(bits);
            bits &= bits - 1ull;
            const int pos = qn + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
            lds_queue[pos] = (pair_of(bit) << 6) | (unsigned)lane;
        }
        qn += __builtin_popcountll(bal);
        queue_room(WAVE, BQ_CAP, rt, lds_queue, qn, base_cfg, q_count, q_items, cap_sub, lane, ovf);
    }
}

// ---- mask epilogue ----------------------------------------------------------------------------------------------------------------
// one bit per configuration of the block (and / or one byte): the hits decided so far; the narrowphase ORs the rest in
template <class Word>
NBK_BF32_DEV void write_mask(bool hit, bool active, long long base, int lane, Word* mask_bits, unsigned char* mask_bytes) {
    const unsigned long long word = __builtin_amdgcn_ballot_w64(hit && active);
    if (mask_bits != nullptr && lane == 0) mask_bits[blockIdx.x] = word;
    if (mask_bytes != nullptr && active) mask_bytes[base + lane] = hit ? 1 : 0;
}

}  // namespace nbk

#endif  // NBK_BF32_COMMON_HPP
