// The float32 fast path of k_broad_f32, compiled at run time for ONE robot (hipRTC): k_broad_f32_spec.
//
// nbk.hip generates a `struct Spec` from a descriptor's tables (bf32_spec_text) and compiles it in front of this file.  What is
// fixed for a descriptor becomes a compile-time constant: the joint kinds and q columns of the chain, which shapes hang off
// which frame, the real robot-robot and robot-world slots and their pair indices, the world shapes and their kinds, the
// float32 table offsets.  What depends on the threshold stays in the table k_prepare_f32 writes (same layout as for the
// generic kernel).  With every index a constant, the centres are plain registers: no VGPR indexing, no v_readlane broadcast
// of the shape offsets, no z coordinates parked in LDS; and groups of two slots (2i, 2i + 1) that hold no pair are not
// computed at all.
//
// The arithmetic of every slot that IS computed is the generic kernel's, operation for operation (same fma chains, same
// table values), and the float32 stage only culls or certifies with the same conservative thresholds: every survivor is
// decided again in float64 by k_narrow_*, so the masks are those of the generic kernel.
//
// The table layout, the sweep joint, the plain-row q staging, the queue appends and flush and the mask epilogue are
// nbk_bf32_common.hpp's: the functions k_broad_f32 calls as well.  The per-slot tests are that header's too; k_broad_f32 keeps
// the same statements inline (see the header for why).  What is here is the specialised control flow around them.  nbk.hip hands hipRTC the generated Spec, then nbk_bf32_common.hpp, then this file.  Self-contained for hipRTC:
// no host headers, nothing beyond what hiprtc supplies.

// Compile-time switches, reachable through NBK_JIT_OPTIONS (diagnostics; the product path defines none):
//   NBK_SPEC_NO_ALIGNED, NBK_SPEC_NO_QREG   one of the two trims below off (same masks): the axis-aligned box slot, the q rows
//       loaded straight into registers
//   NBK_SPEC_NO_FOLD   the chain sweep without the folded tables (same masks): the unfolded sweep alone
//   NBK_SPEC_FOLD_PARTS=<bits>   the folded sweep with only one of its parts (same masks; for measuring them apart): 1 the
//       axis-aligned joints, 2 the shape centres
//   NBK_SPEC_DIAG_NO_WORLD, NBK_SPEC_DIAG_NO_RR, NBK_SPEC_DIAG_NO_ENQUEUE   the fast stage without its world blocks / its robot-robot
//       rows / its queue appends: WRONG masks, for attributing instructions and time only (tools/spec_variant.sh)
#ifdef NBK_SPEC_NO_ALIGNED
#define NBK_SPEC_ALIGNED 0
#else
#define NBK_SPEC_ALIGNED 1
#endif
#ifdef NBK_SPEC_NO_QREG
#define NBK_SPEC_QREG 0
#else
#define NBK_SPEC_QREG 1
#endif
#ifdef NBK_SPEC_NO_FOLD
#define NBK_SPEC_FOLD 0
#else
#define NBK_SPEC_FOLD 1
#endif
#ifndef NBK_SPEC_FOLD_PARTS
#define NBK_SPEC_FOLD_PARTS 3
#endif
#ifdef NBK_SPEC_DIAG_NO_WORLD
#define NBK_SPEC_WORLD 0
#else
#define NBK_SPEC_WORLD 1
#endif
#ifdef NBK_SPEC_DIAG_NO_RR
#define NBK_SPEC_RR 0
#else
#define NBK_SPEC_RR 1
#endif
#ifdef NBK_SPEC_DIAG_NO_ENQUEUE
#define NBK_SPEC_ENQUEUE 0
#else
#define NBK_SPEC_ENQUEUE 1
#endif

#define NBK_SPEC_DEV __device__ __forceinline__
#define NBK_SPEC_INLINE __attribute__((always_inline))      // every lambda of the kernel: its captures must stay registers

namespace nbk_spec {

using namespace nbk;            // nbk_bf32_common.hpp: the table layout, the sweep joint, the slot tests, the queue appends and flush
enum { K_BOX = 2, K_HULL = 4, K_PLANE = 5 };
enum { JK_PRISMATIC = 4 };

template <int V> struct IC { static constexpr int value = V; };
// compile-time loop: f(IC<I>{}) for I = B .. E-1
template <int B, int E, class F> NBK_SPEC_DEV void sfor(F&& f) {
    if constexpr (B < E) { f(IC<B>{}); sfor<B + 1, E>(f); }
}

// queue routing of the descriptor as constants (flush_items_r)
template <class Spec> struct SpecRoute {
    const int* __restrict__ vp_cls;
    NBK_SPEC_DEV int cls(unsigned p) const { return vp_cls[p]; }
    NBK_SPEC_DEV int base(int c) const { return Spec::cls_base[c]; }
    NBK_SPEC_DEV int groups(int c) const { return Spec::cls_groups[c]; }
};

// ---- folded tables ------------------------------------------------------------------------------------------------------------------
// The generated Spec classes every float32 table value of the robot that the sweep multiplies by (fc_pk, fc_tl; the
// classes: nbk_tables.hpp, fold_class).  In the folded sweep a term whose constant is FC_ZERO is not issued, a term whose constant
// is +-1 is an add, a subtract or a negation, and everything else is the unfolded sweep's fma chain in its order.  For finite
// operands an exact zero or +-1 folds to the unfolded value bit for bit up to the sign of a zero (fma(a, 0, x) = x,
// fma(a, 1, x) = a + x); a residue classed zero moves a centre by less than the slack charges.
//
// A wave takes the folded sweep only when every lane's sum of |q_k| (float32) is below FOLD_QMAX; any other wave (a NaN fails the
// compare) runs the unfolded sweep, whose fma(inf, 0, .) terms make the NaN the generic kernel has.  Below the bound nothing of
// the sweep overflows, so neither arm sees an inf or a NaN and the folds are exact.  The argument, with the ranges the generator
// checks before it classes anything (rotation-type table entries at most 2, lengths and slides at most 2^20): |sin|, |cos| <= 1,
// so an entry of L = M0 + s M2 - c M1 is at most 6 and a frame entry grows by at most 3 * 6 = 18 per joint, to 2 * 18^8 < 2^35
// after eight; a joint's own translation is at most 2^20 + 2^20 * 2^20 < 2^41 and a shape offset at most 2^20; a frame
// translation is at most 2^20 + 8 * 3 * 2^35 * 2^41 < 2^81 and a centre at most that + 3 * 2^35 * 2^20 -- every product and
// partial sum far below 2^127.
constexpr float FOLD_QMAX = 0x1p20f;
enum { FC_GEN = 0, FC_ZERO = 1, FC_ONE = 2, FC_NEG = 3 };

NBK_SPEC_DEV V2f fold_mul(V2f a, float k) { return a * splat2(k); }
NBK_SPEC_DEV V2f fold_mul(V2f a, V2f k) { return a * k; }
NBK_SPEC_DEV float fold_mul(float a, float k) { return a * k; }
NBK_SPEC_DEV V2f fold_fma(V2f a, float k, V2f acc) { return fma2(a, splat2(k), acc); }
NBK_SPEC_DEV V2f fold_fma(V2f a, V2f k, V2f acc) { return fma2(a, k, acc); }
NBK_SPEC_DEV float fold_fma(float a, float k, float acc) { return __builtin_fmaf(a, k, acc); }

// acc + a * k for a k of class CL; EMPTY: the chain has issued no term yet and acc holds nothing
template <int CL, bool EMPTY, class T, class K> NBK_SPEC_DEV T fold_term(T a, K k, T acc) {
    if constexpr (CL == FC_ZERO) return acc;
    else if constexpr (CL == FC_ONE) { if constexpr (EMPTY) return a; else return a + acc; }
    else if constexpr (CL == FC_NEG) { if constexpr (EMPTY) return -a; else return acc - a; }
    else { if constexpr (EMPTY) return fold_mul(a, k); else return fold_fma(a, k, acc); }
}
// the sweep's three-term chains: fma(a2, k2, fma(a1, k1, fma(a0, k0, init))) with HAS, fma(a2, k2, fma(a1, k1, a0 * k0)) without (init = 0)
template <int C0, int C1, int C2, bool HAS, class T, class K> NBK_SPEC_DEV T fold_dot3(T a0, T a1, T a2, K k0, K k1, K k2, T init) {
    constexpr bool e0 = !HAS, e1 = e0 && C0 == FC_ZERO, e2 = e1 && C1 == FC_ZERO;
    return fold_term<C2, e2>(a2, k2, fold_term<C1, e1>(a1, k1, fold_term<C0, e0>(a0, k0, init)));
}
// one entry of L = s M2 - c M1 (columns U and V hold no M0) from the classes of its M2 and M1 entries
template <int C2, int C1> NBK_SPEC_DEV float fold_l(float s, float c, float m2, float m1) {
    if constexpr (C2 == FC_ZERO && C1 == FC_ZERO) return 0.0f;
    else if constexpr (C2 == FC_ZERO) return -fold_term<C1, true>(c, m1, 0.0f);
    else if constexpr (C1 == FC_ZERO) return fold_term<C2, true>(s, m2, 0.0f);
    else return __builtin_fmaf(s, m2, -(c * m1));
}
// C::at(i): the class of float i of a joint's packed block, in the order m2p[6], m1p[6], mk[3], toff[3]
template <class C> struct FoldL {
    float x[3], y[3];                       // L[r][U], L[r][V]
    static constexpr int z(int i) { return C::at(i) == FC_ZERO && C::at(6 + i) == FC_ZERO ? FC_ZERO : FC_GEN; }       // i = 2 r + (0: U, 1: V)
    static constexpr int pz(int r) { return z(2 * r) == FC_ZERO && z(2 * r + 1) == FC_ZERO ? FC_ZERO : FC_GEN; }     // the pair of row r
    NBK_SPEC_DEV FoldL(const JPk& jp, float s, float c) {
        x[0] = fold_l<C::at(0), C::at(6)>(s, c, jp.m2p[0], jp.m1p[0]);  y[0] = fold_l<C::at(1), C::at(7)>(s, c, jp.m2p[1], jp.m1p[1]);
        x[1] = fold_l<C::at(2), C::at(8)>(s, c, jp.m2p[2], jp.m1p[2]);  y[1] = fold_l<C::at(3), C::at(9)>(s, c, jp.m2p[3], jp.m1p[3]);
        x[2] = fold_l<C::at(4), C::at(10)>(s, c, jp.m2p[4], jp.m1p[4]); y[2] = fold_l<C::at(5), C::at(11)>(s, c, jp.m2p[5], jp.m1p[5]);
    }
};
// joint_apply_axis_p with the joint's classes: the same chains in the same order, less the folded terms
template <int KZ, class C>
NBK_SPEC_DEV void joint_apply_axis_fold(const JPk& jp, const XfP& P, float s, float c, XfP& o) {
    constexpr int U = (KZ + 1) % 3, V = (KZ + 2) % 3;
    using Z = FoldL<C>;
    const Z L(jp, s, c);
    const V2f z2 = V2f{0.0f, 0.0f};
    const V2f cu = fold_dot3<Z::z(0), Z::z(2), Z::z(4), false>(P.Rc[0], P.Rc[1], P.Rc[2], L.x[0], L.x[1], L.x[2], z2);
    const V2f cv = fold_dot3<Z::z(1), Z::z(3), Z::z(5), false>(P.Rc[0], P.Rc[1], P.Rc[2], L.y[0], L.y[1], L.y[2], z2);
    const V2f ck = fold_dot3<C::at(12), C::at(13), C::at(14), false>(P.Rc[0], P.Rc[1], P.Rc[2], jp.mk[0], jp.mk[1], jp.mk[2], z2);
    const V2f r2 = fold_dot3<Z::pz(0), Z::pz(1), Z::pz(2), false>(splat2(P.R2[0]), splat2(P.R2[1]), splat2(P.R2[2]), V2f{L.x[0], L.y[0]},
                                                                  V2f{L.x[1], L.y[1]}, V2f{L.x[2], L.y[2]}, z2);
    const float r2k = fold_dot3<C::at(12), C::at(13), C::at(14), false>(P.R2[0], P.R2[1], P.R2[2], jp.mk[0], jp.mk[1], jp.mk[2], 0.0f);
    const V2f tc = fold_dot3<C::at(15), C::at(16), C::at(17), true>(P.Rc[0], P.Rc[1], P.Rc[2], jp.toff[0], jp.toff[1], jp.toff[2], P.tc);
    const float t2 = fold_dot3<C::at(15), C::at(16), C::at(17), true>(P.R2[0], P.R2[1], P.R2[2], jp.toff[0], jp.toff[1], jp.toff[2], P.t2);
    o.Rc[U] = cu; o.Rc[V] = cv; o.Rc[KZ] = ck;
    o.R2[U] = r2.x; o.R2[V] = r2.y; o.R2[KZ] = r2k;
    o.tc = tc; o.t2 = t2;
}
template <class Spec, int K> struct PkClass { static constexpr int at(int i) { return Spec::fc_pk[18 * K + i]; } };

// Spec (generated) provides:
//   S (robot shapes), SB (even register bucket >= S), NQ, J (<= 8), W (world shapes of the descriptor), NW (world shapes with a pair)
//   jkind[J], qcol[J]; sh_begin[J + 2] (shapes of frame k - 1 are [sh_begin[k], sh_begin[k + 1]))
//   f_pk, f_tl, f_base, f_wc, f_wobb, f_trans, f_slide, f_rot (= 0)         float offsets into f_tab
//   f_eps, f_reach, f_e2max                                                 the descriptor's slack constants
//   rr_any; rpair(a, b) (a < b), rr_p(a, b): pair index of robot-robot slot (a, b), -1 = none
//   wl[NW], wk[NW]: world shape and kind; wpair(i, a): pair index of (wl[i], a), -1 = none
//   wbox_aligned[NW]: 1 = a box of a descriptor that cannot move whose axes at f_wc are exactly the coordinate axes
//   fc_any, fc_pk[18 J], fc_tl[3 S]: the classes of the robot's table values for the folded sweep (fc_any = 0: none)
//   cls_base[4], cls_groups[4]
template <class Spec>
NBK_SPEC_DEV void broad_f32_spec(const double* __restrict__ q, long long B, const float* __restrict__ ftb, const float* __restrict__ tab,
                                 unsigned long long* __restrict__ mask_bits, unsigned char* __restrict__ mask_bytes,
                                 unsigned long long* __restrict__ q_count, unsigned long long* __restrict__ q_items, unsigned long long cap,
                                 unsigned char* ovf, const int* __restrict__ vp_cls) {
    constexpr int S = Spec::S, SB = Spec::SB, NQ = Spec::NQ, J = Spec::J, W = Spec::W;
    constexpr FTabOffsets FO = ftab_offsets(W);
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const long long base = (long long)blockIdx.x * WAVE;
    double* lds_raw = lds;
    constexpr int qrows = NQ > (SB + 2) / 2 ? NQ : (SB + 2) / 2;
    constexpr int qcap = qrows * (WAVE * 2);
    static_assert(qcap >= BQ_CAP && qcap >= S * WAVE, "the q slab must hold the general stage's queue and one unrolled block's items");
    unsigned* lds_queue = reinterpret_cast<unsigned*>(lds_raw);
    if (base >= B) return;
    const int rows_i = (int)((B - base) < WAVE ? (B - base) : WAVE);
    const bool active = lane < rows_i;
    // NQ <= 8: every lane loads its own row straight into registers, as k_fk<true> does (eight-byte loads at an 8 NQ-byte stride:
    // the wave's NQ instructions hit the same lines); no LDS pass and no barrier before the sweep.  A lane past the batch takes
    // row `base`, lane 0's: it is inactive, and its slack is lane 0's, so the wave's choice of stage is that of its real rows.
    // Longer rows go through the LDS slab.
    constexpr bool QREG = NBK_SPEC_QREG != 0 && NQ <= 8;
    double qd[QREG ? NQ : 1];
    if constexpr (QREG) {
        const double* row = q + (base + (active ? lane : 0)) * NQ;
#pragma unroll
        for (int j = 0; j < NQ; ++j) qd[j] = row[j];
    } else {
        stage_plain_rows(q, base, rows_i, NQ, lds_raw, lane);
        __syncthreads();
    }
    auto qat = [&](int j) NBK_SPEC_INLINE { if constexpr (QREG) return qd[j]; else return lds_raw[lane * NQ + j]; };
    int hit = 0;                // (an int: a bool captured by the lambdas below was kept in scratch, two bytes per lane)
#pragma unroll
    for (int j = 0; j < NQ; ++j) hit = hit || !(__builtin_fabs(qat(j)) <= 1.7976931348623157e308);
    // ---- chain sweep: every shape's centre in named registers ------------------------------------------------------------------
    float cxa[SB], cya[SB], cza[SB];
#pragma unroll
    for (int i = 0; i < SB; ++i) { cxa[i] = 0.0f; cya[i] = 0.0f; cza[i] = 0.0f; }
    float rmax = Spec::f_reach, qabs = 0.0f;
    float qv[J];
#pragma unroll
    for (int k = 0; k < J; ++k) { qv[k] = (float)qat(Spec::qcol[k]); qabs += __builtin_fabsf(qv[k]); }
    // FOLD = 1: the sweep with the robot's folded tables (above); FOLD = 0: the unfolded one, the generic kernel's operation for operation
    auto sweep = [&](auto FOLD) NBK_SPEC_INLINE {
        constexpr bool fold = decltype(FOLD)::value != 0;
        constexpr bool fold_joints = fold && (NBK_SPEC_FOLD_PARTS & 1) != 0, fold_shapes = fold && (NBK_SPEC_FOLD_PARTS & 2) != 0;
        XfP T;
        {
            const float* bp = ftb + Spec::f_base;
#pragma unroll
            for (int k = 0; k < 3; ++k) { T.Rc[k] = V2f{bp[k], bp[4 + k]}; T.R2[k] = bp[8 + k]; }
            T.tc = V2f{bp[3], bp[7]}; T.t2 = bp[11];
        }
        auto shapes = [&](auto K) NBK_SPEC_INLINE {                 // the shapes of frame K - 1 from the current frame T
            constexpr int k = decltype(K)::value;
            sfor<Spec::sh_begin[k], Spec::sh_begin[k + 1]>([&](auto SH) NBK_SPEC_INLINE {
                constexpr int sh = decltype(SH)::value;
                const float tl0 = ftb[Spec::f_tl + 3 * sh], tl1 = ftb[Spec::f_tl + 3 * sh + 1], tl2 = ftb[Spec::f_tl + 3 * sh + 2];
                V2f cp;
                float c2;
                if constexpr (fold_shapes) {
                    constexpr int c0 = Spec::fc_tl[3 * sh], c1 = Spec::fc_tl[3 * sh + 1], c2c = Spec::fc_tl[3 * sh + 2];
                    cp = fold_dot3<c0, c1, c2c, true>(T.Rc[0], T.Rc[1], T.Rc[2], tl0, tl1, tl2, T.tc);
                    c2 = fold_dot3<c0, c1, c2c, true>(T.R2[0], T.R2[1], T.R2[2], tl0, tl1, tl2, T.t2);
                } else {
                    cp = fma2(T.Rc[2], splat2(tl2), fma2(T.Rc[1], splat2(tl1), fma2(T.Rc[0], splat2(tl0), T.tc)));
                    c2 = __builtin_fmaf(T.R2[2], tl2, __builtin_fmaf(T.R2[1], tl1, __builtin_fmaf(T.R2[0], tl0, T.t2)));
                }
                cxa[sh] = cp.x; cya[sh] = cp.y; cza[sh] = c2;
                rmax = __builtin_fmaxf(rmax, __builtin_fmaxf(__builtin_fabsf(cp.x), __builtin_fmaxf(__builtin_fabsf(cp.y), __builtin_fabsf(c2))));
            });
        };
        shapes(IC<0>{});
        sfor<0, J>([&](auto K) NBK_SPEC_INLINE {
            constexpr int k = decltype(K)::value;
            constexpr int kind = Spec::jkind[k];
            float s = 0.0f, c = 0.0f;
            if constexpr (kind != JK_PRISMATIC) sincos_f(qv[k], s, c);
            if constexpr (kind <= 2) {
                const JPk jp = *reinterpret_cast<const JPk*>(ftb + Spec::f_pk + 20 * k);
                if constexpr (fold_joints) joint_apply_axis_fold<kind, PkClass<Spec, k>>(jp, T, s, c, T);
                else joint_apply_axis_p<kind>(jp, T, s, c, T);
            } else {
                joint_apply_gen_p(ftb + Spec::f_rot + 27 * k, ftb + Spec::f_trans + 3 * k, ftb + Spec::f_slide + 3 * k, T, qv[k], s, c, T);
            }
            shapes(IC<k + 1>{});
        });
    };
    if constexpr (NBK_SPEC_FOLD != 0 && (NBK_SPEC_FOLD_PARTS & 3) != 0 && Spec::fc_any != 0) {
        if (__builtin_amdgcn_ballot_w64(!(qabs < FOLD_QMAX)) == 0ull) sweep(IC<1>{});
        else sweep(IC<0>{});
    } else {
        sweep(IC<0>{});
    }
    const float e2 = 2.0f * rmax * __builtin_fmaf(2.4e-7f, qabs, Spec::f_eps);
    if constexpr (!QREG) __syncthreads();            // the q slab is dead from here on: its LDS region becomes the item queue
    int qn = 0;
    const SpecRoute<Spec> route{vp_cls};
    const float* wbx_all = tab + FO.wbx;
    if (__builtin_amdgcn_ballot_w64(!(e2 <= Spec::f_e2max)) == 0ull) {
        // ---- fast stage: world shapes -----------------------------------------------------------------------------------------
        // (A group both of whose slots k_prepare_f32 left at the "never" defaults -- out of static reach at this threshold -- is
        // computed all the same: a scalar branch around it took 16 VALU off the wave and added 54 SALU, for no time: DESIGN.md §6.)
        sfor<0, NBK_SPEC_WORLD ? Spec::NW : 0>([&](auto WI) NBK_SPEC_INLINE {
            constexpr int wi = decltype(WI)::value;
            constexpr int w = Spec::wl[wi];
            constexpr int wk = Spec::wk[wi];
            const float* wc = ftb + Spec::f_wc + 18 * w;
            if constexpr (wk == K_BOX || wk == K_HULL) {
                const float* wb = wbx_all + w * 96;
                const float* ob = ftb + Spec::f_wobb + 6 * w;
                int cwv[SB];
                int acc_c = 0, acc_h = 0;
                sfor<0, SB / 2>([&](auto I) NBK_SPEC_INLINE {
                    constexpr int i = decltype(I)::value;
                    cwv[2 * i] = 0; cwv[2 * i + 1] = 0;
                    if constexpr (Spec::wpair(wi, 2 * i) >= 0 || Spec::wpair(wi, 2 * i + 1) >= 0) {
                        const V2f dx = V2f{cxa[2 * i], cxa[2 * i + 1]} - splat2(wc[0]);
                        const V2f dy = V2f{cya[2 * i], cya[2 * i + 1]} - splat2(wc[1]);
                        const V2f dz = V2f{cza[2 * i], cza[2 * i + 1]} - splat2(wc[2]);
                        V2i cand, certh;
                        if constexpr (wk == K_BOX) box_slot2<NBK_SPEC_ALIGNED != 0 && Spec::wbox_aligned[wi] != 0>(dx, dy, dz, wc, wb + 12 * i, cand, certh);
                        else hull_slot2(dx, dy, dz, wc, ob, wb + 12 * i, cand, certh);
                        cwv[2 * i] = cand.x; cwv[2 * i + 1] = cand.y;
                        acc_c |= cand.x | cand.y;
                        acc_h |= certh.x | certh.y;
                    }
                });
                hit = hit || (acc_h < 0);
                const bool live = active && !hit;
                if (NBK_SPEC_ENQUEUE && __builtin_amdgcn_ballot_w64(acc_c < 0 && live) != 0ull) {
                    queue_room(S * WAVE, qcap, route, lds_queue, qn, base, q_count, q_items, cap, lane, ovf);
                    sfor<0, S>([&](auto A) NBK_SPEC_INLINE {
                        constexpr int a = decltype(A)::value;
                        if constexpr (Spec::wpair(wi, a) >= 0) enqueue_lanes(cwv[a] < 0 && live, (unsigned)Spec::wpair(wi, a), lds_queue, qn, lane);
                    });
                }
            } else {
                // planes and the other kinds: one compare per slot against the table's squared / height thresholds
                const Row16f wkey2r = *reinterpret_cast<const Row16f*>(tab + FO.wkey2 + w * 16);
                const Row16f wcertr = *reinterpret_cast<const Row16f*>(tab + FO.wcert + w * 16);
                const Row16f wkeyr = *reinterpret_cast<const Row16f*>(tab + FO.wkey + w * 16);
                const int* tab_wp = reinterpret_cast<const int*>(tab + FO.wp);
                bool c[SB];
                bool ch = false, anyc = false;
                sfor<0, S>([&](auto A) NBK_SPEC_INLINE {
                    constexpr int a = decltype(A)::value;
                    c[a] = false;
                    if constexpr (Spec::wpair(wi, a) >= 0) {
                        if constexpr (wk == K_PLANE) {
                            if (tab_wp[w * 16 + a] >= 0) plane_slot1(cxa[a] - wc[0], cya[a] - wc[1], cza[a] - wc[2], wc, wkey2r.v[a], wcertr.v[a], c[a], ch);
                        } else {
                            if (wkeyr.v[a] >= 0.0f) sphere_slot1(cxa[a] - wc[0], cya[a] - wc[1], cza[a] - wc[2], wkey2r.v[a], wcertr.v[a], c[a], ch);
                        }
                        anyc = anyc || c[a];
                    }
                });
                hit = hit || ch;
                const bool live = active && !hit;
                if (NBK_SPEC_ENQUEUE && __builtin_amdgcn_ballot_w64(anyc && live) != 0ull) {
                    queue_room(S * WAVE, qcap, route, lds_queue, qn, base, q_count, q_items, cap, lane, ovf);
                    sfor<0, S>([&](auto A) NBK_SPEC_INLINE {
                        constexpr int a = decltype(A)::value;
                        if constexpr (Spec::wpair(wi, a) >= 0) enqueue_lanes(c[a] && live, (unsigned)Spec::wpair(wi, a), lds_queue, qn, lane);
                    });
                }
            }
        });
        // ---- fast stage: robot-robot rows, only the groups (2i, 2i + 1) that hold a pair of row a ------------------------------
        if constexpr (Spec::rr_any && NBK_SPEC_RR != 0) {
            sfor<0, S - 1>([&](auto A) NBK_SPEC_INLINE {
                constexpr int a = decltype(A)::value;
                if constexpr (Spec::row_slots(a) > 0) {
                    const Row16f nk = *reinterpret_cast<const Row16f*>(tab + FO.rneg + a * 16);
                    const V2f ax2 = V2f{cxa[a], cxa[a]}, ay2 = V2f{cya[a], cya[a]}, az2 = V2f{cza[a], cza[a]};
                    V2f ev[SB / 2];
                    int acc_e = 0;
                    sfor<(a + 1) / 2, SB / 2>([&](auto I) NBK_SPEC_INLINE {
                        constexpr int i = decltype(I)::value;
                        if constexpr (Spec::rr_group(a, i)) {
                            ev[i] = slot_e2(ax2 - V2f{cxa[2 * i], cxa[2 * i + 1]}, ay2 - V2f{cya[2 * i], cya[2 * i + 1]},
                                            az2 - V2f{cza[2 * i], cza[2 * i + 1]}, V2f{nk.v[2 * i], nk.v[2 * i + 1]});
                            const V2i ei = __builtin_bit_cast(V2i, ev[i]);
                            acc_e |= ei.x | ei.y;
                        }
                    });
                    if (__builtin_amdgcn_ballot_w64(acc_e < 0 && active && !hit) != 0ull) {
                        const Row16f nd = *reinterpret_cast<const Row16f*>(tab + FO.rnd + a * 16);
                        int acc_f = 0;
                        sfor<(a + 1) / 2, SB / 2>([&](auto I) NBK_SPEC_INLINE {
                            constexpr int i = decltype(I)::value;
                            if constexpr (Spec::rr_group(a, i)) {
                                const V2i fi = __builtin_bit_cast(V2i, ev[i] + V2f{nd.v[2 * i], nd.v[2 * i + 1]});
                                acc_f |= fi.x | fi.y;
                            }
                        });
                        hit = hit || (acc_f < 0);
                        const bool live = active && !hit;
                        if (NBK_SPEC_ENQUEUE) queue_room(Spec::row_slots(a) * WAVE, qcap, route, lds_queue, qn, base, q_count, q_items, cap, lane, ovf);
                        sfor<NBK_SPEC_ENQUEUE ? a + 1 : S, S>([&](auto Bb) NBK_SPEC_INLINE {
                            constexpr int b = decltype(Bb)::value;
                            if constexpr (Spec::rr_p(a, b) >= 0) {
                                const V2i ei = __builtin_bit_cast(V2i, ev[b / 2]);
                                enqueue_lanes(((b % 2) ? ei.y : ei.x) < 0 && live, (unsigned)Spec::rr_p(a, b), lds_queue, qn, lane);
                            }
                        });
                    }
                }
            });
        }
    } else {
        // ---- general stage (some lane's slack exceeds the static bound: prismatic travel, huge joint values): the generic
        // kernel's, over the descriptor's real slots ----------------------------------------------------------------------------
        const bool cert_ok = e2 <= Spec::f_e2max;
        bool certh = false;
        const float* tab_wkey = tab + FO.wkey; const float* tab_wtc = tab + FO.wtc; const float* tab_wcert = tab + FO.wcert;
        const float* tab_wcin = tab + FO.wcin; const float* tab_rho = tab + FO.rho;
        const int* tab_wp = reinterpret_cast<const int*>(tab + FO.wp);
        const int* tab_rp = reinterpret_cast<const int*>(tab + FO.rp);
        const float* tab_rkey = tab + FO.rkey; const float* tab_rcert = tab + FO.rcert;
        sfor<0, Spec::NW>([&](auto WI) NBK_SPEC_INLINE {
            constexpr int wi = decltype(WI)::value;
            constexpr int w = Spec::wl[wi];
            constexpr int wk = Spec::wk[wi];
            const float* wc = ftb + Spec::f_wc + 18 * w;
            unsigned long long bits = 0ull;
            sfor<0, S>([&](auto A) NBK_SPEC_INLINE {
                constexpr int a = decltype(A)::value;
                if constexpr (Spec::wpair(wi, a) >= 0) {
                    const float dx = cxa[a] - wc[0], dy = cya[a] - wc[1], dz = cza[a] - wc[2];
                    if constexpr (wk == K_PLANE) {
                        if (tab_wp[w * 16 + a] >= 0)
                            bits |= plane_slot_gen(dx, dy, dz, wc, tab_wkey[w * 16 + a], tab_rho[a], e2, tab_wcert[w * 16 + a], certh) ? (1ull << a) : 0ull;
                    } else if constexpr (wk == K_BOX) {
                        if (tab_wkey[w * 16 + a] >= 0.0f)
                            bits |= box_slot_gen(dx, dy, dz, wc, tab_wkey[w * 16 + a], tab_wtc[w * 16 + a], tab_rho[a], e2, tab_wcin[w * 16 + a],
                                                 certh, hit) ? (1ull << a) : 0ull;
                    } else {
                        if (tab_wkey[w * 16 + a] >= 0.0f)
                            bits |= other_slot_gen(dx, dy, dz, wc, ftb + Spec::f_wobb + 6 * w, wk == K_HULL, tab_wkey[w * 16 + a], tab_wtc[w * 16 + a],
                                                   tab_rho[a], e2, tab_wcert[w * 16 + a], certh) ? (1ull << a) : 0ull;
                    }
                }
            });
            hit = hit || (cert_ok && certh);
            if (!active || hit) bits = 0ull;
            drain_bits(bits, PairTab{tab_wp + w * 16}, route, lds_queue, qn, base, q_count, q_items, cap, lane, ovf);
        });
        if constexpr (Spec::rr_any) {
            sfor<0, S - 1>([&](auto A) NBK_SPEC_INLINE {
                constexpr int a = decltype(A)::value;
                unsigned long long bits = 0ull;
                sfor<a + 1, S>([&](auto Bb) NBK_SPEC_INLINE {
                    constexpr int b = decltype(Bb)::value;
                    if constexpr (Spec::rr_p(a, b) >= 0) {
                        bits |= robot_slot_gen(cxa[a] - cxa[b], cya[a] - cya[b], cza[a] - cza[b], tab_rkey[a * 16 + b], e2, tab_rcert[a * 16 + b], certh)
                                    ? (1ull << b) : 0ull;
                    }
                });
                hit = hit || (cert_ok && certh);
                if (!active || hit) bits = 0ull;
                drain_bits(bits, PairTab{tab_rp + a * 16}, route, lds_queue, qn, base, q_count, q_items, cap, lane, ovf);
            });
        }
    }
    if (qn > 0) flush_items_r(route, lds_queue, qn, base, q_count, q_items, cap, lane, ovf);
    write_mask(hit != 0, active, base, lane, mask_bits, mask_bytes);
}

}  // namespace nbk_spec

#ifndef NBK_SPEC_WAVES
#define NBK_SPEC_WAVES 5
#endif
// the generated text defines `struct Spec` before this point
extern "C" __global__ __launch_bounds__(64, NBK_SPEC_WAVES) void k_broad_f32_spec(
        const double* __restrict__ q, long long B, const float* __restrict__ ftb, const float* __restrict__ tab,
        unsigned long long* __restrict__ mask_bits, unsigned char* __restrict__ mask_bytes, unsigned long long* __restrict__ q_count,
        unsigned long long* __restrict__ q_items, unsigned long long cap, unsigned char* ovf, const int* __restrict__ vp_cls) {
    nbk_spec::broad_f32_spec<Spec>(q, B, ftb, tab, mask_bits, mask_bytes, q_count, q_items, cap, ovf, vp_cls);
}
