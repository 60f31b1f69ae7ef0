// nbk_lds.hpp -- the dynamic LDS of every kernel family, each layout once ("The LDS layouts"): the kernel carves its
// regions with the struct, the host takes the launch's byte count (bytes()) and its refusal (!fits()) from the same struct, and creation
// (check_limits, nbk_tables.hpp) takes its verdicts from them.  Host and device share this file, so every function carries NBK_HD; apart
// from that: no HIP include, type or call, no global -- g++ -std=c++17 compiles it alone (tests/lds_check.cpp sweeps it under the host
// sanitizers and holds the properties the kernels rely on).
#pragma once
#include <stddef.h>

#ifdef __HIPCC__
#define NBK_HD __host__ __device__
#else
#define NBK_HD
#endif

namespace nbk {

// WAVE and BQ_CAP belong to nbk_bf32_common.hpp, which also travels to hipRTC as text: this file works with its own copies, which
// nbk.hip holds against them with a static_assert.  NBK_ZFIRST and NBK_ZSLOTS are per-build switches of k_broad_f32 (nbk.hip): a
// variant build that sets them on the command line sets them here too.  The other constants live here and nbk.hip uses them from here.
constexpr int LDS_WAVE = 64, LDS_BQ_CAP = 512;
#if defined(NBK_ZFIRST) && defined(NBK_ZSLOTS)
constexpr int LDS_ZFIRST = NBK_ZFIRST, LDS_ZSLOTS = NBK_ZSLOTS;
#else
constexpr int LDS_ZFIRST = 4, LDS_ZSLOTS = 2;
#endif
constexpr size_t LDS_MAX = 160 * 1024;     // LDS per workgroup on gfx950 (MI355X_MICROARCH.md)
constexpr int QUEUE_CAP = 512;             // wave_collides: (lane, pair) items; flushed whenever fewer than 64 slots are left
constexpr int CQ_CAP = 512;                // k_closest: (lane, pair) items of its branch-and-bound queue
constexpr int EPAQ_CAP = 128;              // k_distances: (lane, pair) items waiting for their EPA pass, per wave
constexpr int EPAQ_DOUBLES = EPAQ_CAP + EPAQ_CAP / 2;        // one wave's EPA queue: depths [EPAQ_CAP] double, items [EPAQ_CAP] unsigned
constexpr int JAC_ROWS = 32;               // k_jacobian_reg: configurations whose rows go through LDS at a time
constexpr int NARROW_T = 64;               // k_narrow*: threads (= items of a chunk) per workgroup
constexpr int HULL_LDS_MAX = 16 * 1024;    // k_narrow*: the scene's hull vertices live in LDS when they fit this (the per-lane vertex loop of
                                           // the hull support is 3 loads per vertex at lane-varying addresses: LDS serves those several
                                           // times faster than the vector memory path)

// Every layout lists its regions in the order they lie in LDS.  Its members are the regions' lengths, `<region>_len`, in elements of the
// region's own type (double unless the comment says otherwise); `<region>(base)` is the region's pointer, of its own element type, in
// the dynamic LDS that starts at `base`: the previous region's pointer plus the previous region's length, re-typed inside the accessor
// where the type changes -- the chain of pointer additions the kernels always had, written once.  Order and types stand nowhere else:
// every kernel of nbk.hip takes its region pointers from the accessors of a named `const ...Lds L(...)`, and tests/lds_check.cpp proves
// its properties over what the same accessors return for a host buffer (begin = pointer - base, element size = sizeof(*pointer)).
// bytes() is what the launch asks for, a sum over the lengths, fits() whether a workgroup can have it.  A constructor computes the
// lengths and nothing else (the kernels run it); what only the byte count needs is kept as given and worked out in bytes().  An argument
// that only sizes the last region comes last and has a default: the kernel, which needs no end, leaves it out.  Out of scope: the kernel
// compiled per robot (nbk_bf32_spec.hpp) travels to hipRTC as text and carves its slab for itself.
#define NBK_LDS_TOTAL(expr) NBK_HD size_t bytes() const { return (expr); } NBK_HD bool fits() const { return bytes() <= LDS_MAX; }

// ---- kinematics ---------------------------------------------------------------------------------------------------------------------
// k_fk: the raw q slab [64][n_q], later the transposed poses [64][17]
struct FkLds {
    int n_q;
    NBK_HD explicit FkLds(int n_q_) : n_q(n_q_) {}
    NBK_HD int rows() const { return n_q > 17 ? n_q : 17; }      // rows of 64 doubles
    NBK_LDS_TOTAL(sizeof(double) * LDS_WAVE * (size_t)rows())
};
// k_fk_frames: q rows [n_q][64] | saved frames [12 slots][64] | transpose [64][17], which first holds the raw q slab [64][n_q]
struct FkFramesLds {
    int q_len, fr_len, n_q;
    NBK_HD FkFramesLds(int n_q_, int frame_slots) : q_len(LDS_WAVE * n_q_), fr_len(LDS_WAVE * 12 * frame_slots), n_q(n_q_) {}
    NBK_HD double* q(double* base) const { return base; }
    NBK_HD double* fr(double* base) const { return q(base) + q_len; }
    NBK_HD double* t(double* base) const { return fr(base) + fr_len; }
    NBK_HD size_t t_len() const { return (size_t)LDS_WAVE * FkLds(n_q).rows(); }
    NBK_LDS_TOTAL(sizeof(double) * ((size_t)q_len + (size_t)fr_len + t_len()))
};
// k_jacobian: raw q slab [64][n_q] | output rows [64][stride], stride = 6 n_q | 1 (odd: conflict-free)
struct JacobianLds {
    int q_len, n_q;
    NBK_HD explicit JacobianLds(int n_q_) : q_len(LDS_WAVE * n_q_), n_q(n_q_) {}
    NBK_HD int stride() const { return (6 * n_q) | 1; }
    NBK_HD double* q(double* base) const { return base; }
    NBK_HD double* o(double* base) const { return q(base) + q_len; }
    NBK_LDS_TOTAL(sizeof(double) * ((size_t)q_len + LDS_WAVE * (size_t)(6 * n_q + 1)))
};
// k_jacobian_reg (paths of up to 8 joints): raw q slab [64][n_q]; the output rows [JAC_ROWS][stride] reuse it from 0 once q is read
struct JacobianRegLds {
    int n_q;
    NBK_HD explicit JacobianRegLds(int n_q_) : n_q(n_q_) {}
    NBK_HD int stride() const { return (6 * n_q) | 1; }
    NBK_HD size_t q_len() const { return (size_t)LDS_WAVE * n_q; }
    NBK_HD size_t o_len() const { return (size_t)JAC_ROWS * stride(); }
    NBK_HD double* q(double* base) const { return base; }   NBK_HD double* o(double* base) const { return q(base); }
    NBK_LDS_TOTAL(sizeof(double) * (q_len() > o_len() ? q_len() : o_len()))
};
// k_ik: q rows [n_q][64] | Jacobian [6 n_q][64] | joint axes and origins [6 path_len][64] (one joint at least)
struct IkLds {
    int q_len, J_len, path_len;
    NBK_HD explicit IkLds(int n_q, int path_len_ = 1) : q_len(LDS_WAVE * n_q), J_len(LDS_WAVE * 6 * n_q), path_len(path_len_) {}
    NBK_HD double* q(double* base) const { return base; }
    NBK_HD double* J(double* base) const { return q(base) + q_len; }
    NBK_HD double* jz(double* base) const { return J(base) + J_len; }
    NBK_HD size_t jz_len() const { return (size_t)LDS_WAVE * 6 * (size_t)(path_len > 0 ? path_len : 1); }
    NBK_LDS_TOTAL(sizeof(double) * ((size_t)q_len + (size_t)J_len + jz_len()))
};
// k_pair_items: q rows [64][n_q] (room for one row at least) | with gradient rows: joint axes and origins [6 n_joints][64]
struct PairItemsLds {
    int q_len, n_q, jz_joints;             // jz_joints: n_joints, 0 without gradient rows
    NBK_HD explicit PairItemsLds(int n_q_, int jz_joints_ = 0) : q_len(LDS_WAVE * n_q_), n_q(n_q_), jz_joints(jz_joints_) {}
    NBK_HD double* q(double* base) const { return base; }
    NBK_HD double* jz(double* base) const { return q(base) + q_len; }
    NBK_HD size_t jz_len() const { return (size_t)LDS_WAVE * 6 * (size_t)jz_joints; }
    NBK_LDS_TOTAL(sizeof(double) * ((size_t)LDS_WAVE * (n_q > 0 ? n_q : 1) + jz_len()))
};
// a q slab [64][n_q] and nothing else: the three cloud kernels; k_spline_ca (one row at least)
struct QSlabLds {
    int rows;
    NBK_HD explicit QSlabLds(int n_q, int min_rows = 0) : rows(n_q > min_rows ? n_q : min_rows) {}
    NBK_LDS_TOTAL(sizeof(double) * LDS_WAVE * (size_t)rows)
};
// k_cloud_self_filter: one record per selected robot shape, [n_sel][REC_LEN]: the shape's core at q0 as the kernel's Core struct
// (CORE_LEN doubles: nbk_cloud.hpp holds sizeof(Core) against it) | tc | the squared bounding-sphere sum (-1: the sum is not positive).
// A model whose selected shapes do not fit is refused by the entry (room for one record at least)
struct SelfFilterLds {
    static constexpr int CORE_LEN = 19, REC_LEN = CORE_LEN + 2, TC_AT = CORE_LEN, RS2_AT = CORE_LEN + 1;
    int rec_len;
    NBK_HD explicit SelfFilterLds(int n_sel) : rec_len(REC_LEN * (n_sel > 0 ? n_sel : 1)) {}
    NBK_HD double* rec(double* base) const { return base; }
    NBK_LDS_TOTAL(sizeof(double) * (size_t)rec_len)
};
// k_render_depth: one record per selected robot shape, [n_sel][REC_LEN]: the shape's core at the frame's q (CORE_LEN doubles, as above) |
// the widened radius of its bounding ball; then, for each of the four waves (8x8 pixel tiles) of the workgroup, the tile's candidate
// list over the n_list shapes drawn (the selected robot shapes, then the world's): own [4][n_list] u64, the lanes whose ray meets
// the candidate's ball | idx [4][n_list] int, the candidate's place in the drawn order.  World cores stay in global memory.
struct RenderLds {
    static constexpr int CORE_LEN = SelfFilterLds::CORE_LEN, REC_LEN = CORE_LEN + 1, RB_AT = CORE_LEN, WAVES = 4;
    static constexpr int LIST_BYTES = WAVES * 12;      // what one more drawn shape costs beyond its record
    int rec_len, own_len, idx_len;                     // own: u64, idx: int
    NBK_HD RenderLds(int n_sel, int n_list) : rec_len(REC_LEN * (n_sel > 0 ? n_sel : 1)), own_len(WAVES * n_list), idx_len(WAVES * n_list) {}
    NBK_HD double* rec(double* base) const { return base; }
    NBK_HD unsigned long long* own(double* base) const { return reinterpret_cast<unsigned long long*>(rec(base) + rec_len); }
    NBK_HD int* idx(double* base) const { return reinterpret_cast<int*>(own(base) + own_len); }
    NBK_LDS_TOTAL(sizeof(double) * (size_t)rec_len + sizeof(unsigned long long) * (size_t)own_len + sizeof(int) * (size_t)idx_len)
};
// k_narrow*: q rows [NARROW_T][n_q] | the scene's hull vertices [hull_blob_n] when they fit HULL_LDS_MAX
struct NarrowLds {
    int q_len, hull_blob_n;
    NBK_HD NarrowLds(int n_q, int hull_blob_n_) : q_len(NARROW_T * n_q), hull_blob_n(hull_blob_n_) {}
    NBK_HD bool hull_staged() const { return hull_blob_n > 0 && hull_blob_n <= HULL_LDS_MAX / 8; }      // else the cores keep reading global memory
    NBK_HD double* q(double* base) const { return base; }
    NBK_HD double* hull(double* base) const { return q(base) + q_len; }
    NBK_HD size_t hull_len() const { return hull_staged() ? (size_t)hull_blob_n : 0; }
    NBK_LDS_TOTAL(sizeof(double) * ((size_t)q_len + hull_len()))
};

// ---- the parked robot of 64 configurations -------------------------------------------------------------------------------------------
// q rows [n_q][64] | shape rows [shape_rows][64] | saved frames [12 slots][64] | a tail (the three layouts below).  The raw q slab
// [64][n_q] is staged in the shape area, free until the sweep starts: shape_rows >= n_q (nbk_model_create sees to it).
struct ParkedLds {
    int q_len, s_len, fr_len;
    NBK_HD ParkedLds(int n_q, int shape_rows, int frame_slots) : q_len(LDS_WAVE * n_q), s_len(LDS_WAVE * shape_rows), fr_len(LDS_WAVE * 12 * frame_slots) {}
    NBK_HD double* q(double* base) const { return base; }
    NBK_HD double* s(double* base) const { return q(base) + q_len; }
    NBK_HD double* fr(double* base) const { return s(base) + s_len; }
    NBK_HD double* tail(double* base) const { return fr(base) + fr_len; }
    NBK_HD size_t parked_bytes() const { return sizeof(double) * ((size_t)q_len + (size_t)s_len + (size_t)fr_len); }      // what lies before the tail
};
// tail of k_validity, k_validity_redo, k_edges and k_distances<0>: queue [QUEUE_CAP] unsigned | hit flags [64] unsigned.
// k_distances<0> keeps its one EPA queue (EPAQ_DOUBLES doubles) in it
struct ValidityLds : ParkedLds {
    static constexpr int QUEUE_LEN = QUEUE_CAP, HIT_LEN = LDS_WAVE;      // unsigned
    static constexpr int TAIL_BYTES = QUEUE_LEN * 4 + HIT_LEN * 4;
    NBK_HD ValidityLds(int n_q, int shape_rows, int frame_slots) : ParkedLds(n_q, shape_rows, frame_slots) {}
    NBK_HD unsigned* queue(double* base) const { return reinterpret_cast<unsigned*>(tail(base)); }
    NBK_HD unsigned* hit(double* base) const { return queue(base) + QUEUE_LEN; }
    NBK_LDS_TOTAL(parked_bytes() + TAIL_BYTES)
};
// tail of k_distances<MODE>: for MODE 3 the joint axes and origins [6 n_joints][64], then one EPA queue per wave (MODE 0: one wave,
// else two), each depths [EPAQ_CAP] double | items [EPAQ_CAP] unsigned.  The first wave's queue is paid for by the validity tail, which
// the byte count keeps; every further wave adds its own
struct DistancesLds : ParkedLds {
    int jz_len, mode;
    NBK_HD DistancesLds(int n_q, int shape_rows, int frame_slots, int n_joints, int mode_)
        : ParkedLds(n_q, shape_rows, frame_slots), jz_len(mode_ == 3 ? LDS_WAVE * 6 * n_joints : 0), mode(mode_) {}
    NBK_HD int nwave() const { return mode == 0 ? 1 : 2; }
    NBK_HD double* jz(double* base) const { return tail(base); }
    NBK_HD double* epaq_depth(double* base, int wave) const { return jz(base) + jz_len + wave * EPAQ_DOUBLES; }
    NBK_HD unsigned* epaq_item(double* base, int wave) const { return reinterpret_cast<unsigned*>(epaq_depth(base, wave) + EPAQ_CAP); }
    NBK_LDS_TOTAL(parked_bytes() + sizeof(double) * (size_t)jz_len + ValidityLds::TAIL_BYTES + sizeof(double) * (size_t)(nwave() - 1) * EPAQ_DOUBLES)
};
// tail of k_closest: results [CQ_CAP] double | best [64] u64 | argmin [64] unsigned | queue [CQ_CAP] unsigned | EPA list [CQ_CAP] u16
struct ClosestLds : ParkedLds {
    static constexpr int RES_LEN = CQ_CAP, BEST_LEN = LDS_WAVE, ARG_LEN = LDS_WAVE, QUEUE_LEN = CQ_CAP, ELIST_LEN = CQ_CAP;
    NBK_HD ClosestLds(int n_q, int shape_rows, int frame_slots) : ParkedLds(n_q, shape_rows, frame_slots) {}
    NBK_HD double* res(double* base) const { return tail(base); }
    NBK_HD unsigned long long* best(double* base) const { return reinterpret_cast<unsigned long long*>(res(base) + RES_LEN); }
    NBK_HD unsigned* arg(double* base) const { return reinterpret_cast<unsigned*>(best(base) + BEST_LEN); }
    NBK_HD unsigned* queue(double* base) const { return arg(base) + ARG_LEN; }
    NBK_HD unsigned short* elist(double* base) const { return reinterpret_cast<unsigned short*>(queue(base) + QUEUE_LEN); }
    NBK_LDS_TOTAL(parked_bytes() + sizeof(double) * RES_LEN + sizeof(unsigned long long) * BEST_LEN + sizeof(unsigned) * (ARG_LEN + QUEUE_LEN) + sizeof(unsigned short) * ELIST_LEN)
};

// ---- the broadphases -------------------------------------------------------------------------------------------------------------------
// All of them stage the raw q slab [64][n_q] at 0 and, once the sweep is over, reuse it as the wave's item queue (unsigned words):
// the slab has a floor of rows so that it holds the queue.
// k_broad, k_broad_reg: LDS_BQ_CAP items
NBK_HD constexpr int broad_qrows(int n_q) { return (LDS_WAVE * n_q * 8 >= LDS_BQ_CAP * 4) ? n_q : (LDS_BQ_CAP * 4 + LDS_WAVE * 8 - 1) / (LDS_WAVE * 8); }
// k_broad_f32<S, WH> and the kernel compiled per robot: LDS_BQ_CAP items and the S * 64 items of one unrolled block; S centre z rows of
// floats travel through it as well
NBK_HD constexpr int f32_qrows(int n_q, int S) { return n_q > (S + 2) / 2 ? n_q : (S + 2) / 2; }
NBK_HD constexpr int broad_bucket(int S) { return S <= 8 ? 8 : (S <= 12 ? 12 : 16); }      // template size of the register broadphases

// k_broad: q slab / queue | saved frames [12 slots][64] | centres [3 S][64] | pair constants [P][4] | world cores [W][18]
struct BroadLds {
    int qrows, slab_len, fr_len, c_len, pc_len, w_len;
    NBK_HD BroadLds(int n_q, int frame_slots, int n_rshapes, int n_pairs, int n_wshapes = 0)
        : qrows(broad_qrows(n_q)), slab_len(LDS_WAVE * qrows), fr_len(LDS_WAVE * 12 * frame_slots), c_len(LDS_WAVE * 3 * n_rshapes), pc_len(4 * n_pairs), w_len(18 * n_wshapes) {}
    NBK_HD int qcap() const { return qrows * (LDS_WAVE * 2); }      // queue entries the slab holds
    NBK_HD double* slab(double* base) const { return base; }   NBK_HD unsigned* queue(double* base) const { return reinterpret_cast<unsigned*>(slab(base)); }
    NBK_HD double* fr(double* base) const { return slab(base) + slab_len; }
    NBK_HD double* c(double* base) const { return fr(base) + fr_len; }
    NBK_HD double* pc(double* base) const { return c(base) + c_len; }
    NBK_HD double* w(double* base) const { return pc(base) + pc_len; }
    NBK_LDS_TOTAL(sizeof(double) * ((size_t)slab_len + (size_t)fr_len + (size_t)c_len + (size_t)pc_len + (size_t)w_len))
};
// k_broad_reg<S>: q slab / queue | saved frames | keys [S*S] | world keys [W*S] | world tc [W*S] | pair index [S*S] int | [W*S] int.
// The launch asks for 16 bytes more than the last region ends at
struct BroadRegLds {
    int qrows, slab_len, fr_len, rkey_len, wkey_len, wtc_len, rp_len, wp_len;      // rp, wp: int
    NBK_HD BroadRegLds(int n_q, int frame_slots, int S, int W)
        : qrows(broad_qrows(n_q)), slab_len(LDS_WAVE * qrows), fr_len(LDS_WAVE * 12 * frame_slots), rkey_len(S * S), wkey_len(W * S), wtc_len(W * S), rp_len(S * S), wp_len(W * S) {}
    NBK_HD int qcap() const { return qrows * (LDS_WAVE * 2); }
    NBK_HD double* slab(double* base) const { return base; }   NBK_HD unsigned* queue(double* base) const { return reinterpret_cast<unsigned*>(slab(base)); }
    NBK_HD double* fr(double* base) const { return slab(base) + slab_len; }
    NBK_HD double* rkey(double* base) const { return fr(base) + fr_len; }
    NBK_HD double* wkey(double* base) const { return rkey(base) + rkey_len; }
    NBK_HD double* wtc(double* base) const { return wkey(base) + wkey_len; }
    NBK_HD int* rp(double* base) const { return reinterpret_cast<int*>(wtc(base) + wtc_len); }
    NBK_HD int* wp(double* base) const { return rp(base) + rp_len; }
    NBK_LDS_TOTAL(sizeof(double) * ((size_t)slab_len + (size_t)fr_len + (size_t)rkey_len + (size_t)wkey_len + (size_t)wtc_len) + sizeof(int) * ((size_t)rp_len + (size_t)wp_len) + 16)
};
// k_broad_f32<S, WH>: q slab / queue / centre z rows | saved frames [12 slots][64] float | Z_PAD floats | z rows [NBK_ZSLOTS][64] float:
// the z of slots NBK_ZFIRST .., which the kernel indexes by slot (its pointer starts NBK_ZFIRST rows before them).  The kernel compiled
// per robot (nbk_bf32_spec.hpp carves for itself) has the slab alone
struct BroadF32Lds {
    static constexpr int Z_PAD = 4;        // floats: 16 bytes
    static constexpr size_t TAIL_BYTES = sizeof(float) * (Z_PAD + LDS_WAVE * LDS_ZSLOTS);      // what follows the saved frames
    int qrows, slab_len, fr_len;           // fr: float
    NBK_HD BroadF32Lds(int n_q, int frame_slots, int S) : qrows(f32_qrows(n_q, S)), slab_len(LDS_WAVE * qrows), fr_len(LDS_WAVE * 12 * frame_slots) {}
    NBK_HD int qcap() const { return qrows * (LDS_WAVE * 2); }      // queue entries the slab holds
    NBK_HD size_t slab_bytes() const { return sizeof(double) * (size_t)slab_len; }
    NBK_HD double* slab(double* base) const { return base; }   NBK_HD unsigned* queue(double* base) const { return reinterpret_cast<unsigned*>(slab(base)); }
    NBK_HD float* czrows(double* base) const { return reinterpret_cast<float*>(slab(base)); }      // the centre z rows
    NBK_HD float* fr(double* base) const { return reinterpret_cast<float*>(slab(base) + slab_len); }
    NBK_HD float* zp(double* base) const { return fr(base) + fr_len + Z_PAD - LDS_ZFIRST * LDS_WAVE; }      // indexed by slot: row LDS_ZFIRST is the first stored
    NBK_LDS_TOTAL(slab_bytes() + sizeof(float) * (size_t)fr_len + TAIL_BYTES)
};

// ---- creation (check_limits) ----------------------------------------------------------------------------------------------------------
// Creation is stricter than the launch in two places.  Both verdicts are kept as they were: the launch layout's bytes, with the q slab
// taken as n_q rows (creation knows no floor), plus a named constant.
// lds_broad_ok counts the item queue on top of the q slab, though the queue reuses the slab
constexpr size_t BROAD_QUEUE_COUNTED_TWICE = (size_t)LDS_BQ_CAP * 4;
NBK_HD inline bool lds_broad_ok(int n_q, int frame_slots, int n_rshapes, int n_pairs, int n_wshapes) {
    const BroadLds L(n_q, frame_slots, n_rshapes, n_pairs, n_wshapes);
    return L.bytes() - sizeof(double) * LDS_WAVE * (size_t)(L.qrows - n_q) + BROAD_QUEUE_COUNTED_TWICE <= LDS_MAX;
}
// robots of up to 16 shapes must fit k_broad_f32<S>: a flat 4096 bytes stand for what follows the saved frames (BroadF32Lds::TAIL_BYTES)
constexpr size_t BROAD_F32_FLAT_TAIL = 4096;
NBK_HD inline bool broad_f32_ok(int n_q, int frame_slots, int n_rshapes) {
    const BroadF32Lds L(n_q, frame_slots, broad_bucket(n_rshapes));
    return L.bytes() - sizeof(double) * LDS_WAVE * (size_t)(L.qrows - n_q) - BroadF32Lds::TAIL_BYTES + BROAD_F32_FLAT_TAIL <= LDS_MAX;
}

}  // namespace nbk
