// nbk_plan.hpp -- host only: the arithmetic of the validity launch path of nbk.hip ("The launch plan"): WsLayout, the
// parts of a validity workspace; TilePlan, how a call is cut into tiles and the bytes it needs; TableCache, when a stream's tables and
// counter sets may be reused; the capacity and scratch rules of the edge entry, the spline plan, and the scratch layouts of the edge,
// cloud-edge and spline entries with their typed views.  No kernel, no HIP type or call, no global: g++ -std=c++17 compiles this file
// alone (tests/plan_check.cpp sweeps it under the host sanitizers).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace nbk {

// WAVE, CNT_STRIDE (nbk_bf32_common.hpp) and NSUB (nbk.hip) are the includer's, held against these copies by a static_assert there;
// a program that includes this file alone defines NBK_PLAN_STANDALONE.
constexpr int PLAN_WAVE = 64, PLAN_CNT_STRIDE = 16, PLAN_NSUB = 256;
#ifdef NBK_PLAN_STANDALONE
constexpr int WAVE = PLAN_WAVE, CNT_STRIDE = PLAN_CNT_STRIDE, NSUB = PLAN_NSUB;
#endif

// what sizing reads from a descriptor (filled once, by model_create) and from the switches (Options in nbk.hip derives from it)
struct PlanModel {
    int n_q, n_pairs, n_rshapes, n_wshapes, frame_slots;
    int cls_count[4];         // pairs per kind class
    int cls_groups[4];        // sub-queues that serve each class (>= 1: a divisor, also for a class without pairs)
    bool parked_ok;           // all robot cores of 64 configurations fit LDS: k_validity_redo can re-decide a block without a queue
    bool movable;
};
struct PlanOptions { long long pipeline_tiles, pipe_tile, queue_budget, narrow_parts_max, two_kernel_min_b; };

constexpr size_t WS_MAX_BYTES = size_t(1) << 30;
constexpr int64_t TILE_MAX = int64_t(1) << 22;               // configurations per queue tile at most (65 536 blocks)

// a validity workspace: two counter sets (see TableCache) | per-call float32 broadphase tables | overflow marks | queue items
struct WsLayout {
    static constexpr size_t COUNTER_SET = (size_t)NSUB * CNT_STRIDE * 8;      // NSUB counters, one cache line each
    static constexpr size_t FLAGS = (size_t)(TILE_MAX / WAVE);                // one overflow mark per block of a tile
    size_t tables, flags, items;                                              // byte offsets; the counter sets are at 0 and COUNTER_SET
    explicit WsLayout(int n_wshapes = 0)
        : tables(2 * COUNTER_SET),
          flags((tables + 4 * (5 * 256 + 128 + 6 * (size_t)n_wshapes * 16 + 32 + (size_t)n_wshapes + 16 + 96 * (size_t)n_wshapes + 16) + 255) & ~size_t(255)),
          items(flags + FLAGS) {}
};

struct PairCounts { int n[4]; };      // pairs per kind class that can produce queue items
inline PairCounts all_pairs(const PlanModel& m) { PairCounts c; for (int i = 0; i < 4; ++i) c.n[i] = m.cls_count[i]; return c; }

// capacity (items) of one sub-queue for a tile of nblk 64-configuration blocks: the blocks that feed it times 64 times
// the pairs of its class, maximised over the classes (all sub-queues get the same stride)
inline unsigned long long sub_queue_cap(const PlanModel& m, const PairCounts& pc, unsigned long long nblk) {
    unsigned long long cap = WAVE;
    for (int c = 0; c < 4; ++c) {
        if (pc.n[c] == 0) continue;
        const unsigned long long g = (unsigned long long)m.cls_groups[c];
        const unsigned long long v = ((nblk + g - 1) / g) * WAVE * (unsigned long long)pc.n[c];
        if (v > cap) cap = v;
    }
    return cap;
}

// Queue sizing.  Robots that fit the LDS-parked layout (the queue-less kernel can re-decide a block): one tile of up to TILE_MAX
// configurations, every sub-queue as large as the worst case needs but at most its share of WS_MAX_BYTES -- blocks whose items do
// not fit are re-decided by k_validity_redo.  Larger robots: tiles small enough for the worst case (every pair of every
// configuration), as nothing can catch an overflow for them.
inline int64_t tile_configs(const PlanModel& m, const PairCounts& pc, int64_t B) {
    const int64_t Bp = ((B + WAVE - 1) / WAVE) * WAVE;
    if (m.parked_ok) return Bp < TILE_MAX ? Bp : TILE_MAX;
    double per_cfg = 1.0;
    for (int c = 0; c < 4; ++c) if (pc.n[c] > 0) { const double v = (double)NSUB * pc.n[c] / m.cls_groups[c]; if (v > per_cfg) per_cfg = v; }
    const int64_t P = (int64_t)per_cfg + 1;
    const size_t ws_max = size_t(8) << 30;
    int64_t t = (int64_t)((ws_max - WsLayout(m.n_wshapes).items) / (8 * (size_t)P)) - (int64_t)NSUB * WAVE;
    t = (t / WAVE) * WAVE;
    if (t < 2 * (int64_t)NSUB * WAVE) t = 2 * (int64_t)NSUB * WAVE;
    if (t > TILE_MAX) t = TILE_MAX;
    return Bp < t ? Bp : t;
}
inline unsigned long long tile_queue_cap(const PlanModel& m, const PlanOptions& o, const PairCounts& pc, unsigned long long nblk) {
    const unsigned long long worst = sub_queue_cap(m, pc, nblk);
    if (!m.parked_ok) return worst;
    const size_t header = WsLayout(m.n_wshapes).items;
    size_t bytes = o.queue_budget > 0 ? (size_t)o.queue_budget : WS_MAX_BYTES;
    if (bytes > 2 * header) bytes -= header;                      // the whole workspace, tables included, stays within the budget
    unsigned long long budget = (unsigned long long)(bytes / (8 * (size_t)NSUB));
    if (budget < (unsigned long long)WAVE) budget = WAVE;
    return worst < budget ? worst : budget;
}

// tile size of pipelined batches (pipe_tile): whole 64-configuration blocks (tiles on the two streams must not share a mask word
// or a block), at least one block per sub-queue; anything else is rounded / clamped here, so no value of the switch changes a result
inline int64_t pipe_tile_configs(const PlanOptions& o) {
    int64_t t = o.pipe_tile > 0 ? (int64_t)o.pipe_tile : (int64_t(1) << 20);
    t &= ~int64_t(WAVE - 1);
    const int64_t lo = (int64_t)NSUB * WAVE;
    return t < lo ? lo : t;
}
// batches of at least two such tiles run them alternately on two streams (never inside a capture: the caller's business)
inline bool pipelined(const PlanModel& m, const PlanOptions& o, int64_t B) { return o.pipeline_tiles != 0 && m.parked_ok && B >= 2 * pipe_tile_configs(o); }
inline int64_t call_tile(const PlanModel& m, const PlanOptions& o, const PairCounts& pc, int64_t B, bool pipe) {
    const int64_t t = tile_configs(m, pc, B), pt = pipe_tile_configs(o);
    return pipe && t > pt ? pt : t;
}
// narrowphase workgroups per sub-queue: one 64-item chunk each at a few survivors per configuration; more chunks are strided over
inline unsigned narrow_parts(const PlanOptions& o, unsigned nblk) {
    if (nblk <= 4u) return 1u;                       // a handful of configurations (the scalar calls): 256 workgroups are plenty
    const unsigned pmax = o.narrow_parts_max > 0 ? (unsigned)o.narrow_parts_max : 16u, parts = 4u * nblk / NSUB < 4u ? 4u : 4u * nblk / NSUB;
    return parts > pmax ? pmax : parts;
}

// tiles one after the other on the caller's stream | the tiles of a pipelined batch, odd ones on the library's second stream | those
// tiles, all on the caller's stream (a capture on a stream whose scratch a pipelined call sized).  Tiling never changes a result.
enum class TileMode { Plain, TwoStreams, PipeSerial };

// first configuration, configurations, blocks, items per sub-queue, k_validity_redo follows (the budget sized the queue), narrowphase workgroups per sub-queue
struct Tile { int64_t b0, nb; unsigned nblk; unsigned long long cap_sub; bool redo; unsigned parts; };

// How a call is tiled and what it needs: the entry points size workspaces from `bytes`, the launcher walks at(0 .. tiles - 1).  Tiles
// start on multiples of 64 configurations (mask words never straddle them); `bytes` covers the largest, the first.
struct TilePlan {
    int64_t tile, tiles;
    size_t bytes;
    Tile full, last;
    TilePlan(const PlanModel& m, const PlanOptions& o, const PairCounts& pc, int64_t B, TileMode mode)
        : tile(call_tile(m, o, pc, B, mode != TileMode::Plain)), tiles(tile > 0 ? (B + tile - 1) / tile : 0) {
        auto make = [&](int64_t nb) {
            const unsigned nblk = (unsigned)((nb + WAVE - 1) / WAVE);
            const unsigned long long cap = tile_queue_cap(m, o, pc, nblk);
            return Tile{0, nb, nblk, cap, m.parked_ok && cap < sub_queue_cap(m, pc, nblk), narrow_parts(o, nblk)};
        };
        full = make(B < tile ? B : tile);
        last = tiles > 1 ? make(B - (tiles - 1) * tile) : full;
        bytes = WsLayout(m.n_wshapes).items + 8 * (size_t)NSUB * (size_t)full.cap_sub;
    }
    Tile at(int64_t i) const { Tile t = i + 1 < tiles ? full : last; t.b0 = i * tile; return t; }
};

// bytes nbk_validity_batch_ws needs from its caller (every pair: one workspace serves every threshold); 0 = the fused kernel serves the call
inline int64_t caller_workspace_bytes(const PlanModel& m, const PlanOptions& o, int64_t B) {
    if ((B < o.two_kernel_min_b && m.parked_ok) || m.n_pairs == 0 || B == 0) return 0;
    return (int64_t)TilePlan(m, o, all_pairs(m), B, TileMode::Plain).bytes;
}

// The float32 broadphase tables of a stream's workspace stay valid while the threshold and the world poses do not change, and the
// queue counters exist twice -- a call uses one set, its narrowphase clears the other for the next call -- so steady-state calls
// launch two kernels, not three.  `captured`: a call on this stream has been captured into a hipGraph: its nodes reuse the workspace
// (counter set 0, the tables for THEIR threshold) whenever the graph is replayed, behind the host's back, so direct calls on this
// stream never trust `ready` again -- each prepares its tables and clears both counter sets itself (one more 5 us launch per call).
// The same holds for every stream of a movable descriptor once an update of its world poses has been captured (`world_captured`);
// `world_epoch` is the descriptor's update count the tables were prepared at.
struct TableCache {
    bool ready = false, captured = false; double thr = 0.0; unsigned epoch = 0; unsigned long long world_epoch = 0;
    struct Use { bool prepare; int set, clear; };      // run k_prepare_f32 (it clears both sets)? | this call's set | the set its narrowphase clears
    Use begin(double thr_, unsigned long long world_epoch_, bool world_captured) {
        const bool reuse = ready && !captured && thr == thr_ && world_epoch == world_epoch_ && !world_captured;
        if (!reuse) { ready = true; thr = thr_; world_epoch = world_epoch_; epoch = 0; }
        const Use u = {!reuse, (int)(epoch & 1u), (int)((epoch + 1u) & 1u)};
        epoch += 1u;
        return u;
    }
    void invalidate() { ready = false; }                                 // a new buffer, a failed launch, a broadphase without tables
    void mark_captured() { ready = false; captured = true; }
};

// ---- the sample-generating entries: edge capacity and scratch, the spline plan, the scratch layouts and their typed views ---------
constexpr unsigned long long EDGE_SAMPLES_MAX = 4000000000ull;      // an edge batch stays below this many samples (just under 2^32)

// Capacity = E x (ceil(max_distance / resolution) + 2) samples at least (see nbk_edge_validity_batch), in whole 64-sample blocks
inline unsigned long long edge_capacity(int64_t E, double resolution, double max_distance) {
    double per = ceil(max_distance / resolution) + 2.0;
    if (!(per < 4096.0)) per = 4096.0;                    // an unbounded max_distance: start from 4096 samples per edge
    double c = (double)E * per;
    if (c < 4096.0) c = 4096.0;
    if (c > (double)EDGE_SAMPLES_MAX) c = (double)EDGE_SAMPLES_MAX;
    return ((unsigned long long)c + 63ull) & ~63ull;
}
inline unsigned long long round64(unsigned long long n) { return (n + 63ull) & ~63ull; }

struct EdgeCap { long long edges = 0; unsigned long long samples = 0; };      // what a stream's edge scratch holds

// the capacity a call asks for: the static bound, and 1.25 x the samples the last finished call on the stream needed (`seen`) when it
// had edges that did not fit (`overflowed`: edges its overflow kernel served) -- the two pinned words, 0 before the first call
inline unsigned long long edge_call_capacity(int64_t E, double resolution, double max_distance, unsigned long long seen, unsigned long long overflowed) {
    const unsigned long long cap = edge_capacity(E, resolution, max_distance), want = seen + seen / 4;
    return overflowed != 0ull && want > cap && want < EDGE_SAMPLES_MAX ? round64(want) : cap;
}
// does a scratch of `have` with a validity workspace of ws_bytes serve E edges at capacity `cap`?  The call uses all of have.samples,
// so the workspace has to hold the plain plan of that
inline bool edge_scratch_fits(const PlanModel& m, const PlanOptions& o, const PairCounts& pc, const EdgeCap& have, size_t ws_bytes, int64_t E, unsigned long long cap) {
    return have.edges >= E && have.samples >= cap && ws_bytes >= TilePlan(m, o, pc, (int64_t)have.samples, TileMode::Plain).bytes;
}
inline EdgeCap edge_scratch_grown(const EdgeCap& have, int64_t E, unsigned long long cap) {      // never shrinks
    return {have.edges > E ? have.edges : (long long)E, have.samples > cap ? have.samples : cap};
}
// robots without the parked layout (no overflow kernel) read the exact sample total T back: the capacity it asks for; false = refused
inline bool edge_exact_capacity(unsigned long long T, unsigned long long& cap) { cap = round64(T); return T < EDGE_SAMPLES_MAX; }

// a stream's edge scratch for ne edges and nc samples: plan [ne][3] double | cnt [ne + 1] | offs [ne + 1] | overflow flags [ne],
// then the sample map [nc] and the mask words [nc / 64], each of the three parts rounded up to 4 KiB.  Byte offsets (plan at 0), total
struct EdgeLayout {
    size_t cnt, offs, ovf, map, words, bytes;
    static size_t r4k(size_t n) { return (n + 4095) & ~size_t(4095); }
    EdgeLayout(long long ne, unsigned long long nc)
        : cnt((size_t)ne * 3 * 8), offs(cnt + (size_t)(ne + 1) * 8), ovf(offs + (size_t)(ne + 1) * 8), map(r4k(ovf + (size_t)ne)),
          words(map + r4k((size_t)nc * 8)), bytes(words + r4k(((size_t)nc + 63) / 64 * 8)) {}
    struct View { double* plan; unsigned long long *cnt, *offs; uint8_t* ovf; unsigned long long* map; uint64_t* words; };
    View view(void* base) const {
        char* p = static_cast<char*>(base);
        return {reinterpret_cast<double*>(p), reinterpret_cast<unsigned long long*>(p + cnt), reinterpret_cast<unsigned long long*>(p + offs),
                reinterpret_cast<uint8_t*>(p + ovf), reinterpret_cast<unsigned long long*>(p + map), reinterpret_cast<uint64_t*>(p + words)};
    }
};

// the caller's workspace of nbk_edge_cloud_validity_batch: plan [E][3] double | cnt [E] | offs [E + 1], each part rounded up to 64 bytes
struct EdgeCloudLayout {
    size_t cnt, offs, bytes;
    static size_t r64(size_t n) { return (n + 63) & ~size_t(63); }
    explicit EdgeCloudLayout(int64_t E) : cnt(r64((size_t)E * 24)), offs(cnt + r64((size_t)E * 8)), bytes(offs + r64(((size_t)E + 1) * 8)) {}
    struct View { double* plan; unsigned long long *cnt, *offs; };
    View view(void* base) const {
        char* p = static_cast<char*>(base);
        return {reinterpret_cast<double*>(p), reinterpret_cast<unsigned long long*>(p + cnt), reinterpret_cast<unsigned long long*>(p + offs)};
    }
};
constexpr int64_t EDGE_CLOUD_MAX_E = int64_t(1) << 56;      // the layout's 40 bytes per edge stay far inside int64

// the caller's workspace of nbk_frame_cloud_append for a store of M slots and N new points: the per-256 block counts of the free
// slots (bf blocks) and then of the points kept (ba blocks) as one list cnt [bf + ba] | its exclusive scan offs [bf + ba + 1] |
// slot [N]: the k-th free slot, for k < N (more are never taken).  Each part rounded up to 64 bytes
struct CloudAppendLayout {
    int64_t bf, ba;
    size_t offs, slot, bytes;
    static size_t r64(size_t n) { return (n + 63) & ~size_t(63); }
    CloudAppendLayout(int64_t M, int64_t N)
        : bf((M + 255) / 256), ba((N + 255) / 256), offs(r64((size_t)(bf + ba) * 8)), slot(offs + r64((size_t)(bf + ba + 1) * 8)),
          bytes(slot + r64((size_t)N * 4)) {}
    struct View { unsigned long long *cnt, *offs; int* slot; };
    View view(void* base) const {
        char* p = static_cast<char*>(base);
        return {reinterpret_cast<unsigned long long*>(p), reinterpret_cast<unsigned long long*>(p + offs), reinterpret_cast<int*>(p + slot)};
    }
};

constexpr int64_t SPLINE_TILE = int64_t(1) << 20;           // q rows written and checked per tile of nbk_spline_validity_batch
constexpr int64_t SPLINE_MAX_S = int64_t(1) << 26;          // a spline batch has fewer trajectories than this ...
constexpr unsigned long long SPLINE_MAX_T = 1ull << 31;     // ... and fewer samples than this
// the small half of a stream's spline scratch: knots [nk] | plan [S][2] | cnt [S] | offs [S + 1], each part 256-byte aligned
struct SplineLayout {
    size_t plan, cnt, offs, bytes;
    static size_t r256(size_t n) { return (n + 255) & ~size_t(255); }
    SplineLayout(int nk, int64_t S)
        : plan(r256((size_t)nk * 8)), cnt(plan + r256((size_t)S * 16)), offs(cnt + r256((size_t)S * 8)), bytes(offs + r256((size_t)(S + 1) * 8)) {}
    struct View { double *knots, *plan; unsigned long long *cnt, *offs; };
    View view(void* base) const {
        char* p = static_cast<char*>(base);
        return {reinterpret_cast<double*>(p), reinterpret_cast<double*>(p + plan), reinterpret_cast<unsigned long long*>(p + cnt),
                reinterpret_cast<unsigned long long*>(p + offs)};
    }
};
// the caller's workspace of nbk_spline_cloud_validity_batch: plan [S][2] double | cnt [S] | offs [S + 1] | first [S] (the first-hit
// keys), each part rounded up to 64 bytes: 40 bytes per trajectory whatever the sample count
struct SplineCloudLayout {
    size_t cnt, offs, first, bytes;
    static size_t r64(size_t n) { return (n + 63) & ~size_t(63); }
    explicit SplineCloudLayout(int64_t S)
        : cnt(r64((size_t)S * 16)), offs(cnt + r64((size_t)S * 8)), first(offs + r64(((size_t)S + 1) * 8)), bytes(first + r64((size_t)S * 8)) {}
    struct View { double* plan; unsigned long long *cnt, *offs, *first; };
    View view(void* base) const {
        char* p = static_cast<char*>(base);
        return {reinterpret_cast<double*>(p), reinterpret_cast<unsigned long long*>(p + cnt), reinterpret_cast<unsigned long long*>(p + offs),
                reinterpret_cast<unsigned long long*>(p + first)};
    }
};
// The sample kernel of that entry runs on a grid of fixed size, CUs x this many 64-lane workgroups, and strides to the sample total,
// which only the device knows.  The kernel takes 256 + 162 registers, so ONE wave fits a SIMD and four workgroups are resident per
// CU; 8 per CU is two rounds of them, so that a workgroup whose samples are mostly skipped (behind a first hit) ends early and its
// SIMD takes another instead of idling to the end of the launch.  A guess until it is measured against 4 and 16.
constexpr int SPLINE_CLOUD_WAVES_PER_CU = 8;

// the large half, known once the sample total T (< SPLINE_MAX_T) is read back: mask words [T / 64], rounded up to 256 bytes | the q
// slab [tile][n_q] of one tile, only for a robot with pairs.  Tiles of min(T in whole 64-row blocks, SPLINE_TILE) rows: at(0 .. tiles - 1)
struct SplinePlan {
    int64_t T, tile, tiles;
    bool pairs;
    size_t words_bytes, slab_bytes, bytes;
    SplinePlan(int64_t T_, int n_q, bool pairs_)
        : T(T_), tile((T_ + WAVE - 1) / WAVE * WAVE < SPLINE_TILE ? (T_ + WAVE - 1) / WAVE * WAVE : SPLINE_TILE), tiles(tile > 0 ? (T_ + tile - 1) / tile : 0),
          pairs(pairs_), words_bytes(((size_t)(T_ + 63) / 64 * 8 + 255) & ~size_t(255)), slab_bytes(pairs_ ? (size_t)tile * (size_t)n_q * sizeof(double) : 0),
          bytes(words_bytes + slab_bytes) {}
    struct Tile { int64_t b0, nb; };
    Tile at(int64_t i) const { return {i * tile, T - i * tile < tile ? T - i * tile : tile}; }
    struct View { uint64_t* words; double* slab; };      // slab: nullptr for a robot without pairs
    View view(void* base) const { return {static_cast<uint64_t*>(base), pairs ? reinterpret_cast<double*>(static_cast<char*>(base) + words_bytes) : nullptr}; }
};

}  // namespace nbk
