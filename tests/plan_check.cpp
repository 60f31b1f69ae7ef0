// plan_check.cpp -- stand-alone check of numbotics_amd/csrc/nbk_plan.hpp (tests/test_plan_host.py builds it with the host sanitizers and
// runs it): sweeps the tiling / sizing arithmetic of the validity launch path and holds it against the properties the launcher
// relies on, the scratch layouts against their comments, TableCache against the reuse condition written out, and three plans against
// values read from the library on an MI355X.  Includes nothing of the project but that header; exits 0 and prints the counts, or
// prints every failed check and exits 1.
#define NBK_PLAN_STANDALONE
#include "../numbotics_amd/csrc/nbk_plan.hpp"

#include <stdio.h>
#include <initializer_list>

using namespace nbk;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        ++g_checks;                                                                       \
        if (!(cond)) { if (++g_failed <= 40) { printf("FAILED %s:%d  %s  [", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("]\n"); } } \
    } while (0)

static const PlanOptions DEFAULTS = {1, 1ll << 20, 1ll << 30, 16, 1};      // OPTION_TABLE of nbk.hip

static PlanModel model(bool parked_ok, const int (&count)[4], const int (&groups)[4], int n_wshapes = 3) {
    PlanModel m = {7, count[0] + count[1] + count[2] + count[3], 9, n_wshapes, 8, {}, {}, parked_ok, false};
    for (int c = 0; c < 4; ++c) { m.cls_count[c] = count[c]; m.cls_groups[c] = groups[c]; }
    return m;
}

// the rounding rule in the comment on pipe_tile_configs, written out
static int64_t expected_pipe_tile(long long value) {
    int64_t t = value > 0 ? value : (int64_t(1) << 20);
    t = t / 64 * 64;
    return t < 16384 ? 16384 : t;
}

static void check_plan(const PlanModel& m, const PlanOptions& o, const PairCounts& pc, int64_t B, TileMode mode) {
    const TilePlan p(m, o, pc, B, mode);
    const size_t header = WsLayout(m.n_wshapes).items;
    const int md = (int)mode;
    CHECK(p.tile > 0 && p.tile % 64 == 0 && p.tile <= TILE_MAX, "B=%lld mode=%d tile=%lld", (long long)B, md, (long long)p.tile);
    CHECK(p.tiles == (B + p.tile - 1) / p.tile, "B=%lld tiles=%lld", (long long)B, (long long)p.tiles);
    int64_t next = 0;
    for (int64_t i = 0; i < p.tiles; ++i) {
        const Tile t = p.at(i);
        CHECK(t.b0 == next && t.b0 % 64 == 0, "B=%lld tile %lld starts at %lld, expected %lld", (long long)B, (long long)i, (long long)t.b0, (long long)next);
        CHECK(t.nb > 0 && (i + 1 == p.tiles ? t.nb <= p.tile : t.nb == p.tile), "B=%lld tile %lld has %lld rows", (long long)B, (long long)i, (long long)t.nb);
        CHECK(t.nblk == (unsigned)((t.nb + 63) / 64), "nblk %u for %lld rows", t.nblk, (long long)t.nb);
        // sizing / launching agreement: what the call asked for holds the queue of every tile it launches
        CHECK(p.bytes >= header + 8 * (size_t)NSUB * (size_t)t.cap_sub, "B=%lld mode=%d tile %lld: bytes %zu < header %zu + queue of %llu", (long long)B, md,
              (long long)i, p.bytes, header, t.cap_sub);
        const unsigned long long worst = sub_queue_cap(m, pc, t.nblk);
        CHECK(t.cap_sub >= 64 && t.cap_sub <= worst, "cap_sub %llu, worst %llu", t.cap_sub, worst);
        CHECK(t.redo == (m.parked_ok && t.cap_sub < worst), "redo %d parked %d cap %llu worst %llu", (int)t.redo, (int)m.parked_ok, t.cap_sub, worst);
        if (!m.parked_ok) CHECK(!t.redo && t.cap_sub == worst, "a robot without the parked layout cannot re-decide a block");
        const unsigned pmax = o.narrow_parts_max > 0 ? (unsigned)o.narrow_parts_max : 16u;
        CHECK(t.parts >= 1 && (t.nblk <= 4 ? t.parts == 1 : (t.parts <= (pmax > 4 ? pmax : 4) && t.parts >= (pmax < 4 ? pmax : 4))), "parts %u for %u blocks", t.parts, t.nblk);
        next += t.nb;
    }
    CHECK(next == B, "tiles cover %lld of %lld rows", (long long)next, (long long)B);
    const int64_t pt = pipe_tile_configs(o);
    CHECK(pt == expected_pipe_tile(o.pipe_tile), "pipe_tile %lld -> %lld", o.pipe_tile, (long long)pt);
    CHECK(pipelined(m, o, B) == (o.pipeline_tiles != 0 && m.parked_ok && B >= 2 * pt), "pipelined(B=%lld)", (long long)B);
    const int64_t whole = tile_configs(m, pc, B);
    CHECK(p.tile == (mode != TileMode::Plain && whole > pt ? pt : whole), "mode %d tile %lld (pipe tile %lld, whole %lld)", md, (long long)p.tile, (long long)pt, (long long)whole);
    if (m.parked_ok && mode == TileMode::Plain) CHECK(p.tiles == (B + TILE_MAX - 1) / TILE_MAX, "parked robots: one tile up to TILE_MAX");
    // a capture after a pipelined call runs that call's tiles in that call's workspace
    if (mode == TileMode::PipeSerial) {
        const TilePlan two(m, o, pc, B, TileMode::TwoStreams);
        CHECK(p.bytes <= two.bytes && p.tile == two.tile && p.tiles == two.tiles, "serial %zu bytes, alternating %zu", p.bytes, two.bytes);
    }
}

static void sweep() {
    const int counts[3][4] = {{40, 30, 20, 31}, {0, 60, 0, 61}, {0, 0, 0, 0}};
    const int groups[3][4] = {{85, 64, 43, 64}, {1, 127, 1, 127}, {1, 1, 1, 1}};
    const int64_t batches[] = {1, 63, 64, 65, 4096, 32768, 32769, int64_t(1) << 20, (int64_t(1) << 22) + 1};
    const long long pipe_tiles[] = {0, 1, 63, 64, 16384, 100000, (1ll << 20) + 1};
    const long long budgets[] = {DEFAULTS.queue_budget, 1ll << 20, 1};
    for (int parked = 0; parked < 2; ++parked)
        for (int k = 0; k < 3; ++k) {
            const PlanModel m = model(parked != 0, counts[k], groups[k]);
            const PairCounts all = all_pairs(m);
            PairCounts some = all, none = {{0, 0, 0, 0}};                   // what a threshold can leave of them
            for (int c = 0; c < 4; ++c) some.n[c] = all.n[c] / 2;
            some.n[3] = 0;
            for (int64_t B : batches)
                for (long long pt : pipe_tiles)
                    for (long long budget : budgets) {
                        PlanOptions o = DEFAULTS;
                        o.pipe_tile = pt; o.queue_budget = budget;
                        for (TileMode mode : {TileMode::Plain, TileMode::TwoStreams, TileMode::PipeSerial}) {
                            for (const PairCounts& pc : {all, some, none}) check_plan(m, o, pc, B, mode);
                            const size_t b_all = TilePlan(m, o, all, B, mode).bytes;
                            CHECK(b_all >= TilePlan(m, o, some, B, mode).bytes && b_all >= TilePlan(m, o, none, B, mode).bytes, "every pair sizes for every threshold");
                        }
                        // the caller's workspace: nothing for the fused kernel, else the plain plan for every pair
                        CHECK(caller_workspace_bytes(m, o, 0) == 0, "B = 0");
                        CHECK(caller_workspace_bytes(m, o, B) == (m.n_pairs == 0 ? 0 : (int64_t)TilePlan(m, o, all, B, TileMode::Plain).bytes), "caller bytes");
                        o.two_kernel_min_b = B + 1;
                        CHECK((caller_workspace_bytes(m, o, B) == 0) == (m.parked_ok || m.n_pairs == 0), "two_kernel_min_b");
                    }
        }
    PlanOptions off = DEFAULTS;
    off.pipeline_tiles = 0;
    CHECK(!pipelined(model(true, counts[0], groups[0]), off, int64_t(1) << 23), "pipeline_tiles = 0");
    CHECK(!pipelined(model(false, counts[0], groups[0]), DEFAULTS, int64_t(1) << 23), "no pipeline without the parked layout");
}

static void check_layouts() {
    for (int W : {0, 1, 3, 1000}) {
        const WsLayout L(W);
        CHECK(L.tables == 2 * WsLayout::COUNTER_SET && WsLayout::COUNTER_SET == 256 * 16 * 8, "two counter sets ahead of the tables");
        CHECK(L.flags >= L.tables + 4 * (size_t)(1472 + 193 * W) && L.flags % 256 == 0 && L.items == L.flags + 65536 && L.items % 256 == 0, "W=%d", W);
    }
    const long long edges[] = {1, 2, 500, 1300, 100000, 0x7fffffffLL};
    const unsigned long long samples[] = {64, 4096, 35136, 78016, 4000000000ull};
    for (long long ne : edges)
        for (unsigned long long nc : samples) {
            const EdgeLayout L((long long)ne, nc);
            const size_t e = (size_t)ne, c = (size_t)nc;
            CHECK(L.cnt == e * 24 && L.offs == L.cnt + (e + 1) * 8 && L.ovf == L.offs + (e + 1) * 8, "plan | cnt | offs | flags");
            CHECK(L.map >= L.ovf + e && L.map % 4096 == 0, "map");
            CHECK(L.words >= L.map + c * 8 && L.words % 4096 == 0, "words");
            CHECK(L.bytes >= L.words + (c + 63) / 64 * 8 && L.bytes % 4096 == 0 && L.bytes < L.words + (c + 63) / 64 * 8 + 4096, "bytes");
        }
    for (int nk : {3, 8, 70, 65536 + 6})
        for (int64_t S : {int64_t(1), int64_t(31), int64_t(10000), (int64_t(1) << 26) - 1}) {
            const SplineLayout L(nk, S);
            CHECK(L.plan >= (size_t)nk * 8 && L.cnt >= L.plan + (size_t)S * 16 && L.offs >= L.cnt + (size_t)S * 8 && L.bytes >= L.offs + (size_t)(S + 1) * 8, "ordered");
            CHECK(L.plan % 256 == 0 && L.cnt % 256 == 0 && L.offs % 256 == 0 && L.bytes % 256 == 0, "256-byte parts");
        }
    CHECK(SPLINE_TILE == 1 << 20, "SPLINE_TILE");
    CHECK(edge_capacity(1, 0.05, 1.5) == 4096 && edge_capacity(1500, 0.02, 1.0) == 78016 && edge_capacity(1300, 0.01, 0.25) == 35136, "edge_capacity");
    CHECK(edge_capacity(10, 0.01, INFINITY) == 40960 && edge_capacity(int64_t(1) << 31, 1.0, 100.0) == 4000000000ull, "edge_capacity at its limits");
}

// the reuse condition and the state updates of the launcher before TableCache, statement by statement
struct OldState {
    bool ready = false, captured = false; double thr = 0.0; unsigned epoch = 0; unsigned long long world_epoch = 0;
    TableCache::Use begin(double threshold, unsigned long long world_epoch_, bool world_captured) {
        TableCache::Use u;
        if (ready && !captured && thr == threshold && world_epoch == world_epoch_ && !world_captured) {
            u = {false, (int)(epoch & 1u), (int)((epoch + 1u) & 1u)};
        } else {
            u = {true, 0, 1};
            ready = true; thr = threshold; world_epoch = world_epoch_; epoch = 0;
        }
        epoch += 1u;
        return u;
    }
};

static void check_table_cache() {
    TableCache t;
    OldState old;
    struct Step { const char* what; double thr; unsigned long long world; bool world_captured; int before; bool prepare; };    // before: 1 invalidate, 2 mark_captured
    const Step script[] = {
        {"first call", 0.0, 0, false, 0, true},          {"same threshold", 0.0, 0, false, 0, false},
        {"same threshold again", 0.0, 0, false, 0, false}, {"and again", 0.0, 0, false, 0, false},
        {"new threshold", 0.01, 0, false, 0, true},      {"same", 0.01, 0, false, 0, false},
        {"world epoch bump", 0.01, 1, false, 0, true},   {"same", 0.01, 1, false, 0, false},
        {"after a new buffer / failed launch", 0.01, 1, false, 1, true}, {"same", 0.01, 1, false, 0, false},
        {"a captured world update", 0.01, 1, true, 0, true}, {"world moves on", 0.01, 2, false, 0, true}, {"same", 0.01, 2, false, 0, false},
        {"after a capture on this stream", 0.01, 2, false, 2, true}, {"same threshold again", 0.01, 2, false, 0, true},
        {"and never again", 0.01, 2, false, 0, true},
    };
    int last_set = -1;
    for (const Step& s : script) {
        if (s.before == 1) { t.invalidate(); old.ready = false; }
        if (s.before == 2) { t.mark_captured(); old.ready = false; old.captured = true; }
        const TableCache::Use u = t.begin(s.thr, s.world, s.world_captured), w = old.begin(s.thr, s.world, s.world_captured);
        CHECK(u.prepare == s.prepare && u.prepare == w.prepare, "%s: prepare %d", s.what, (int)u.prepare);
        CHECK(u.set == w.set && u.clear == w.clear, "%s: sets %d/%d, before %d/%d", s.what, u.set, u.clear, w.set, w.clear);
        CHECK(u.clear == 1 - u.set && (u.prepare ? u.set == 0 : u.set == 1 - last_set), "%s: set %d after %d", s.what, u.set, last_set);
        CHECK(t.ready == old.ready && t.captured == old.captured && t.thr == old.thr && t.epoch == old.epoch && t.world_epoch == old.world_epoch, "%s: state", s.what);
        last_set = u.set;
    }
}

// Three plans of the parent of this header (commit fab2e798bd0c, where this arithmetic still lived in nbk.hip), the descriptors of the
// scenes c2, c3 and c5m (pairs per kind class from their pair lists, sub-queues per class by queue_groups' rule): the bytes
// nbk_validity_workspace_bytes answered there, and (tiles, rows per tile, pipelined) as DeviceModel.last_tiling() reported after a
// validity call of that size.  Constants of that build, not of this header.
struct Pinned { const char* what; int n_wshapes; int count[4], groups[4]; int64_t B; long long pipe_tile, budget; int64_t bytes, tiles, tile; bool piped; };
static void check_pinned() {
    const Pinned pins[] = {
        {"c2, 20 000 rows, defaults", 1, {2, 18, 18, 6}, {12, 105, 104, 35}, 20000, 1ll << 20, 1ll << 30, 9575168, 1, 20032, false},
        {"c3, 81 937 rows, pipe_tile 16384", 8, {16, 74, 18, 13}, {34, 156, 38, 28}, 81937, 16384, 1ll << 30, 87437312, 6, 16384, true},
        {"c5m, 32 768 rows, pipe_tile 16384, queue_budget 1 MiB", 8, {0, 0, 0, 121}, {1, 1, 1, 256}, 32768, 16384, 1ll << 20, 1048576, 2, 16384, true},
    };
    for (const Pinned& p : pins) {
        const PlanModel m = model(true, p.count, p.groups, p.n_wshapes);
        PlanOptions o = DEFAULTS;
        o.pipe_tile = p.pipe_tile; o.queue_budget = p.budget;
        CHECK(caller_workspace_bytes(m, o, p.B) == p.bytes, "%s: %lld bytes, pinned %lld", p.what, (long long)caller_workspace_bytes(m, o, p.B), (long long)p.bytes);
        CHECK(pipelined(m, o, p.B) == p.piped, "%s: pipelined", p.what);
        const TilePlan plan(m, o, all_pairs(m), p.B, p.piped ? TileMode::TwoStreams : TileMode::Plain);
        CHECK(plan.tiles == p.tiles && plan.tile == p.tile, "%s: %lld tiles of %lld rows, pinned %lld of %lld", p.what, (long long)plan.tiles, (long long)plan.tile,
              (long long)p.tiles, (long long)p.tile);
    }
}

int main() {
    sweep();
    check_layouts();
    check_table_cache();
    check_pinned();
    printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
