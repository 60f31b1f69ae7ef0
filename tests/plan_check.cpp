// plan_check.cpp -- stand-alone check of numbotics_amd/csrc/nbk_plan.hpp (tests/test_plan_host.py builds it with the host sanitizers and
// runs it): sweeps the tiling / sizing arithmetic of the validity launch path and holds it against the properties the launcher
// relies on, the scratch layouts and their typed views against their comments, TableCache against the reuse condition written out, the
// capacity and scratch rules of the edge entry and the spline plan against the statements the entry points held before, and three plans
// against values read from the library on an MI355X.  Includes nothing of the project but that header; exits 0 and prints the counts, or
// prints every failed check and exits 1.
#define NBK_PLAN_STANDALONE
#include "../numbotics_amd/csrc/nbk_plan.hpp"

#include <stdio.h>
#include <initializer_list>
#include <utility>

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
    for (int64_t E : {int64_t(1), int64_t(2), int64_t(7), int64_t(8), int64_t(9), int64_t(1000), int64_t(0x7fffffff), EDGE_CLOUD_MAX_E}) {
        const EdgeCloudLayout L(E);
        const size_t e = (size_t)E;
        CHECK(L.cnt >= e * 24 && L.offs >= L.cnt + e * 8 && L.bytes >= L.offs + (e + 1) * 8 && L.bytes <= e * 40 + 8 + 3 * 63, "plan | cnt | offs, E=%lld", (long long)E);
        CHECK(L.cnt % 64 == 0 && L.offs % 64 == 0 && L.bytes % 64 == 0, "64-byte parts");
    }
    for (int nk : {3, 8, 70, 65536 + 6})
        for (int64_t S : {int64_t(1), int64_t(31), int64_t(10000), (int64_t(1) << 26) - 1}) {
            const SplineLayout L(nk, S);
            CHECK(L.plan >= (size_t)nk * 8 && L.cnt >= L.plan + (size_t)S * 16 && L.offs >= L.cnt + (size_t)S * 8 && L.bytes >= L.offs + (size_t)(S + 1) * 8, "ordered");
            CHECK(L.plan % 256 == 0 && L.cnt % 256 == 0 && L.offs % 256 == 0 && L.bytes % 256 == 0, "256-byte parts");
        }
    CHECK(SPLINE_TILE == 1 << 20 && SPLINE_MAX_S == 1 << 26 && SPLINE_MAX_T == 2147483648ull && EDGE_SAMPLES_MAX == 4000000000ull, "the limits of the entries");
    CHECK(edge_capacity(1, 0.05, 1.5) == 4096 && edge_capacity(1500, 0.02, 1.0) == 78016 && edge_capacity(1300, 0.01, 0.25) == 35136, "edge_capacity");
    CHECK(edge_capacity(10, 0.01, INFINITY) == 40960 && edge_capacity(int64_t(1) << 31, 1.0, 100.0) == 4000000000ull, "edge_capacity at its limits");
}

// The typed views: every part where its layout's offset says, inside `bytes`, at the alignment the layout's comment states, and no part
// reaching into the next (checked on a real buffer, for the sizes that fit it)
alignas(4096) static char g_arena[1 << 20];
struct Part { const void* p; size_t size, align; };
static void check_parts(const char* what, std::initializer_list<Part> parts, size_t bytes) {
    size_t end = 0;
    for (const Part& x : parts) {
        const size_t at = (size_t)(static_cast<const char*>(x.p) - g_arena);
        CHECK(x.p != nullptr && at >= end && at % x.align == 0 && at + x.size <= bytes, "%s: a part of %zu bytes at %zu, the one before ends at %zu, %zu in all", what, x.size, at, end, bytes);
        end = at + x.size;
    }
}
static void check_views() {
    for (long long ne : {1ll, 2ll, 500ll, 1300ll})
        for (unsigned long long nc : {64ull, 4096ull, 35136ull, 78016ull}) {
            const EdgeLayout L(ne, nc);
            if (L.bytes > sizeof(g_arena)) continue;
            const EdgeLayout::View v = L.view(g_arena);
            const size_t e = (size_t)ne, c = (size_t)nc;
            check_parts("edge scratch", {{v.plan, e * 24, 8}, {v.cnt, (e + 1) * 8, 8}, {v.offs, (e + 1) * 8, 8}, {v.ovf, e, 1}, {v.map, c * 8, 4096}, {v.words, (c + 63) / 64 * 8, 4096}}, L.bytes);
            CHECK((char*)v.plan == g_arena && (char*)v.cnt == g_arena + L.cnt && (char*)v.offs == g_arena + L.offs && (char*)v.ovf == g_arena + L.ovf &&
                  (char*)v.map == g_arena + L.map && (char*)v.words == g_arena + L.words, "the view follows the offsets");
        }
    for (int64_t E : {int64_t(1), int64_t(2), int64_t(7), int64_t(8), int64_t(9), int64_t(1000), int64_t(26000)}) {
        const EdgeCloudLayout L(E);
        const EdgeCloudLayout::View v = L.view(g_arena);
        const size_t e = (size_t)E;
        CHECK(L.bytes <= sizeof(g_arena), "E=%lld fits the buffer", (long long)E);
        check_parts("cloud edge workspace", {{v.plan, e * 24, 64}, {v.cnt, e * 8, 64}, {v.offs, (e + 1) * 8, 64}}, L.bytes);
        CHECK((char*)v.plan == g_arena && (char*)v.cnt == g_arena + L.cnt && (char*)v.offs == g_arena + L.offs, "the view follows the offsets");
    }
    for (int nk : {3, 8, 70, 65536 + 6})
        for (int64_t S : {int64_t(1), int64_t(31), int64_t(10000)}) {
            const SplineLayout L(nk, S);
            const SplineLayout::View v = L.view(g_arena);
            CHECK(L.bytes <= sizeof(g_arena), "nk=%d S=%lld fits the buffer", nk, (long long)S);
            check_parts("spline scratch", {{v.knots, (size_t)nk * 8, 256}, {v.plan, (size_t)S * 16, 256}, {v.cnt, (size_t)S * 8, 256}, {v.offs, (size_t)(S + 1) * 8, 256}}, L.bytes);
            CHECK((char*)v.knots == g_arena && (char*)v.plan == g_arena + L.plan && (char*)v.cnt == g_arena + L.cnt && (char*)v.offs == g_arena + L.offs, "the view follows the offsets");
        }
}

// ---- the edge and spline entries of nbk.hip before this arithmetic moved into the header (commit 820f3000): their inline statements,
// one by one, as the old rules the header's functions are held equal to -------------------------------------------------------------
static unsigned long long old_edge_capacity(int64_t E, double resolution, double max_distance) {
    double per = ceil(max_distance / resolution) + 2.0;
    if (!(per < 4096.0)) per = 4096.0;
    double c = (double)E * per;
    if (c < 4096.0) c = 4096.0;
    if (c > 4.0e9) c = 4.0e9;
    return ((unsigned long long)c + 63ull) & ~63ull;
}
struct OldEdge {
    long long ecap_edges = 0; unsigned long long ecap_samples = 0; size_t ws_bytes = 0; bool stats = false;
    unsigned long long stats0 = 0, stats1 = 0;          // the pinned words
    unsigned long long capacity(int64_t E, double resolution, double max_distance) const {
        unsigned long long cap = old_edge_capacity(E, resolution, max_distance);
        if (stats && stats1 != 0ull) {
            const unsigned long long seen = stats0;
            const unsigned long long want = seen + seen / 4;
            if (want > cap && want < 4000000000ull) cap = (want + 63ull) & ~63ull;
        }
        return cap;
    }
    bool fits(const PlanModel& m, const PlanOptions& o, const PairCounts& pc, int64_t E, unsigned long long cap) const {
        const bool fits = ecap_edges >= E && ecap_samples >= cap && stats &&
                          ws_bytes >= TilePlan(m, o, pc, (int64_t)ecap_samples, TileMode::Plain).bytes;
        return fits;
    }
    void grow(const PlanModel& m, const PlanOptions& o, const PairCounts& pc, int64_t E, unsigned long long cap) {
        stats = true;
        const long long ne = ecap_edges > E ? ecap_edges : E;
        const unsigned long long nc = ecap_samples > cap ? ecap_samples : cap;
        ecap_edges = ne; ecap_samples = nc;
        const size_t need = TilePlan(m, o, pc, (int64_t)nc, TileMode::Plain).bytes;
        if (ws_bytes < need) ws_bytes = need;                // ensure_validity_ws
    }
    // the read-back of a robot without the parked layout: 0 go on, 1 resize to `cap` and go round again, 2 refused
    static int exact(unsigned long long total, unsigned long long& cap, int attempt) {
        if (total <= cap) return 0;
        if (attempt == 1 || total >= 4000000000ull) return 2;
        cap = (total + 63ull) & ~63ull;
        return 1;
    }
};

static void check_edge_rules() {
    const int count[4] = {16, 74, 18, 13}, groups[4] = {34, 156, 38, 28};
    const std::pair<double, double> steps[] = {{0.05, 1.5}, {0.02, 1.0}, {0.01, 0.25}, {0.01, (double)INFINITY}};
    for (int parked = 0; parked < 2; ++parked) {
        const PlanModel m = model(parked != 0, count, groups, 8);
        const PairCounts pc = all_pairs(m);
        for (int64_t E : {int64_t(1), int64_t(2), int64_t(400), int64_t(1300), int64_t(1500), int64_t(0x7fffffff)})
            for (const auto& rd : steps) {
                const unsigned long long bound = edge_capacity(E, rd.first, rd.second);
                CHECK(bound == old_edge_capacity(E, rd.first, rd.second) && bound % 64 == 0 && bound >= 4096 && bound <= EDGE_SAMPLES_MAX, "E=%lld: static bound %llu", (long long)E, bound);
                for (unsigned long long seen : {0ull, 1ull, bound - 1, bound, 5 * bound, 3990000000ull, 4000000000ull})
                    for (unsigned long long overflowed : {0ull, 1ull}) {
                        OldEdge old;
                        old.stats = true; old.stats0 = seen; old.stats1 = overflowed;
                        const unsigned long long cap = edge_call_capacity(E, rd.first, rd.second, seen, overflowed);
                        CHECK(cap == old.capacity(E, rd.first, rd.second), "E=%lld seen=%llu overflowed=%llu: capacity %llu, before %llu", (long long)E, seen, overflowed, cap, old.capacity(E, rd.first, rd.second));
                        CHECK(cap % 64 == 0 && cap >= bound && cap <= EDGE_SAMPLES_MAX + 63, "capacity %llu over the bound %llu", cap, bound);
                        if (overflowed && seen + seen / 4 < EDGE_SAMPLES_MAX) CHECK(cap >= seen + seen / 4, "headroom over the %llu samples seen: %llu", seen, cap);
                        // scratch sizes below, at and above what is asked, workspaces one byte short of, at and above what they serve
                        for (long long he : {(long long)E - 1, (long long)E, (long long)E + 1})
                            for (unsigned long long hs : {cap - 64, cap, cap + 64}) {
                                const EdgeCap have = {he, hs};
                                const size_t serve = TilePlan(m, DEFAULTS, pc, (int64_t)hs, TileMode::Plain).bytes;
                                for (size_t ws : {serve - 1, serve, serve + 4096}) {
                                    old.ecap_edges = he; old.ecap_samples = hs; old.ws_bytes = ws;
                                    const bool fits = edge_scratch_fits(m, DEFAULTS, pc, have, ws, E, cap);
                                    CHECK(fits == old.fits(m, DEFAULTS, pc, E, cap), "fits: %lld edges %llu samples %zu bytes for E=%lld cap=%llu", he, hs, ws, (long long)E, cap);
                                    CHECK(fits == (he >= E && hs >= cap && ws >= serve), "fits, written out");
                                    // the call then covers all of have.samples: its plan is what the workspace has to hold
                                    if (fits) CHECK(have.samples >= cap && have.edges >= E && ws >= TilePlan(m, DEFAULTS, pc, (int64_t)have.samples, TileMode::Plain).bytes, "fits and cannot serve");
                                    const EdgeCap g = edge_scratch_grown(have, E, cap);
                                    OldEdge after = old;
                                    after.grow(m, DEFAULTS, pc, E, cap);
                                    CHECK(g.edges == after.ecap_edges && g.samples == after.ecap_samples, "growth to %lld edges %llu samples, before %lld and %llu", g.edges, g.samples, after.ecap_edges, after.ecap_samples);
                                    CHECK(g.edges >= have.edges && g.samples >= have.samples && g.edges >= E && g.samples >= cap && g.samples % 64 == 0, "growth never shrinks and serves the call");
                                    CHECK(edge_scratch_fits(m, DEFAULTS, pc, g, after.ws_bytes, E, cap), "a grown scratch fits");
                                }
                            }
                    }
                // the exact resize of a robot without the parked layout: one read-back, one more pass at the most
                for (unsigned long long T : {0ull, 1ull, 63ull, 64ull, 65ull, (1ull << 20) - 1, 1ull << 20, (1ull << 20) + 1, (1ull << 31) - 1, 3990000000ull, 3999999999ull, 4000000000ull, 1ull << 40}) {
                    unsigned long long old_cap = bound, exact = 0;
                    const int verdict = OldEdge::exact(T, old_cap, 0);
                    const bool ok = edge_exact_capacity(T, exact);
                    CHECK(ok == (T < EDGE_SAMPLES_MAX), "T=%llu refused at the limit only", T);
                    if (T > bound) {                  // (the launcher asks only then)
                        CHECK((verdict == 2) == !ok && (verdict != 1 || exact == old_cap), "T=%llu over %llu: exact %llu ok %d, before %llu verdict %d", T, bound, exact, (int)ok, old_cap, verdict);
                        if (ok) CHECK(exact % 64 == 0 && exact >= T && exact < T + 64 && OldEdge::exact(T, exact, 1) == 0, "the second pass holds T=%llu: %llu", T, exact);
                    } else {
                        CHECK(verdict == 0, "T=%llu fits %llu", T, bound);
                    }
                }
            }
    }
}

static void check_spline_plan() {
    for (int64_t T : {int64_t(0), int64_t(1), int64_t(63), int64_t(64), int64_t(65), (int64_t(1) << 20) - 1, int64_t(1) << 20, (int64_t(1) << 20) + 1, (int64_t(1) << 31) - 1})
        for (int n_q : {1, 7, 32})
            for (bool pairs : {false, true}) {
                // nbk_spline_validity_batch before SplinePlan
                const int64_t a = (T + WAVE - 1) / WAVE * WAVE;
                const int64_t tile = a < SPLINE_TILE ? a : SPLINE_TILE;                        // std::min<int64_t>(.., SPLINE_TILE)
                const size_t words_bytes = ((size_t)(T + 63) / 64 * 8 + 255) & ~size_t(255);
                const size_t slab_bytes = pairs ? (size_t)tile * (size_t)n_q * sizeof(double) : 0;
                const SplinePlan p(T, n_q, pairs);
                CHECK(p.T == T && p.pairs == pairs && p.tile == tile && p.words_bytes == words_bytes && p.slab_bytes == slab_bytes && p.bytes == words_bytes + slab_bytes,
                      "T=%lld n_q=%d pairs=%d: tile %lld words %zu slab %zu", (long long)T, n_q, (int)pairs, (long long)p.tile, p.words_bytes, p.slab_bytes);
                CHECK(p.tile % 64 == 0 && p.tile <= SPLINE_TILE && (T == 0) == (p.tile == 0) && p.words_bytes % 256 == 0 && p.words_bytes >= (size_t)(T + 63) / 64 * 8, "tile %lld", (long long)p.tile);
                int64_t next = 0, i = 0;
                for (int64_t b0 = 0; b0 < T; b0 += tile, ++i) {                                 // the loop of the entry point, before
                    const int64_t nb = tile < T - b0 ? tile : T - b0;
                    const SplinePlan::Tile t = p.at(i);
                    CHECK(i < p.tiles && t.b0 == b0 && t.nb == nb, "tile %lld: rows %lld + %lld, before %lld + %lld", (long long)i, (long long)t.b0, (long long)t.nb, (long long)b0, (long long)nb);
                    CHECK(t.b0 == next && t.b0 % 64 == 0 && t.nb > 0 && t.nb <= p.tile, "tile %lld starts at %lld", (long long)i, (long long)t.b0);
                    CHECK(((size_t)t.b0 / 64 + (size_t)(t.nb + 63) / 64) * 8 <= p.words_bytes && (!pairs || (size_t)t.nb * (size_t)n_q * 8 <= p.slab_bytes), "tile %lld stays inside its buffer", (long long)i);
                    next += t.nb;
                }
                CHECK(i == p.tiles && next == T, "%lld tiles cover %lld of %lld rows", (long long)p.tiles, (long long)next, (long long)T);
                if (p.bytes <= sizeof(g_arena) && T > 0) {
                    const SplinePlan::View v = p.view(g_arena);
                    CHECK((char*)v.words == g_arena && (pairs ? (char*)v.slab == g_arena + p.words_bytes : v.slab == nullptr), "words | slab");
                }
            }
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
    check_views();
    check_edge_rules();
    check_spline_plan();
    check_table_cache();
    check_pinned();
    printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
