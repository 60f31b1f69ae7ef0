// lds_check.cpp -- stand-alone check of numbotics_amd/csrc/nbk_lds.hpp (tests/test_lds_host.py builds it with the host sanitizers and runs
// it).  Sweeps n_q 1..32, n_joints 1..32, frame_slots 0..32, path_len 0..32, shape_rows from 0 to beyond the parked limit, S 0..40 (the
// three buckets), W and P over small values, the boundaries and the descriptor limits, hull_blob_n around HULL_LDS_MAX / 8, the four
// k_distances modes, and holds for every layout, over the pointers its accessors (the kernels' own carve) return for a host buffer:
//   parent equality      bytes() and every served / refused verdict equal the host expressions this header replaced (the *_lds helpers,
//                        lds_f, nlds, the cloud launches and the three rules of check_limits), transcribed below as they stood;
//   in bounds            every region ends at or before bytes(), the last one at it (two exceptions, stated where they are checked);
//   no overlap           regions that are live at the same time do not overlap;
//   aliases covered      each region that reuses another fits into it (named at its check);
//   alignment            every region starts on a multiple of its element size, what stage_q / stage_rows read as double2 on 16 bytes;
//   creation implies fit for every descriptor check_limits accepts, every kernel the dispatch can choose fits or its entry point refuses --
//                        with ONE exemption, asserted to be exactly this: k_edges for a robot without pairs and without the parked layout
//                        (nbk_edge_validity_batch launches it unguarded; the launch over-asks).  Its count is printed on a line of its own.
// Includes nothing of the project but that header; exits 0 and prints the counts, or prints every failed check and exits 1.
#include "../numbotics_amd/csrc/nbk_lds.hpp"

#include <stdio.h>
#include <algorithm>
#include <vector>

using namespace nbk;
constexpr int WAVE = LDS_WAVE, BQ_CAP = LDS_BQ_CAP;      // the names the transcribed expressions use

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        ++g_checks;                                                                       \
        if (!(cond)) { if (++g_failed <= 40) { printf("FAILED %s:%d  %s  [", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("]\n"); } } \
    } while (0)

// ---- the parent's host expressions, as they stood in nbk.hip, nbk_cloud.hpp and nbk_tables.hpp ---------------------------------------
namespace parent {
struct Desc { int n_q, shape_rows, frame_slots, n_rshapes, n_wshapes, n_pairs, hull_blob_n; };
struct Model { int n_q, n_joints; Desc d; };
constexpr int VALIDITY_LDS_EXTRA = QUEUE_CAP * 4 + WAVE * 4;
constexpr int NBK_ZSLOTS = 2;
static size_t fk_lds(const Model* m) { return sizeof(double) * WAVE * (size_t)(m->n_q > 17 ? m->n_q : 17); }
static size_t fk_frames_lds(const Model* m) { return fk_lds(m) + sizeof(double) * WAVE * ((size_t)m->n_q + 12 * (size_t)m->d.frame_slots); }
static size_t jacobian_reg_lds(const Model* m) { return sizeof(double) * std::max((size_t)WAVE * m->n_q, (size_t)JAC_ROWS * ((6 * m->n_q) | 1)); }
static size_t jacobian_lds(const Model* m) { return sizeof(double) * WAVE * ((size_t)m->n_q + 6 * (size_t)m->n_q + 1); }
static size_t ik_lds(const Model* m, int path_len) { return sizeof(double) * WAVE * ((size_t)m->n_q * 7 + 6 * (size_t)(path_len > 0 ? path_len : 1)); }
static size_t collide_lds(const Model* m) {
    return sizeof(double) * WAVE * ((size_t)m->d.n_q + (size_t)m->d.shape_rows + 12 * (size_t)m->d.frame_slots) + VALIDITY_LDS_EXTRA;
}
static size_t closest_lds(const Model* m) { return collide_lds(m) - VALIDITY_LDS_EXTRA + sizeof(double) * CQ_CAP + 12 * WAVE + 6 * CQ_CAP; }
static size_t distances_lds(const Model* m) { return collide_lds(m) + 8 * EPAQ_DOUBLES; }
static size_t proximity_lds(const Model* m) { return distances_lds(m) + sizeof(double) * WAVE * 6 * (size_t)m->n_joints; }
static int broad_bucket(int S) { return S <= 8 ? 8 : (S <= 12 ? 12 : 16); }
static int f32_qrows(int nq, int S) { return nq > (S + 2) / 2 ? nq : (S + 2) / 2; }
static size_t broad_lds(const Model* m) {
    const size_t qrows = ((size_t)WAVE * m->d.n_q * 8 >= (size_t)BQ_CAP * 4) ? (size_t)m->d.n_q : ((size_t)BQ_CAP * 4 + WAVE * 8 - 1) / (WAVE * 8);
    return sizeof(double) * (WAVE * (qrows + 12 * (size_t)m->d.frame_slots + 3 * (size_t)m->d.n_rshapes) + 4 * (size_t)m->d.n_pairs + 18 * (size_t)m->d.n_wshapes);
}
static size_t broad_reg_lds(const Model* m, int S) {
    const size_t qrows = ((size_t)WAVE * m->d.n_q * 8 >= (size_t)BQ_CAP * 4) ? (size_t)m->d.n_q : ((size_t)BQ_CAP * 4 + WAVE * 8 - 1) / (WAVE * 8);
    const size_t W = (size_t)m->d.n_wshapes;
    return sizeof(double) * (WAVE * (qrows + 12 * (size_t)m->d.frame_slots) + (size_t)S * S + 2 * W * S) + sizeof(int) * ((size_t)S * S + W * S) + 16;
}
static size_t lds_f(const Model* m, int bucket) {      // launch_tile
    const size_t qrows_f = (size_t)f32_qrows(m->d.n_q, bucket);
    return sizeof(double) * WAVE * qrows_f + sizeof(float) * WAVE * 12 * (size_t)m->d.frame_slots + 16 + sizeof(float) * WAVE * NBK_ZSLOTS;
}
static size_t spec_lds(const Model* m, int bucket) { return sizeof(double) * WAVE * (size_t)f32_qrows(m->d.n_q, bucket); }      // the hipModuleLaunchKernel of launch_tile
static size_t narrow_hull_lds(int hull_blob_n) { return (hull_blob_n > 0 && (size_t)hull_blob_n * 8 <= (size_t)HULL_LDS_MAX) ? (size_t)hull_blob_n * 8 : 0; }
static size_t nlds(const Model* m) { return sizeof(double) * NARROW_T * (size_t)m->n_q + narrow_hull_lds(m->d.hull_blob_n); }
static size_t pair_items_lds(const Model* m, bool rows) {
    return sizeof(double) * WAVE * ((size_t)(m->n_q > 0 ? m->n_q : 1) + (rows ? 6 * (size_t)m->n_joints : 0));
}
static size_t cloud_lds(const Model* m) { return sizeof(double) * WAVE * (size_t)m->n_q; }      // the three launches of nbk_cloud.hpp
static size_t spline_ca_lds(const Model* m) { return sizeof(double) * WAVE * (size_t)(m->n_q > 0 ? m->n_q : 1); }
// check_limits: 0 = NBK_OK, 1 = NBK_ERR_UNSUPPORTED; rows and slots are ModelTables' (t.rows, t.slots)
struct Limits { int rc; bool lds_broad_ok, parked_ok; };
static Limits check_limits(int n_q, int rows, int slots, int S, int W, int P) {
    Limits t = {1, false, false};
    if (3 * S >= 65536 || W >= 65536) return t;
    t.lds_broad_ok = (size_t)(n_q + 12 * slots + 3 * S) * 64 * sizeof(double) + (4 * (size_t)P + 18 * (size_t)W) * sizeof(double) + BQ_CAP * 4 <= LDS_MAX;
    if (!t.lds_broad_ok && S > 16) return t;
    if (P >= (1 << 20)) return t;
    const size_t lds_bytes = (size_t)(n_q + (rows > n_q ? rows : n_q) + 12 * slots) * 64 * sizeof(double) + VALIDITY_LDS_EXTRA;
    t.parked_ok = lds_bytes <= LDS_MAX;
    if (S <= 16 && (size_t)n_q * 64 * sizeof(double) + 12 * (size_t)slots * 64 * sizeof(float) + 4096 > LDS_MAX) return t;
    if (P >= (1 << 26)) return t;
    t.rc = 0;
    return t;
}
}  // namespace parent

// check_limits as it stands now (nbk_tables.hpp), on plain integers
static parent::Limits check_limits_now(int n_q, int rows, int slots, int S, int W, int P) {
    parent::Limits t = {1, false, false};
    if (3 * S >= 65536 || W >= 65536 || P >= (1 << 20)) return t;
    t.lds_broad_ok = lds_broad_ok(n_q, slots, S, P, W);
    if (!t.lds_broad_ok && S > 16) return t;
    t.parked_ok = ValidityLds(n_q, rows > n_q ? rows : n_q, slots).fits();
    if (S <= 16 && !broad_f32_ok(n_q, slots, S)) return t;
    t.rc = 0;
    return t;
}

// ---- regions ------------------------------------------------------------------------------------------------------------------------------
struct Region { const char* name; size_t begin, bytes, elem; bool d2; size_t end() const { return begin + bytes; } };      // d2: read or written as double2
// The host buffer the accessors are called on in place of the dynamic LDS: it holds the largest layout of the sweep (check_regions holds that)
static std::vector<double> g_buf((size_t)6 << 20);
static double* const lds = g_buf.data();
// `count` elements from `p`, a pointer an accessor returned: the begin is its distance from the base, the element size its type's
template <class T> static Region region(const char* name, T* p, size_t count, bool d2 = false) { return {name, (size_t)((const char*)p - (const char*)lds), count * sizeof(T), sizeof(T), d2}; }

// in bounds, aligned, pairwise disjoint (the regions given are live at the same time); end_slack >= 0: the last one ends that many bytes before bytes()
static void check_regions(const char* what, const std::vector<Region>& rs, size_t total, long end_slack = -1) {
    CHECK(total <= g_buf.size() * sizeof(double), "%s: %zu bytes beyond the host buffer", what, total);
    if (end_slack >= 0) CHECK(rs.back().end() + (size_t)end_slack == total, "%s: %s ends at %zu, bytes() = %zu", what, rs.back().name, rs.back().end(), total);
    for (size_t i = 0; i < rs.size(); ++i) {
        const Region& r = rs[i];
        CHECK(r.end() <= total, "%s: %s ends at %zu of %zu", what, r.name, r.end(), total);
        CHECK(r.begin % r.elem == 0 && (!r.d2 || r.begin % 16 == 0), "%s: %s starts at byte %zu", what, r.name, r.begin);
        for (size_t j = i + 1; j < rs.size(); ++j) {
            const Region& o = rs[j];
            CHECK(r.bytes == 0 || o.bytes == 0 || r.end() <= o.begin || o.end() <= r.begin, "%s: %s [%zu, %zu) and %s [%zu, %zu)", what, r.name, r.begin, r.end(), o.name, o.begin, o.end());
        }
    }
}
// `alias` lies inside `host`
static void check_alias(const char* what, const Region& alias, const Region& host) {
    CHECK(alias.begin >= host.begin && alias.end() <= host.end(), "%s: %s [%zu, %zu) outside %s [%zu, %zu)", what, alias.name, alias.begin, alias.end(), host.name, host.begin, host.end());
    CHECK(alias.begin % alias.elem == 0 && (!alias.d2 || alias.begin % 16 == 0), "%s: %s starts at byte %zu", what, alias.name, alias.begin);
}

static long g_edges_no_pairs = 0;      // see check_creation

// ---- the families ---------------------------------------------------------------------------------------------------------------------------
static void check_kinematics(int n_q, int n_joints, int slots, int path_len) {
    const parent::Model pm = {n_q, n_joints, {n_q, n_q, slots, 0, 0, 0, 0}};
    const size_t slab = (size_t)WAVE * n_q;
    {
        const FkLds L(n_q);
        CHECK(L.bytes() == parent::fk_lds(&pm) && L.fits(), "fk n_q=%d", n_q);
        check_regions("k_fk q", {region("raw q", lds, slab, true)}, L.bytes());      // one region, no accessor: the base itself
        check_regions("k_fk out", {region("poses", lds, (size_t)WAVE * 17)}, L.bytes());
    }
    {
        const FkFramesLds L(n_q, slots);
        CHECK(L.bytes() == parent::fk_frames_lds(&pm) && L.fits() == (parent::fk_frames_lds(&pm) <= LDS_MAX), "fk_frames n_q=%d slots=%d", n_q, slots);
        const Region t = region("transpose", L.t(lds), L.t_len());
        check_regions("k_fk_frames", {region("q rows", L.q(lds), (size_t)L.q_len), region("frames", L.fr(lds), (size_t)L.fr_len), t}, L.bytes(), 0);
        CHECK((size_t)L.q_len == slab && L.fr_len == WAVE * 12 * slots, "k_fk_frames lengths");
        check_alias("k_fk_frames", region("raw q", L.t(lds), slab, true), t);
        check_alias("k_fk_frames", region("poses", L.t(lds), (size_t)WAVE * 17), t);
    }
    {
        const JacobianLds L(n_q);
        CHECK(L.bytes() == parent::jacobian_lds(&pm) && L.fits() == (parent::jacobian_lds(&pm) <= LDS_MAX), "jacobian n_q=%d", n_q);
        CHECK(L.stride() == ((6 * n_q) | 1), "jacobian stride");
        check_regions("k_jacobian", {region("raw q", L.q(lds), (size_t)L.q_len, true), region("rows", L.o(lds), (size_t)WAVE * L.stride())}, L.bytes(), 0);
    }
    {
        const JacobianRegLds L(n_q);
        CHECK(L.bytes() == parent::jacobian_reg_lds(&pm) && L.fits(), "jacobian_reg n_q=%d", n_q);
        const Region all = region("LDS", lds, L.bytes() / 8), q = region("raw q", L.q(lds), L.q_len(), true), o = region("rows", L.o(lds), L.o_len());
        check_alias("k_jacobian_reg", q, all);
        check_alias("k_jacobian_reg", o, all);      // the rows reuse the q area
        CHECK(L.q_len() == slab && L.o_len() == (size_t)JAC_ROWS * ((6 * n_q) | 1) && o.begin == q.begin, "k_jacobian_reg lengths; the rows start where q starts");
        CHECK(std::max(q.end(), o.end()) == L.bytes(), "k_jacobian_reg: the longer of the two ends where the launch's bytes end");
    }
    {
        const IkLds L(n_q, path_len);
        CHECK(L.bytes() == parent::ik_lds(&pm, path_len) && L.fits() == (parent::ik_lds(&pm, path_len) <= LDS_MAX), "ik n_q=%d len=%d", n_q, path_len);
        CHECK(L.jz_len() >= (size_t)WAVE * 6 * path_len, "k_ik: jz holds 6 rows per joint of the path");
        check_regions("k_ik", {region("q rows", L.q(lds), (size_t)L.q_len), region("J", L.J(lds), (size_t)L.J_len), region("jz", L.jz(lds), L.jz_len())}, L.bytes(), 0);
        CHECK(IkLds(n_q).q_len == L.q_len && IkLds(n_q).J_len == L.J_len, "k_ik: the kernel's construction, without the path length");
    }
    for (int rows = 0; rows < 2; ++rows) {
        const PairItemsLds L(n_q, rows ? n_joints : 0);
        CHECK(L.bytes() == parent::pair_items_lds(&pm, rows != 0) && L.fits(), "pair_items n_q=%d J=%d", n_q, n_joints);
        check_regions("k_pair_items", {region("q rows", L.q(lds), (size_t)L.q_len), region("jz", L.jz(lds), L.jz_len())}, L.bytes(), 0);
        CHECK(L.jz_len() == (rows ? (size_t)WAVE * 6 * n_joints : 0) && PairItemsLds(n_q).q_len == L.q_len, "k_pair_items lengths");
    }
    CHECK(QSlabLds(n_q).bytes() == parent::cloud_lds(&pm) && QSlabLds(n_q).fits(), "cloud n_q=%d", n_q);
    CHECK(QSlabLds(n_q, 1).bytes() == parent::spline_ca_lds(&pm) && QSlabLds(n_q, 1).fits(), "spline_ca n_q=%d", n_q);
    check_regions("q slab", {region("q rows", lds, slab)}, QSlabLds(n_q).bytes(), 0);
}

static void check_narrow(int n_q, int hull_blob_n) {
    const parent::Model pm = {n_q, 1, {n_q, n_q, 0, 0, 0, 0, hull_blob_n}};
    const NarrowLds L(n_q, hull_blob_n);
    CHECK(L.bytes() == parent::nlds(&pm) && L.fits(), "narrow n_q=%d hull=%d", n_q, hull_blob_n);
    CHECK(L.hull_staged() == (hull_blob_n > 0 && (size_t)hull_blob_n * 8 <= (size_t)HULL_LDS_MAX) && L.hull_len() == (L.hull_staged() ? (size_t)hull_blob_n : 0), "hull_staged(%d)", hull_blob_n);
    check_regions("k_narrow", {region("q rows", L.q(lds), (size_t)L.q_len), region("hull", L.hull(lds), L.hull_len())}, L.bytes(), 0);
    CHECK(L.q_len == NARROW_T * n_q, "k_narrow q rows");
}

static void check_parked(int n_q, int n_joints, int shape_rows, int slots) {
    const parent::Model pm = {n_q, n_joints, {n_q, shape_rows, slots, 0, 0, 0, 0}};
    const size_t slab = (size_t)WAVE * n_q;
    auto body = [&](const ParkedLds& L) {
        CHECK((size_t)L.q_len == slab && L.s_len == WAVE * shape_rows && L.fr_len == WAVE * 12 * slots, "parked lengths");
        return std::vector<Region>{region("q rows", L.q(lds), (size_t)L.q_len), region("shape rows", L.s(lds), (size_t)L.s_len), region("frames", L.fr(lds), (size_t)L.fr_len)};
    };
    {
        const ValidityLds L(n_q, shape_rows, slots);
        CHECK(L.bytes() == parent::collide_lds(&pm) && L.fits() == (parent::collide_lds(&pm) <= LDS_MAX), "validity n_q=%d rows=%d slots=%d", n_q, shape_rows, slots);
        CHECK(ValidityLds::TAIL_BYTES == parent::VALIDITY_LDS_EXTRA, "VALIDITY_LDS_EXTRA");
        std::vector<Region> rs = body(L);
        rs.insert(rs.end(), {region("queue", L.queue(lds), ValidityLds::QUEUE_LEN), region("hit flags", L.hit(lds), ValidityLds::HIT_LEN)});
        check_regions("validity", rs, L.bytes(), 0);
        // the raw q slab is staged in the shape area: holds for every descriptor, whose shape_rows is max(rows, n_q)
        if (shape_rows >= n_q) check_alias("validity", region("raw q", L.s(lds), slab, true), rs[1]);
    }
    for (int mode = 0; mode < 4; ++mode) {
        const DistancesLds L(n_q, shape_rows, slots, n_joints, mode);
        const size_t was = mode == 0 ? parent::collide_lds(&pm) : (mode == 3 ? parent::proximity_lds(&pm) : parent::distances_lds(&pm));
        CHECK(L.bytes() == was && L.fits() == (was <= LDS_MAX), "distances<%d> n_q=%d rows=%d slots=%d J=%d", mode, n_q, shape_rows, slots, n_joints);
        CHECK(L.nwave() == (mode == 0 ? 1 : 2) && L.jz_len == (mode == 3 ? WAVE * 6 * n_joints : 0), "distances<%d> waves, jz", mode);
        std::vector<Region> rs = body(L);
        rs.push_back(region("jz", L.jz(lds), (size_t)L.jz_len));
        for (int w = 0; w < L.nwave(); ++w) {
            rs.push_back(region(w ? "EPA depths 1" : "EPA depths 0", L.epaq_depth(lds, w), EPAQ_CAP));
            rs.push_back(region(w ? "EPA items 1" : "EPA items 0", L.epaq_item(lds, w), EPAQ_CAP));
        }
        check_regions("distances", rs, L.bytes(), ValidityLds::TAIL_BYTES - 8 * EPAQ_DOUBLES);      // bytes() keeps the whole validity tail where the first wave's EPA queue lies
        // the first wave's EPA queue lives in the tail the validity path sized for its own queue
        CHECK((size_t)EPAQ_DOUBLES * 8 <= (size_t)ValidityLds::TAIL_BYTES && EPAQ_DOUBLES * 8 == EPAQ_CAP * (8 + 4), "the validity tail holds one EPA queue");
    }
    {
        const ClosestLds L(n_q, shape_rows, slots);
        CHECK(L.bytes() == parent::closest_lds(&pm) && L.fits() == (parent::closest_lds(&pm) <= LDS_MAX), "closest n_q=%d rows=%d slots=%d", n_q, shape_rows, slots);
        std::vector<Region> rs = body(L);
        rs.insert(rs.end(), {region("results", L.res(lds), ClosestLds::RES_LEN), region("best", L.best(lds), ClosestLds::BEST_LEN), region("argmin", L.arg(lds), ClosestLds::ARG_LEN),
                             region("queue", L.queue(lds), ClosestLds::QUEUE_LEN), region("EPA list", L.elist(lds), ClosestLds::ELIST_LEN)});
        check_regions("closest", rs, L.bytes(), 0);      // the unsigned short list ends where the launch's bytes end
    }
}

static void check_broad(int n_q, int slots, int S, int W, int P) {
    const parent::Model pm = {n_q, 1, {n_q, n_q, slots, S, W, P, 0}};
    const size_t slab = (size_t)WAVE * n_q;
    {
        const BroadLds L(n_q, slots, S, P, W);
        CHECK(L.bytes() == parent::broad_lds(&pm) && L.fits() == (parent::broad_lds(&pm) <= LDS_MAX), "broad n_q=%d slots=%d S=%d W=%d P=%d", n_q, slots, S, W, P);
        const Region q = region("q slab", L.slab(lds), (size_t)L.slab_len, true);
        check_regions("k_broad", {q, region("frames", L.fr(lds), (size_t)L.fr_len), region("centres", L.c(lds), (size_t)L.c_len),
                                  region("pair constants", L.pc(lds), (size_t)L.pc_len), region("world cores", L.w(lds), (size_t)L.w_len)}, L.bytes(), 0);
        CHECK(L.slab_len == WAVE * L.qrows && L.fr_len == WAVE * 12 * slots && L.c_len == WAVE * 3 * S && L.pc_len == 4 * P && L.w_len == 18 * W, "k_broad lengths");
        const BroadLds K(n_q, slots, S, P);      // the kernel's construction, without the world shapes
        CHECK(K.slab_len == L.slab_len && K.fr_len == L.fr_len && K.c_len == L.c_len && K.pc_len == L.pc_len, "k_broad: the kernel's construction");
        check_alias("k_broad", region("raw q", L.slab(lds), slab, true), q);
        check_alias("k_broad", region("item queue", L.queue(lds), BQ_CAP), q);
        CHECK(L.qcap() >= BQ_CAP && (size_t)L.qcap() * 4 == q.bytes, "k_broad qcap %d", L.qcap());
    }
    if (S <= 16) {
        const int b = broad_bucket(S);
        CHECK(b == parent::broad_bucket(S) && b >= S && f32_qrows(n_q, b) == parent::f32_qrows(n_q, b), "bucket of S=%d", S);
        {
            const BroadRegLds L(n_q, slots, b, W);
            CHECK(L.bytes() == parent::broad_reg_lds(&pm, b) && L.fits() == (parent::broad_reg_lds(&pm, b) <= LDS_MAX), "broad_reg n_q=%d slots=%d S=%d W=%d", n_q, slots, b, W);
            const Region q = region("q slab", L.slab(lds), (size_t)L.slab_len, true);
            check_regions("k_broad_reg", {q, region("frames", L.fr(lds), (size_t)L.fr_len), region("rkey", L.rkey(lds), (size_t)L.rkey_len), region("wkey", L.wkey(lds), (size_t)L.wkey_len),
                                          region("wtc", L.wtc(lds), (size_t)L.wtc_len), region("rp", L.rp(lds), (size_t)L.rp_len), region("wp", L.wp(lds), (size_t)L.wp_len)}, L.bytes(), 16);      // the launch asks for 16 bytes more
            CHECK(L.slab_len == WAVE * L.qrows && L.rkey_len == b * b && L.wkey_len == W * b && L.wtc_len == W * b && L.rp_len == b * b && L.wp_len == W * b, "k_broad_reg lengths");
            check_alias("k_broad_reg", region("raw q", L.slab(lds), slab, true), q);
            check_alias("k_broad_reg", region("item queue", L.queue(lds), BQ_CAP), q);
            CHECK(L.qcap() >= BQ_CAP, "k_broad_reg qcap %d", L.qcap());
        }
        {
            const BroadF32Lds L(n_q, slots, b);
            CHECK(L.bytes() == parent::lds_f(&pm, b) && L.slab_bytes() == parent::spec_lds(&pm, b), "broad_f32 n_q=%d slots=%d S=%d", n_q, slots, b);
            const Region q = region("q slab", L.slab(lds), (size_t)L.slab_len, true), fr = region("frames", L.fr(lds), (size_t)L.fr_len);
            const Region z = region("z", L.zp(lds) + LDS_ZFIRST * WAVE, (size_t)WAVE * LDS_ZSLOTS);      // the kernel's pointer is indexed by slot: row NBK_ZFIRST is the first stored
            check_regions("k_broad_f32", {q, fr, z}, L.bytes(), 0);
            CHECK(z.begin % 16 == 0 && z.begin - (fr.begin + fr.bytes) == 16, "z starts 16 bytes behind the frames, on 16 bytes");
            CHECK(L.bytes() == fr.begin + fr.bytes + BroadF32Lds::TAIL_BYTES && L.fr_len == WAVE * 12 * slots, "TAIL_BYTES");
            CHECK(fr.begin == L.slab_bytes() && fr.begin + 4 * ((size_t)L.fr_len + BroadF32Lds::Z_PAD) == z.begin, "the z row of slot NBK_ZFIRST");
            check_alias("k_broad_f32", region("raw q", L.slab(lds), slab, true), q);
            check_alias("k_broad_f32", region("item queue", L.queue(lds), (size_t)L.qcap()), q);
            check_alias("k_broad_f32", region("centre z rows", L.czrows(lds), (size_t)b * WAVE), q);
            CHECK(L.qcap() >= BQ_CAP && L.qcap() >= b * WAVE, "qcap %d: the general stage's queue and one unrolled block's items", L.qcap());
            CHECK(L.slab_bytes() == q.bytes, "the per-robot kernel's LDS is the slab");
        }
    }
}

// Creation implies fit.  rows, slots: ModelTables'; the descriptor's shape_rows is max(rows, n_q).  The dispatch conditions of call_setup /
// launch_tile and of the entry points as plain booleans, the switches both ways.  Sites whose guard is the fits() of the very layout they
// launch hold by construction and are not restated: k_broad_reg (call_setup falls back to k_broad_f32), k_closest (else k_distances<0>),
// k_distances<1..3>, k_fk_frames, k_jacobian, k_ik; and the sites behind parked_ok, which IS ValidityLds::fits() of the descriptor's numbers:
// k_validity, k_validity_redo, k_distances<0>, the small-batch and overflow launches of k_edges.
static void check_creation(int n_q, int n_joints, int rows, int slots, int S, int W, int P) {
    const parent::Limits was = parent::check_limits(n_q, rows, slots, S, W, P), now = check_limits_now(n_q, rows, slots, S, W, P);
    CHECK(was.rc == now.rc, "check_limits n_q=%d rows=%d slots=%d S=%d W=%d P=%d: %d, was %d", n_q, rows, slots, S, W, P, now.rc, was.rc);
    if (was.rc != 0 || now.rc != 0) return;
    CHECK(was.lds_broad_ok == now.lds_broad_ok && was.parked_ok == now.parked_ok, "verdicts n_q=%d rows=%d slots=%d S=%d W=%d P=%d", n_q, rows, slots, S, W, P);
    const int shape_rows = rows > n_q ? rows : n_q;
    const bool parked_ok = now.parked_ok;
    // nbk_edge_validity_batch launches k_edges directly when (E < edge_batch_min_e && parked_ok) || n_pairs == 0.  The one exemption: it
    // over-asks exactly for a robot without pairs and without the parked layout, whatever the batch size
    for (int small = 0; small < 2; ++small) {
        const bool launched = (small && parked_ok) || P == 0;
        const bool over_asks = launched && !ValidityLds(n_q, shape_rows, slots).fits();
        CHECK(over_asks == (P == 0 && !parked_ok), "k_edges over-asks: n_q=%d rows=%d slots=%d P=%d small=%d", n_q, rows, slots, P, small);
    }
    if (P == 0 && !parked_ok) ++g_edges_no_pairs;
    // the broadphase of call_setup: creation's two rules (each stricter than the launch by its named constant) must cover the launch
    for (int no_reg_broad = 0; no_reg_broad < 2; ++no_reg_broad) {
        if (S <= 16 && (!no_reg_broad || !now.lds_broad_ok))      // k_broad_f32 (or k_broad_reg where it fits), and the per-robot kernel's slab
            CHECK(BroadF32Lds(n_q, slots, broad_bucket(S)).fits(), "k_broad_f32 n_q=%d slots=%d S=%d", n_q, slots, S);
        else
            CHECK(BroadLds(n_q, slots, S, P, W).fits(), "k_broad n_q=%d slots=%d S=%d W=%d P=%d", n_q, slots, S, W, P);
    }
    // launched without any test: k_narrow* with the largest staged hull, k_pair_items, k_fk, k_jacobian_reg, k_spline_ca and the cloud kernels
    CHECK(NarrowLds(n_q, HULL_LDS_MAX / 8).fits() && PairItemsLds(n_q, n_joints).fits() && FkLds(n_q).fits() && JacobianRegLds(n_q).fits() && QSlabLds(n_q, 1).fits(),
          "entries that refuse nothing n_q=%d J=%d", n_q, n_joints);
}

int main() {
    const int hull_edge = HULL_LDS_MAX / 8;
    for (int n_q = 1; n_q <= 32; ++n_q) {
        for (int hb : {0, 1, hull_edge - 1, hull_edge, hull_edge + 1, 1 << 20, 1 << 28, 0x7fffffff}) check_narrow(n_q, hb);
        for (int slots = 0; slots <= 32; ++slots) {
            for (int len = 0; len <= 32; ++len) check_kinematics(n_q, 1 + (len + slots) % 32, slots, len);
            check_kinematics(n_q, 32, slots, 32);
            // shape_rows: small, every value around the parked limit of this (n_q, slots), and beyond
            const int limit = ((int)LDS_MAX - ValidityLds::TAIL_BYTES) / 512 - n_q - 12 * slots;
            std::vector<int> rows = {0, 1, n_q - 1, n_q, n_q + 1, 37, 100, 200, 400, 1000};
            for (int r = limit - 12; r <= limit + 12; ++r) if (r >= 0) rows.push_back(r);
            for (int r : rows) {
                for (int J : {1, 7, 24, 32}) check_parked(n_q, J, r, slots);
                for (int S : {0, 1, 8, 9, 16, 17, 25, 40})
                    for (int W : {0, 3})
                        check_creation(n_q, 1 + (r + slots) % 32, r, slots, S, W, S == 0 ? 0 : 5 * S + 2 * W);
            }
        }
        for (int slots : {0, 1, 8, 31, 32})
            for (int S = 0; S <= 40; ++S)
                for (int W : {0, 1, 2, 7, 100, 1000, 2000, 9000, 65535})
                    for (int P : {0, 1, 63, 64, 65, 1000, 5000, 20000, (1 << 20) - 1}) {
                        check_broad(n_q, slots, S, W, P);
                        check_creation(n_q, 7, 3 * S, slots, S, W, P);
                    }
    }
    // the descriptor limits of check_limits, and the lds_broad_ok boundary (P steps the bytes by 32)
    for (int n_q : {1, 3, 4, 7, 32})
        for (int S : {0, 16, 17, 40, 21844, 21845, 21846})
            for (int W : {0, 65535, 65536})
                for (int P : {0, (1 << 20) - 1, 1 << 20, (1 << 26) - 1, 1 << 26, 0x7fffffff}) check_creation(n_q, 7, S < 100 ? 3 * S : 12, 8, S, W, P);
    for (int n_q = 1; n_q <= 32; ++n_q)
        for (int S : {17, 25, 40}) {
            const int slots = 8, W = 4;
            const int edge = (int)((LDS_MAX - 8 * (64 * (size_t)(n_q + 12 * slots + 3 * S) + 18 * W) - 2048) / 32);
            for (int P = edge - 80; P <= edge + 80; ++P) if (P >= 0) { check_creation(n_q, 7, 3 * S, slots, S, W, P); check_broad(n_q, slots, S, W, P); }
        }
    printf("exempt: k_edges launched beyond LDS_MAX for a robot without pairs and without the parked layout: %ld descriptors\n", g_edges_no_pairs);
    printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
