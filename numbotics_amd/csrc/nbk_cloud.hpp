// nbk_cloud.hpp -- point-cloud obstacles (include/nbk.h: nbk_cloud_*; DESIGN.md 3, "Point clouds").  Included once by nbk.hip, after
// its own entry points: the kernels here use DevModel, joint_apply, build_core and epa_refine of nbk.hip and the predicate / distance
// routines of nbk_device.hpp, and nothing of the validity launch path (no queue, no table, no scratch of a descriptor).
//
// A cloud is N points of one radius, sorted into a uniform grid (nbk_cloud_grid.hpp) on the device:
//   hdr            status (0 ok, 2 a non-finite point), N and the radius of the last update -- written on the device, in stream order,
//                  so that a query sees what the update ahead of it in its stream (or in its graph) set, not what the host last asked for
//   fill  [cells]  points per cell while counting; the scatter's cursors afterwards
//   start [cells+1] first sorted slot of each cell (exclusive scan of the counts); start[cells] = N
//   cell_of [cap]  cell of each original point (count -> scatter)
//   idx   [cap]    original index of each sorted point
//   pts   [cap][3] sorted points
// nbk_cloud_set_points: one memset (hdr + fill) | k_cloud_count | k_cloud_scan | k_cloud_scatter.  The order of the points of one
// cell depends on the arrival of the scatter's atomics; no result does (a verdict is an OR; the clearance breaks ties by the original
// index).  With a mask (nbk_frame_cloud_set_points; the plain update is that call without one) N is the number of points kept: the
// others are neither counted nor stored, and idx keeps the indices the caller's array has.
//
// Depth frames: k_cloud_backproject (one pixel per lane, the arithmetic of nbk_cloud_depth.hpp) and k_cloud_self_filter (the query
// predicate at ONE configuration against many points, the selected shapes' cores once per workgroup in LDS) write the points and the
// mask such an update takes.
//
// Fused frames (several frames in one cloud): the caller's store of point slots is the array an update with a mask takes, so a point's
// index in a record is its slot.  k_cloud_carve releases the slots a new frame sees through (depth_carve_point, nbk_cloud_depth.hpp),
// k_cloud_novel drops the frame points the cloud of the previous update still holds within a merge distance (the walk of the queries),
// k_cloud_append_count | nbk.hip's k_scan | k_cloud_append_slots | k_cloud_append_write move the rest into free slots by the ranks of
// a two-level scan (CloudAppendLayout, nbk_plan.hpp: the caller's workspace).
//
// Queries: one configuration per lane, 64 per workgroup; the wave takes the selected robot shapes one after the other (Core.kind and
// the hull a core names are wave-uniform this way), replays FK along the shape's joint mask from the lane's staged q row, builds the
// shape's core and walks the cells cloud_cell_range gives for the ball the pair predicate's bounding-sphere step can pass.  Cells are
// numbered x fastest, so one (y, z) row of the range is one contiguous run of sorted points.
//
// Sampled edges (nbk_edge_cloud_validity_batch): the edge rule is nbk.hip's own (k_edge_plan, k_scan, edge_sample_row); the samples of
// all edges form one flat range (cloud_flat_owner: whose sample a lane holds) that k_cloud_edges walks one sample per lane with the
// walk of k_cloud_validity (cloud_row_hits).  Plan, counts and offsets live in the caller's workspace (EdgeCloudLayout, nbk_plan.hpp).
//
// Certified edges (nbk_edge_cloud_continuous_batch): nbk.hip's k_edge_ca_init -> k_cloud_edge_ca (ca_walk on CloudEdgeLane) -> nbk.hip's
// k_ca_final; the keys and their reserved values are defined once, beside ca_key.
//
// B-spline trajectories (nbk_spline_cloud_validity_batch, nbk_spline_cloud_continuous_batch): the trajectory rule is nbk.hip's own
// (k_spline_plan, k_scan, spline_span, de_boor, k_spline_ca_init, SplineSpanMotion); k_cloud_spline walks one sample per lane on a grid
// of fixed size with a first-hit word per trajectory in the caller's workspace (SplineCloudLayout, nbk_plan.hpp), k_cloud_spline_ca is
// ca_walk on CloudSplineLane.
//
// Entry points: each states its own argument rules, then cloud_call_begin (selection limit, devices, selection, selected count); the
// sampled entries check their workspace with cloud_workspace_ok.
#pragma once
#define NBK_GRID_FN __host__ __device__ inline
#include "nbk_cloud_grid.hpp"
#include "nbk_cloud_depth.hpp"

namespace nbk {

constexpr int SELF_FILTER_WGS_PER_CU = 4;      // k_cloud_self_filter: workgroups per CU of its bounded grid

struct CloudHdr { int status; int n; double radius; };
static_assert(sizeof(CloudHdr) == 16, "the update's memset covers the header and the counters in one piece");

struct CloudDev {                 // what the query kernels read (by value)
    CloudGrid g;
    const CloudHdr* hdr;
    const double* pts;
    const int* idx;
    const unsigned* start;
};

// robot shapes a query looks at, in the descriptor's device (frame) order
struct CloudSel { unsigned long long w[4]; int all; };
NBK_DEV bool cloud_selected(const CloudSel& s, int i) { return s.all != 0 || ((s.w[(i >> 6) & 3] >> (i & 63)) & 1ull) != 0ull; }

// ---- the update ---------------------------------------------------------------------------------------------------------------
// keep (optional, nbk_frame_cloud_set_points): point i takes part iff keep[i] != 0 -- a point that does not is neither counted nor
// looked at (its coordinates may be anything), and k_cloud_scatter leaves it out by the same test
__global__ __launch_bounds__(256) void k_cloud_count(CloudGrid g, const double* __restrict__ pts, int n, const uint8_t* __restrict__ keep,
                                                     int* __restrict__ cell_of, unsigned* __restrict__ fill, int* __restrict__ status) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    if (keep != nullptr && keep[i] == 0) return;
    const double p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    const bool finite = (p[0] - p[0] == 0.0) && (p[1] - p[1] == 0.0) && (p[2] - p[2] == 0.0);
    if (!finite) atomicMax(status, 2);
    const int c = finite ? cloud_cell(g, p) : 0;
    cell_of[i] = c;
    atomicAdd(&fill[c], 1u);
}

// one workgroup: thread t owns the cells [t * per, (t + 1) * per); counts -> exclusive offsets in `start` and the scatter's cursors in `fill`.
// The points the cloud holds are the points counted (all that were submitted, or those a mask kept): the scan's own total
__global__ __launch_bounds__(1024) void k_cloud_scan(unsigned* __restrict__ fill, unsigned* __restrict__ start, int cells,
                                                     CloudHdr* __restrict__ hdr, double radius) {
    __shared__ unsigned part[1024];
    const int t = (int)threadIdx.x;
    const int per = (cells + 1023) / 1024;
    const int lo = t * per < cells ? t * per : cells;
    const int hi = lo + per < cells ? lo + per : cells;
    unsigned sum = 0u;
    for (int c = lo; c < hi; ++c) sum += fill[c];
    part[t] = sum;
    __syncthreads();
    // inclusive scan of the 1024 partial sums (Hillis-Steele)
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned run = part[t] - sum;
    for (int c = lo; c < hi; ++c) {
        const unsigned v = fill[c];
        start[c] = run;
        fill[c] = run;
        run += v;
    }
    if (t == 0) { const unsigned total = part[1023]; start[cells] = total; hdr->n = (int)total; hdr->radius = radius; }
}

__global__ __launch_bounds__(256) void k_cloud_scatter(const double* __restrict__ pts, int n, const uint8_t* __restrict__ keep,
                                                       const int* __restrict__ cell_of, unsigned* __restrict__ fill,
                                                       double* __restrict__ sorted, int* __restrict__ idx, unsigned cap) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    if (keep != nullptr && keep[i] == 0) return;
    const unsigned pos = atomicAdd(&fill[cell_of[i]], 1u);
    if (pos >= cap) return;            // (cannot happen: the cursors start at the scan of these very counts)
    sorted[3 * (size_t)pos] = pts[3 * (size_t)i];
    sorted[3 * (size_t)pos + 1] = pts[3 * (size_t)i + 1];
    sorted[3 * (size_t)pos + 2] = pts[3 * (size_t)i + 2];
    idx[pos] = i;
}

// ---- depth frames (nbk_frame_cloud_backproject) -------------------------------------------------------------------------------------------
// One pixel per lane, i = v * W + u its point; the arithmetic is depth_backproject_pixel's (nbk_cloud_depth.hpp).  T: the optical
// frame's pose [3][4] in DEVICE memory, read when the kernel runs: a replayed graph follows a camera whose pose is rewritten in place.
__global__ __launch_bounds__(256) void k_cloud_backproject(const void* __restrict__ depth, int depth_type, int W, int n, DepthCam cam,
                                                           const double* __restrict__ T, double* __restrict__ pts,
                                                           uint8_t* __restrict__ keep) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    double Tm[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) Tm[e] = T[e];
    double w[3];
    const bool valid = depth_backproject_pixel(cam, Tm, i % W, i / W, depth_pixel_value(depth, depth_type, i), w);
    pts[3 * (size_t)i] = w[0];
    pts[3 * (size_t)i + 1] = w[1];
    pts[3 * (size_t)i + 2] = w[2];
    keep[i] = valid ? 1 : 0;
}

// ---- fused frames: carving (nbk_frame_cloud_carve) ------------------------------------------------------------------------------------
// One stored point per lane: a slot that is held and that the frame sees through (depth_carve_point, nbk_cloud_depth.hpp) is released.
// Only store_keep is written, and only 1 -> 0; T as k_cloud_backproject takes it.
__global__ __launch_bounds__(256) void k_cloud_carve(const void* __restrict__ depth, int depth_type, int H, int W, DepthCam cam,
                                                     const double* __restrict__ T, double margin, int window,
                                                     const double* __restrict__ store_pts, int m, uint8_t* __restrict__ store_keep) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= m) return;
    if (store_keep[i] == 0) return;
    double Tm[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) Tm[e] = T[e];
    const double p[3] = {store_pts[3 * (size_t)i], store_pts[3 * (size_t)i + 1], store_pts[3 * (size_t)i + 2]};
    if (depth_carve_point(cam, Tm, depth, depth_type, H, W, p, margin, window)) store_keep[i] = 0;
}

// ---- the walk of one lane over the cells of a ball ----------------------------------------------------------------------------
struct CloudWalk { int x0, x1, y0, y1, z1, y, z; unsigned cur, end; bool more; };

NBK_DEV void cloud_walk_begin(const CloudDev& c, bool on, const double* centre, double R, CloudWalk& w) {
    int lo[3], hi[3];
    w.more = cloud_cell_range(c.g, centre, R, lo, hi) && on;
    w.x0 = lo[0]; w.x1 = hi[0]; w.y0 = lo[1]; w.y1 = hi[1]; w.z1 = hi[2];
    w.y = lo[1] - 1; w.z = lo[2];
    w.cur = w.end = 0u;
}
// true: sorted point w.cur is the next one (the caller consumes it with ++w.cur)
NBK_DEV bool cloud_walk_next(const CloudDev& c, CloudWalk& w) {
    while (w.cur == w.end) {
        if (!w.more) return false;
        if (++w.y > w.y1) {
            w.y = w.y0;
            if (++w.z > w.z1) { w.more = false; return false; }
        }
        const int row = (w.z * c.g.dims[1] + w.y) * c.g.dims[0];
        w.cur = c.start[row + w.x0];
        w.end = c.start[row + w.x1 + 1];
    }
    return true;
}

// ---- fused frames: novelty (nbk_frame_cloud_novel) -------------------------------------------------------------------------------------
// One frame point per lane: keep[i] goes 1 -> 0 iff the cloud holds a point s -- counted only while held[idx[s]] != 0, when a `held`
// mask is given: the cloud of the last update less what has been released since -- with
//     ((dx * dx + dy * dy) + dz * dz) < merge * merge,   dx = p[0] - pts[s][0], ...          (strict; plain products and sums)
// The walk is the ball of radius merge around the point (nbk_cloud_grid.hpp: the range is sound for exactly this predicate form).
// N, status and the grid are the device's: while the status is set or N is 0 nothing of the grid is read.  An OR: the order of the
// points of a cell plays no part.  A non-finite frame point satisfies the predicate for no s and stays; it is not walked.
__global__ __launch_bounds__(256) void k_cloud_novel(CloudDev cd, const uint8_t* __restrict__ held, const double* __restrict__ pts, int n,
                                                     double merge, uint8_t* __restrict__ keep) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    if (keep[i] == 0) return;
    if (cd.hdr->status != 0 || cd.hdr->n == 0) return;
    const double p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    if (!((p[0] - p[0] == 0.0) && (p[1] - p[1] == 0.0) && (p[2] - p[2] == 0.0))) return;
    const double m2 = merge * merge;
    CloudWalk w;
    cloud_walk_begin(cd, true, p, merge, w);
    while (cloud_walk_next(cd, w)) {
        const unsigned s = w.cur++;
        if (held != nullptr && held[cd.idx[s]] == 0) continue;
        const double dx = p[0] - cd.pts[3 * (size_t)s], dy = p[1] - cd.pts[3 * (size_t)s + 1], dz = p[2] - cd.pts[3 * (size_t)s + 2];
        if (((dx * dx + dy * dy) + dz * dz) < m2) { keep[i] = 0; return; }
    }
}

// ---- fused frames: append (nbk_frame_cloud_append) -------------------------------------------------------------------------------------
// F: the free slots of the store (store_keep == 0), A: the new points kept (keep != 0), both ascending; the k-th of A goes to the k-th
// of F.  Ranks come from a two-level scan, never from atomics: k_cloud_append_count (per-256 block counts of F, then of A, one list) |
// nbk.hip's k_scan over that list | k_cloud_append_slots (slot[k] = F[k] for k < N, into the workspace) | k_cloud_append_write.  The
// store is written by the last kernel alone, after both lists' ranks are complete.

// the rank of this thread among the threads of its 256-thread workgroup whose flag is set (by ballot and the four waves' totals),
// and their number; every thread of the workgroup calls it, once per kernel
NBK_DEV unsigned cloud_block_rank(bool flag, unsigned& total) {
    __shared__ unsigned wave_sum[4];
    const unsigned long long b = __ballot(flag);
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    if (lane == 0) wave_sum[wv] = (unsigned)__popcll(b);
    __syncthreads();
    unsigned base = 0u;
    total = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned v = wave_sum[k];
        if (k < wv) base += v;
        total += v;
    }
    return base + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
}

// blocks 0 .. bf - 1: the free slots of their 256 store slots; blocks bf .. bf + ba - 1: the kept ones of their 256 new points
__global__ __launch_bounds__(256) void k_cloud_append_count(const uint8_t* __restrict__ store_keep, int m, const uint8_t* __restrict__ keep,
                                                            int n, int bf, unsigned long long* __restrict__ cnt) {
    const int b = (int)blockIdx.x;
    bool flag;
    if (b < bf) {
        const int j = b * 256 + (int)threadIdx.x;
        flag = j < m && store_keep[j] == 0;
    } else {
        const int i = (b - bf) * 256 + (int)threadIdx.x;
        flag = i < n && keep[i] != 0;
    }
    unsigned total;
    (void)cloud_block_rank(flag, total);
    if (threadIdx.x == 0) cnt[b] = total;
}

// one block per 256 store slots: free slot j of rank k < n -> slot[k] = j
__global__ __launch_bounds__(256) void k_cloud_append_slots(const uint8_t* __restrict__ store_keep, int m, int n,
                                                            const unsigned long long* __restrict__ offs, int* __restrict__ slot) {
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    const bool flag = j < m && store_keep[j] == 0;
    unsigned total;
    const unsigned long long k = offs[blockIdx.x] + cloud_block_rank(flag, total);
    if (flag && k < (unsigned long long)n) slot[k] = j;
}

// one block per 256 new points (one block at least: it writes the counts): the kept point i of rank k < |F| moves to slot[k]
__global__ __launch_bounds__(256) void k_cloud_append_write(const double* __restrict__ new_pts, const uint8_t* __restrict__ keep, int n, int m,
                                                            int bf, int ba, const unsigned long long* __restrict__ offs,
                                                            const int* __restrict__ slot, double* __restrict__ store_pts,
                                                            uint8_t* __restrict__ store_keep, int* __restrict__ slot_of,
                                                            long long* __restrict__ counts) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    const bool flag = i < n && keep[i] != 0;
    const unsigned long long n_free = offs[bf], n_new = offs[bf + ba] - n_free;
    const unsigned long long appended = n_free < n_new ? n_free : n_new;
    unsigned total;
    const unsigned r = cloud_block_rank(flag, total);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counts[0] = (long long)((unsigned long long)m - n_free + appended);
        counts[1] = (long long)appended;
        counts[2] = (long long)(n_new - appended);
    }
    if (i >= n) return;
    int to = -1;
    if (flag) {
        const unsigned long long k = (offs[bf + (int)blockIdx.x] - n_free) + r;
        if (k < appended) {
            to = slot[k];
            store_pts[3 * (size_t)to] = new_pts[3 * (size_t)i];
            store_pts[3 * (size_t)to + 1] = new_pts[3 * (size_t)i + 1];
            store_pts[3 * (size_t)to + 2] = new_pts[3 * (size_t)i + 2];
            store_keep[to] = 1;
        }
    }
    if (slot_of != nullptr) slot_of[i] = to;
}

// the lane's q row into its LDS row (eight loads in flight, as k_pair_items stages it); returns whether every value is finite
NBK_DEV bool cloud_stage_q(const double* __restrict__ q, int64_t b, int nq, double* myq) {
    const double* qrow = q + b * nq;
    const int nq1 = nq - 1;
    bool fin = true;
    for (int j0 = 0; j0 < nq; j0 += 8) {
        double qv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int j = (j0 + u) < nq1 ? (j0 + u) : nq1; qv[u] = qrow[j]; }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (j0 + u <= nq1) { myq[j0 + u] = qv[u]; fin = fin && (qv[u] - qv[u] == 0.0); }
    }
    return fin;
}

// frame of robot shape s (device order) for the lane's q: the joints of the shape's mask, base first
NBK_DEV void cloud_shape_frame(const DevModel& m, int s, const double* myq, Xf& T) {
    const unsigned mask = m.rs_mask[s];
    xf_from12(m.base_pose, T);
    for (int k = 0; k < m.n_joints; ++k) {
        if (((mask >> k) & 1u) == 0u) continue;
        Xf nxt;
        joint_apply(m, k, T, myq[m.joint_qidx[k]], nxt);
        T = nxt;
    }
}

NBK_DEV void cloud_core_init(Core& A) {
    A.kind = K_POINT;
#pragma unroll
    for (int e = 0; e < 3; ++e) { A.c[e] = 0.0; A.h[e] = 0.0; A.ax[0][e] = A.ax[1][e] = A.ax[2][e] = 0.0; }
    A.rad = A.margin = A.rho = 0.0;
}
// the core of a sphere world shape of radius r with identity rotation: a point core with margin r
NBK_DEV void cloud_point_core(double r, Core& P) {
    cloud_core_init(P);
    P.ax[0][0] = 1.0; P.ax[1][1] = 1.0; P.ax[2][2] = 1.0;
    P.margin = r;
}

// the owner of flat sample f < offs[n]: the largest e in [0, n) with offs[e] <= f (owners without samples fall out by themselves:
// equal offsets); f is sample f - offs[e] of it
NBK_DEV int64_t cloud_flat_owner(const unsigned long long* __restrict__ offs, int64_t n, unsigned long long f) {
    int64_t e = 0, hi = n;                               // offs[e] <= f < offs[hi]
    while (hi - e > 1) {
        const int64_t mid = e + ((hi - e) >> 1);
        if (offs[mid] <= f) e = mid; else hi = mid;
    }
    return e;
}

// ---- validity -----------------------------------------------------------------------------------------------------------------
// The pair predicate for (point core P, shape core A), canonical order (the point first).  cores_collide_exact as it is, except that a
// hull core at tc <= 0 skips that routine's device-only cull: hull_box_far compares the point's distance from the hull's local box
// with max(tc, 0) + the point's bounding radius = 0 and answers "free" for EVERY point there, also one inside the box (its sibling
// box_far_negative asks for d2 > 0).  For a point against a hull cores_collide_pre decides nothing else, and the predicate ends in
// the distance iteration either way: call it directly.
NBK_DEV bool cloud_collides(const Core& P, const Core& A, double tc) {
    if (A.kind == K_HULL && !(tc > 0.0)) return gjk_collides(P, A, tc);
    return cores_collide_exact(P, A, tc);
}

// The walk: does the lane's staged row `myq` touch the cloud?  OR over the selected shapes s and the points i of the pair predicate
// for (s, sphere of the cloud's radius at p_i): tc = (thr + margin_s) + radius; bounding spheres |cA - p|^2 >= ((tc + rhoA) + 0)^2 or a
// non-positive sum => free; else the exact test with the cores in canonical order (cloud_collides; the point first: a point-point pair
// computes the same bits either way).  Called by every lane of the wave (`active`: this lane has a row; `hit`: its verdict so far,
// raised here -- a lane that comes in with a hit, or without a row, only keeps the ballots company); the caller has checked that
// the cloud holds points and that its status is clear.
NBK_DEV void cloud_row_hits(const DevModel& m, const CloudDev& cd, const CloudSel& sel, double radius, double thr, const double* myq,
                            bool active, bool& hit) {
    Core P;
    cloud_point_core(radius, P);
    Xf T;
    int cur_frame = -2;
    for (int s = 0; s < m.n_rshapes; ++s) {
        if (!cloud_selected(sel, s)) continue;
        const bool work = active && !hit;
        if (__builtin_amdgcn_ballot_w64(work) == 0ull) break;
        Core A;
        cloud_core_init(A);
        double tc = 0.0, rs = 0.0;
        if (work) {
            // (a lane that drops out keeps a stale frame and never comes back)
            if (m.rs_frame[s] != cur_frame) cloud_shape_frame(m, s, myq, T);
            build_core(m, s, T, A);
            if (A.kind == K_HULL) A.rad = -1.0;          // every working lane holds this hull: its vertices go through the scalar cache
            tc = (thr + A.margin) + radius;
            rs = (tc + A.rho) + 0.0;
        }
        cur_frame = m.rs_frame[s];
        CloudWalk w;
        cloud_walk_begin(cd, work, A.c, rs, w);
        const double rs2 = rs * rs;
        while (true) {
            // each lane runs ahead to its next point that passes the bounding spheres (a short loop: three loads, one
            // comparison), then the lanes that hold one decide theirs side by side: the exact test is the long part, and inline
            // in the walk it would run for one lane's candidate at a time
            bool cand = false;
            while (!hit && !cand && cloud_walk_next(cd, w)) {
                const double* p = cd.pts + 3 * (size_t)w.cur;
                ++w.cur;
                P.c[0] = p[0]; P.c[1] = p[1]; P.c[2] = p[2];
                double dc[3];
                sub3(A.c, P.c, dc);
                cand = dot3(dc, dc) < rs2;
            }
            if (__builtin_amdgcn_ballot_w64(cand) == 0ull) break;
            if (cand && cloud_collides(P, A, tc)) hit = true;
        }
    }
}

// verdict of row b = the walk's, or 1 for a non-finite row or a set status.  A workgroup owns one mask word, so the word and the
// bytes have one writer each.
__global__ __launch_bounds__(64) void k_cloud_validity(DevModel m, CloudDev cd, CloudSel sel, const double* __restrict__ q, int64_t B,
                                                       double thr, int accumulate, unsigned long long* __restrict__ mask_bits,
                                                       uint8_t* __restrict__ mask_bytes) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * WAVE + lane;
    const bool active = b < B;
    double* myq = lds + lane * m.n_q;
    const int status = cd.hdr->status;
    const int n = cd.hdr->n;
    const double radius = cd.hdr->radius;
    bool hit = false;
    if (active) hit = !cloud_stage_q(q, b, m.n_q, myq) || status != 0;
    if (n > 0 && status == 0) cloud_row_hits(m, cd, sel, radius, thr, myq, active, hit);
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

// ---- the robot's own image in a frame (nbk_frame_cloud_self_filter) ----------------------------------------------------------------------
// k_cloud_validity with the roles of the batch swapped: ONE configuration q0 and many points.  keep[i] goes from 1 to 0 iff, for some
// selected shape s, the query predicate holds for (s, sphere of `radius` at p_i) with thr = padding -- cloud_row_hits' statements
// in cloud_row_hits' operand order: tc = (padding + margin_s) + radius; rs = (tc + rho_s) + 0, free unless rs > 0 and
// |c_s - p|^2 < rs^2; then cloud_collides(P, A, tc), the point first.  So a cloud of the points kept reads free at (q0, padding).
//   preamble  one selected shape per lane (a stride of 256 over the shapes): the shape's frame at q0 (cloud_shape_frame: q0 is read
//             from global memory, every lane the same addresses), build_core, the record into LDS (SelfFilterLds).  Divergent, and
//             once per workgroup: the grid is bounded so that a workgroup serves many points
//   loop      256 points per trip, a stride of the grid over the points.  Two stages, as in cloud_row_hits: each lane runs ahead
//             over the records to its next shape that passes the bounding spheres (while the lanes agree on the record this is an
//             LDS broadcast: four doubles), then the lanes that hold a candidate decide theirs side by side under one ballot.  The
//             candidates of a trip may be DIFFERENT shapes: the hull support's scalar-cache path (rad < 0: every working lane
//             holds that hull) is taken only when the ballot shows one shape, as k_cloud_records' second phase has it; the bits
//             are the same either way.
// A non-finite q0 removes nothing; a non-finite point never passes the bounding spheres and stays as it came.
__global__ __launch_bounds__(256) void k_cloud_self_filter(DevModel m, CloudSel sel, int n_sel, const double* __restrict__ q0,
                                                           const double* __restrict__ pts, int n, double radius, double padding,
                                                           uint8_t* __restrict__ keep) {
    extern __shared__ double lds[];
    static_assert(sizeof(Core) == sizeof(double) * SelfFilterLds::CORE_LEN, "SelfFilterLds holds a Core per record");
    const int tid = (int)threadIdx.x;
    double* const rec = SelfFilterLds(0).rec(lds);
    for (int c = 0; c < m.n_q; ++c)
        if (!(q0[c] - q0[c] == 0.0)) return;                 // (every thread reads the same row: the whole grid leaves)
    // the records, in device order: record k is the k-th selected shape (a selection has at most 256 shapes: four words)
    for (int s = tid; s < m.n_rshapes; s += 256) {
        if (!cloud_selected(sel, s)) continue;
        int k = s;
        if (sel.all == 0) {
            k = __builtin_popcountll(sel.w[(s >> 6) & 3] & ((1ull << (s & 63)) - 1ull));
            for (int w = 0; w < ((s >> 6) & 3); ++w) k += __builtin_popcountll(sel.w[w]);
        }
        Xf T;
        cloud_shape_frame(m, s, q0, T);
        Core A;
        cloud_core_init(A);
        build_core(m, s, T, A);
        const double tc = (padding + A.margin) + radius;
        const double rs = (tc + A.rho) + 0.0;
        double* r = rec + (size_t)k * SelfFilterLds::REC_LEN;
        *reinterpret_cast<Core*>(r) = A;
        r[SelfFilterLds::TC_AT] = tc;
        r[SelfFilterLds::RS2_AT] = rs > 0.0 ? rs * rs : -1.0;      // (a sum that is not positive: free, as the empty cell range of the queries)
    }
    __syncthreads();
    Core P;
    cloud_point_core(radius, P);
    for (int64_t base = (int64_t)blockIdx.x * 256; base < (int64_t)n; base += (int64_t)gridDim.x * 256) {
        const int64_t i = base + tid;
        const bool live = i < (int64_t)n && keep[i] != 0;
        if (live) { P.c[0] = pts[3 * i]; P.c[1] = pts[3 * i + 1]; P.c[2] = pts[3 * i + 2]; }
        bool hit = false;
        int k = 0;
        while (true) {
            bool cand = false;
            int kc = 0;
            while (live && !hit && !cand && k < n_sel) {
                const double* r = rec + (size_t)k * SelfFilterLds::REC_LEN;
                double dc[3];
                sub3(reinterpret_cast<const Core*>(r)->c, P.c, dc);
                cand = dot3(dc, dc) < r[SelfFilterLds::RS2_AT];
                kc = k++;
            }
            const unsigned long long cm = __builtin_amdgcn_ballot_w64(cand);
            if (cm == 0ull) break;
            const int k0 = __shfl(kc, __builtin_ctzll(cm));
            const bool uniform = __builtin_amdgcn_ballot_w64(cand && kc != k0) == 0ull;
            if (cand) {
                const double* r = rec + (size_t)kc * SelfFilterLds::REC_LEN;
                Core A = *reinterpret_cast<const Core*>(r);
                if (uniform && A.kind == K_HULL) A.rad = -1.0;
                if (cloud_collides(P, A, r[SelfFilterLds::TC_AT])) hit = true;
            }
        }
        if (hit) keep[i] = 0;
    }
}

// ---- rendered frames (nbk_render_depth_batch; DESIGN.md 3, "Rendered frames") ----------------------------------------------------------
// Depth frames of the device scene -- the selected robot shapes at the frame's q and, when asked for, the world shapes -- ray-cast
// by sphere tracing on cores_distance: the surface is the set the collision predicates call "distance 0".  One pixel per lane, a wave
// is an 8x8 tile, a workgroup a 16x16 block of one frame; the grid is blocks x B frames, flat.
//   preamble   as k_cloud_self_filter: one selected robot shape per lane (stride 256), its frame at the frame's q row, build_core,
//              the record and the widened radius of its bounding ball into LDS (RenderLds).  World cores are read from m.ws_core.
//   drawn order  the selected robot shapes in device order, then the world shapes: index i < n_sel is record i, else world i - n_sel.
//              Candidates are met in this order everywhere, so "ties go to the smaller index" means this order.
//   tile cull  the lanes test the drawn shapes (stride 64; planes never enter) against a cone around the tile's rays and compact the
//              survivors, ascending, into the wave's LDS list with one ballot per trip; then, per survivor, every lane takes its OWN
//              span (depth_ray_sphere_span with the widened ball) and the ballot of the lanes that have one is kept beside it.  The
//              cone only shortens the second loop: a lane's candidates are the shapes whose span ITS ray has, whatever the tile.
//   planes     closed form, per lane: h = n.(p(z_near) - c); h < eps: hit at z_near; else with den = n.w (w: the ray per unit depth in
//              the world) < 0 the hit is z_near + h / -den when that is <= z_far.  The nearest plane competes with the march.
//   march      z starts at the lane's smallest z0 and ends past its largest z1 (or the plane hit, or z_far).  A step takes d, the
//              minimum over the lane's candidates in order of cores_distance<false, true>(shape, point core at p(z)); a candidate
//              whose bounding-ball lower bound |c - p| - R is not below the running minimum is skipped.  d < eps: hit at this z,
//              labelled with the shape of the minimum (the first that reaches it); else z += d / L.  max_steps steps without a
//              decision: unresolved.  A march hit at the plane's depth or nearer wins.  The lanes run ahead to their next candidate
//              and decide side by side under one ballot; the hull support's scalar path only when the ballot shows one candidate.
// A frame whose q row or pose is not finite, or a set world status (wstatus: the movable descriptor's, else null), is unresolved in
// every pixel.  counts: hit pixels, unresolved pixels, distance evaluations; integer sums, one atomic add per wave and counter.
struct RenderArgs {
    int H, W, bx, by;                 // the image and its 16x16 blocks per row / column
    DepthCam cam;                     // depth_scale 1; z_min, z_max: z_near, z_far
    double eps;
    int max_steps, draw_world, q_one, t_one;
    float miss;
};

NBK_DEV void render_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

NBK_DEV unsigned long long render_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// the widened bounding ball of a core (cloud_search_radius' widening: the iterative distances must not lose a shape to their last digits)
NBK_DEV double render_ball_radius(double rho, double margin) {
    const double R = rho + margin;
    return R + (1e-6 * __builtin_fabs(R) + 1e-7);
}

// the device index of the k-th selected robot shape (record k)
NBK_DEV int render_record_shape(const CloudSel& s, int k) {
    if (s.all != 0) return k;
    for (int w = 0; w < 4; ++w) {
        const int c = __builtin_popcountll(s.w[w]);
        if (k < c) {
            unsigned long long x = s.w[w];
            for (int j = 0; j < k; ++j) x &= x - 1ull;
            return 64 * w + __builtin_ctzll(x);
        }
        k -= c;
    }
    return 0;
}

__global__ __launch_bounds__(256) void k_render_depth(DevModel m, CloudSel sel, int n_sel, const int* __restrict__ rs_user,
                                                      const int* __restrict__ wstatus, const double* __restrict__ q,
                                                      const double* __restrict__ Tp, RenderArgs a, float* __restrict__ depth,
                                                      int* __restrict__ label, unsigned long long* __restrict__ counts) {
    extern __shared__ double lds[];
    static_assert(sizeof(Core) == sizeof(double) * RenderLds::CORE_LEN, "RenderLds holds a Core per record");
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n_world = a.draw_world != 0 ? m.n_wshapes : 0;
    const int n_list = n_sel + n_world;
    const RenderLds L(n_sel, n_list);
    double* const rec = L.rec(lds);
    unsigned long long* const own = L.own(lds) + (size_t)wv * n_list;
    int* const lst = L.idx(lds) + (size_t)wv * n_list;
    const int per = a.bx * a.by;
    const int64_t b = (int64_t)(blockIdx.x / (unsigned)per);
    const int blk = (int)(blockIdx.x % (unsigned)per);
    const int tu0 = (blk % a.bx) * 16 + (wv & 1) * 8, tv0 = (blk / a.bx) * 16 + (wv >> 1) * 8;
    const int u = tu0 + (lane & 7), v = tv0 + (lane >> 3);
    const bool live = u < a.W && v < a.H;
    const int64_t pix = (b * a.H + v) * a.W + u;
    const double* qrow = q + (a.q_one != 0 ? 0 : b * m.n_q);
    const double* Tg = Tp + (a.t_one != 0 ? 0 : b * 12);
    double T[12];
    bool fin = true;
#pragma unroll
    for (int e = 0; e < 12; ++e) { T[e] = Tg[e]; fin = fin && (T[e] - T[e] == 0.0); }
    for (int c = 0; c < m.n_q; ++c) fin = fin && (qrow[c] - qrow[c] == 0.0);
    if (wstatus != nullptr && *wstatus != 0) fin = false;
    if (!fin) {                                              // (every thread of the workgroup reads the same values: all leave)
        if (live) { depth[pix] = a.miss; if (label != nullptr) label[pix] = -2; }
        const unsigned long long nl = (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(live));
        if (counts != nullptr && lane == 0 && nl != 0ull) atomicAdd(counts + 1, nl);
        return;
    }
    // the records, in device order (k_cloud_self_filter's preamble)
    for (int s = tid; s < m.n_rshapes; s += 256) {
        if (!cloud_selected(sel, s)) continue;
        int k = s;
        if (sel.all == 0) {
            k = __builtin_popcountll(sel.w[(s >> 6) & 3] & ((1ull << (s & 63)) - 1ull));
            for (int w = 0; w < ((s >> 6) & 3); ++w) k += __builtin_popcountll(sel.w[w]);
        }
        Xf Ts;
        cloud_shape_frame(m, s, qrow, Ts);
        Core A;
        cloud_core_init(A);
        build_core(m, s, Ts, A);
        double* r = rec + (size_t)k * RenderLds::REC_LEN;
        *reinterpret_cast<Core*>(r) = A;
        r[RenderLds::RB_AT] = render_ball_radius(A.rho, A.margin);
    }
    __syncthreads();
    // the cone around the tile's rays, in the camera frame: axis n through the tile's middle, half angle to its farthest corner ray
    // (the rays of a rectangle of pixels lie inside the cone that holds its corners).  Widened: it must never lose a lane's candidate
    double n[3], cosT = 1.0;
    {
        const double mx = (((double)tu0 + 3.5) - a.cam.cx) / a.cam.fx, my = (((double)tv0 + 3.5) - a.cam.cy) / a.cam.fy;
        const double inv = 1.0 / nbk_sqrt((mx * mx + my * my) + 1.0);
        n[0] = mx * inv; n[1] = my * inv; n[2] = inv;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double ex = ((double)(tu0 + ((k & 1) ? 7 : 0)) - a.cam.cx) / a.cam.fx, ey = ((double)(tv0 + ((k & 2) ? 7 : 0)) - a.cam.cy) / a.cam.fy;
            const double c = ((n[0] * ex + n[1] * ey) + n[2]) / nbk_sqrt((ex * ex + ey * ey) + 1.0);
            cosT = c < cosT ? c : cosT;
        }
        cosT -= 1e-9;
    }
    const double sinT = nbk_sqrt(1.0 - cosT * cosT > 0.0 ? 1.0 - cosT * cosT : 0.0);
    int n_c = 0;                                             // the tile's candidates (wave-uniform)
    for (int i0 = 0; i0 < n_list; i0 += 64) {
        const int i = i0 + lane;
        bool keep = false;
        if (i < n_list) {
            const bool robot = i < n_sel;
            const int w = robot ? 0 : i - n_sel;
            const double* cc = robot ? reinterpret_cast<const Core*>(rec + (size_t)i * RenderLds::REC_LEN)->c : m.ws_core + 18 * (size_t)w;
            if (robot || m.ws_kind[w] != K_PLANE) {
                const double R = robot ? rec[(size_t)i * RenderLds::REC_LEN + RenderLds::RB_AT] : render_ball_radius(cc[17], cc[16]);
                const double d0 = cc[0] - T[3], d1 = cc[1] - T[7], d2 = cc[2] - T[11];
                const double xc = (T[0] * d0 + T[4] * d1) + T[8] * d2, yc = (T[1] * d0 + T[5] * d1) + T[9] * d2, zc = (T[2] * d0 + T[6] * d1) + T[10] * d2;
                const double t = (xc * n[0] + yc * n[1]) + zc * n[2], len2 = (xc * xc + yc * yc) + zc * zc;
                const double perp2 = len2 - t * t;
                const double perp = nbk_sqrt(perp2 > 0.0 ? perp2 : 0.0);
                keep = perp * cosT - t * sinT <= R + 1e-9 * (1.0 + nbk_sqrt(len2));
            }
        }
        const unsigned long long km = __builtin_amdgcn_ballot_w64(keep);
        if (keep) lst[n_c + __popcll(km & ((1ull << lane) - 1ull))] = i;
        n_c += __popcll(km);
    }
    render_wave_sync();
    // every lane's own spans over the tile's candidates; a candidate no lane of the tile has is dropped (the ballot is the wave's)
    double zs = NBK_INF, ze = -NBK_INF;
    int n_o = 0;
    for (int e = 0; e < n_c; ++e) {
        const int i = lst[e];
        const bool robot = i < n_sel;
        const double* cc = robot ? reinterpret_cast<const Core*>(rec + (size_t)i * RenderLds::REC_LEN)->c : m.ws_core + 18 * (size_t)(robot ? 0 : i - n_sel);
        const double R = robot ? rec[(size_t)i * RenderLds::REC_LEN + RenderLds::RB_AT] : render_ball_radius(cc[17], cc[16]);
        const double c3[3] = {cc[0], cc[1], cc[2]};
        double z0 = 0.0, z1 = 0.0;
        const bool has = live && depth_ray_sphere_span(a.cam, T, u, v, c3, R, a.cam.z_min, a.cam.z_max, &z0, &z1);
        if (has) { zs = z0 < zs ? z0 : zs; ze = z1 > ze ? z1 : ze; }
        const unsigned long long hm = __builtin_amdgcn_ballot_w64(has);
        if (hm != 0ull) {                                    // (n_o <= e, and every lane holds lst[e] already: the ballot needed it)
            if (lane == 0) { lst[n_o] = i; own[n_o] = hm; }
            ++n_o;
        }
    }
    render_wave_sync();
    const double Lr = depth_ray_length(a.cam, u, v);
    // planes
    double zp = NBK_INF;
    int lp = -1;
    if (live) {
        double p0[3], wdir[3];
        depth_ray_point(a.cam, T, u, v, a.cam.z_min, p0);
        const double ax = ((double)u - a.cam.cx) / a.cam.fx, ay = ((double)v - a.cam.cy) / a.cam.fy;
#pragma unroll
        for (int e = 0; e < 3; ++e) wdir[e] = (T[4 * e] * ax + T[4 * e + 1] * ay) + T[4 * e + 2];
        for (int w = 0; w < n_world; ++w) {
            if (m.ws_kind[w] != K_PLANE) continue;
            const double* wc = m.ws_core + 18 * (size_t)w;
            const double nn[3] = {wc[9], wc[10], wc[11]};
            const double dd[3] = {p0[0] - wc[0], p0[1] - wc[1], p0[2] - wc[2]};
            const double h = dot3(dd, nn), den = dot3(wdir, nn);
            double z = NBK_INF;
            if (h < a.eps) z = a.cam.z_min;
            else if (den < 0.0) z = a.cam.z_min + h / -den;
            if (z <= a.cam.z_max && z < zp) { zp = z; lp = n_sel + w; }
        }
    }
    // the march
    Core P;
    cloud_point_core(0.0, P);
    double z = zs;
    const double zend = ze < zp ? ze : zp;
    int state = (live && zs <= zend) ? 0 : 2;                // 0 marching, 1 hit, 2 miss
    int lab = -1;
    unsigned long long evals = 0ull;
    for (int step = 0; step < a.max_steps; ++step) {
        if (__builtin_amdgcn_ballot_w64(state == 0) == 0ull) break;
        if (state == 0) depth_ray_point(a.cam, T, u, v, z, P.c);
        double d = NBK_INF;
        int arg = -1, e = 0;
        while (true) {
            bool cand = false;
            int ec = 0;
            while (state == 0 && !cand && e < n_o) {
                ec = e++;
                if (((own[ec] >> lane) & 1ull) == 0ull) continue;
                const int i = lst[ec];
                const bool robot = i < n_sel;
                const double* cc = robot ? reinterpret_cast<const Core*>(rec + (size_t)i * RenderLds::REC_LEN)->c : m.ws_core + 18 * (size_t)(robot ? 0 : i - n_sel);
                const double R = robot ? rec[(size_t)i * RenderLds::REC_LEN + RenderLds::RB_AT] : render_ball_radius(cc[17], cc[16]);
                const double dc[3] = {cc[0] - P.c[0], cc[1] - P.c[1], cc[2] - P.c[2]};
                cand = nbk_sqrt(dot3(dc, dc)) - R < d;
            }
            const unsigned long long cm = __builtin_amdgcn_ballot_w64(cand);
            if (cm == 0ull) break;
            const int e0 = __shfl(ec, __builtin_ctzll(cm));
            const bool uniform = __builtin_amdgcn_ballot_w64(cand && ec != e0) == 0ull;
            if (cand) {
                const int i = lst[ec];
                Core A;
                if (i < n_sel) A = *reinterpret_cast<const Core*>(rec + (size_t)i * RenderLds::REC_LEN);
                else { cloud_core_init(A); load_wcore(m, i - n_sel, A); }
                if (uniform && A.kind == K_HULL) A.rad = -1.0;
                double fam = -1.0;
                const double de = cores_distance<false, true>(A, P, nullptr, &fam);
                ++evals;
                if (de < d) { d = de; arg = i; }
            }
        }
        if (state == 0) {
            if (d < a.eps) { state = 1; lab = arg; }
            else {
                z += d / Lr;
                if (!(z <= zend)) state = 2;
            }
        }
    }
    const bool unres = live && state == 0;
    bool hit = state == 1;
    if (live && !unres && !hit && lp >= 0) { hit = true; z = zp; lab = lp; }
    if (live) {
        depth[pix] = hit ? (float)z : a.miss;
        if (label != nullptr) label[pix] = unres ? -2 : (!hit ? -1 : (lab < n_sel ? rs_user[render_record_shape(sel, lab)] : m.n_rshapes + (lab - n_sel)));
    }
    if (counts != nullptr) {
        const unsigned long long nh = (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(live && hit));
        const unsigned long long nu = (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(unres));
        const unsigned long long ne = render_wave_sum(evals);
        if (lane == 0) {
            if (nh != 0ull) atomicAdd(counts, nh);
            if (nu != 0ull) atomicAdd(counts + 1, nu);
            if (ne != 0ull) atomicAdd(counts + 2, ne);
        }
    }
}

// ---- sampled edges against the cloud (nbk_edge_cloud_validity_batch) -----------------------------------------------------------
// valid[e] before the walk: an edge without samples (the degenerate edge) is invalid; accumulating, an entry only ever goes down.
// An edge of 2^32 samples or more (its sample index no longer fits the packed (edge, sample) word of edge_t) is invalid as well.
__global__ __launch_bounds__(256) void k_cloud_edges_init(const unsigned long long* __restrict__ cnt, int64_t E, int accumulate,
                                                          uint8_t* __restrict__ valid) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const bool ok = cnt[e] != 0ull && cnt[e] <= 0xffffffffull;
    valid[e] = (ok && (!accumulate || valid[e] != 0)) ? 1 : 0;
}

// One sample per lane, FLAT across the edges: sample f of [0, total) belongs to the largest edge e with offs[e] <= f (edges without
// samples fall out by themselves) and is sample f - offs[e] of it, by the expression of the validity kernels (edge_sample_row).  The
// grid covers the static bound edge_capacity; a workgroup strides over 64-sample blocks until `total` (read here, never by the host),
// so a batch longer than the bound is served all the same.  valid[e] is an AND: a lane whose edge already reads 0 skips its sample,
// a lane that finds a hit (or a non-finite sample, or a set status) stores 0 -- several lanes may store the same 0, in any order.
__global__ __launch_bounds__(64) void k_cloud_edges(DevModel m, CloudDev cd, CloudSel sel, EdgeSrc es,
                                                    const unsigned long long* __restrict__ offs, int64_t E, double thr, uint8_t* valid) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    double* myq = lds + lane * m.n_q;
    const unsigned long long total = offs[E];
    const int status = cd.hdr->status;
    const int n = cd.hdr->n;
    const double radius = cd.hdr->radius;
    for (unsigned long long base = (unsigned long long)blockIdx.x * WAVE; base < total; base += (unsigned long long)gridDim.x * WAVE) {
        const unsigned long long f = base + (unsigned long long)lane;
        int64_t e = 0;
        bool work = false;
        if (f < total) {
            e = cloud_flat_owner(offs, E, f);
            if (__hip_atomic_load(valid + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                edge_sample_row(es, ((unsigned long long)e << 32) | (f - offs[e]), m.n_q, myq, 1);
                work = !row_nonfinite(myq, m.n_q, 1) && status == 0;
                if (!work) __hip_atomic_store(valid + e, (uint8_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        bool hit = false;
        if (n > 0 && status == 0) cloud_row_hits(m, cd, sel, radius, thr, myq, work, hit);
        if (hit) __hip_atomic_store(valid + e, (uint8_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- clearance ----------------------------------------------------------------------------------------------------------------
// per row the minimum over the selected (s, i) of the signed distance (cores_distance, EPA's depth where a point lies inside a hull
// core), reported when it is < d_max with the shape (caller's index) and the original point index; ties go to the smallest shape, then
// to the smallest point index, whatever order the walk meets them in.  d >= |cA - p| - rhoA - margin_s - radius, so only points with
// |cA - p| < ((D + margin_s) + radius) + rhoA can reach below D: the walk covers that ball for D = d_max, and the running best shrinks
// the ball a candidate must lie in before its distance is evaluated.  Both radii are widened by 1e-6 relative + 1e-7: the bound holds
// for exact distances, and the iterative ones (GJK to 1e-10, EPA to 1e-8 relative) must not lose a point to their last digits.
NBK_DEV double cloud_search_radius(double D, const Core& A, double radius) {
    const double R = ((D + A.margin) + radius) + A.rho;
    return R + (1e-6 * __builtin_fabs(R) + 1e-7);
}

// The per-shape body of the clearance (k_cloud_clearance, CloudEdgeLane): core A of the robot shape with the caller's index su, built
// by the caller (`ok`: this lane holds one), against every point of the cloud; best / bs / bi come in as the row's running minimum
// and go out lowered.  Called by every lane of the wave.  bslot (optional; k_cloud_records): where a point that lowers the minimum
// stands in the SORTED arrays -- cd.idx maps sorted to original only, and the record needs the winner's coordinates again.
NBK_DEV void cloud_core_clearance(const CloudDev& cd, const Core& A, Core& P, double radius, bool ok, int su, double d_max,
                                  double& best, int& bs, int& bi, unsigned* bslot = nullptr) {
    double R = ok ? cloud_search_radius(best < d_max ? best : d_max, A, radius) : 0.0;
    CloudWalk w;
    cloud_walk_begin(cd, ok, A.c, R, w);
    double R2 = R * R;
    while (true) {
        // as in k_cloud_validity: run ahead to the next point inside the current ball, then evaluate side by side
        bool cand = false;
        int oi = -1;
        while (!cand && R > 0.0 && cloud_walk_next(cd, w)) {
            const double* p = cd.pts + 3 * (size_t)w.cur;
            oi = cd.idx[w.cur];
            ++w.cur;
            P.c[0] = p[0]; P.c[1] = p[1]; P.c[2] = p[2];
            double dc[3];
            sub3(A.c, P.c, dc);
            cand = dot3(dc, dc) < R2;
        }
        if (__builtin_amdgcn_ballot_w64(cand) == 0ull) break;
        if (cand) {
            double fam = -1.0;
            double d = cores_distance<false, true>(A, P, nullptr, &fam);
            if (fam >= 0.0) epa_refine<false>(A, P, fam, d, nullptr);
            if (d < d_max && (d < best || (d == best && (su < bs || (su == bs && oi < bi))))) {
                best = d; bs = su; bi = oi;
                if (bslot != nullptr) *bslot = w.cur - 1u;       // (the run-ahead loop stops behind its candidate)
                R = cloud_search_radius(best, A, radius);
                R2 = R * R;
            }
        }
    }
}

__global__ __launch_bounds__(64) void k_cloud_clearance(DevModel m, CloudDev cd, CloudSel sel, const int* __restrict__ rs_user,
                                                        const double* __restrict__ q, int64_t B, double d_max,
                                                        double* __restrict__ out_d, int32_t* __restrict__ out_s, int32_t* __restrict__ out_p) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * WAVE + lane;
    const bool active = b < B;
    double* myq = lds + lane * m.n_q;
    const int status = cd.hdr->status;
    const int n = cd.hdr->n;
    const double radius = cd.hdr->radius;
    bool ok = false;
    if (active) ok = cloud_stage_q(q, b, m.n_q, myq) && status == 0;
    double best = NBK_INF;
    int bs = -1, bi = -1;
    if (n > 0 && status == 0 && __builtin_amdgcn_ballot_w64(ok) != 0ull) {
        Core P;
        cloud_point_core(radius, P);
        Xf T;
        int cur_frame = -2;
        for (int s = 0; s < m.n_rshapes; ++s) {
            if (!cloud_selected(sel, s)) continue;
            Core A;
            cloud_core_init(A);
            if (ok) {
                if (m.rs_frame[s] != cur_frame) cloud_shape_frame(m, s, myq, T);
                build_core(m, s, T, A);
                if (A.kind == K_HULL) A.rad = -1.0;
            }
            cur_frame = m.rs_frame[s];
            cloud_core_clearance(cd, A, P, radius, ok, rs_user[s], d_max, best, bs, bi);
        }
    }
    if (active) {
        out_d[b] = ok ? best : __builtin_nan("");
        if (out_s != nullptr) out_s[b] = ok ? bs : -1;
        if (out_p != nullptr) out_p[b] = ok ? bi : -1;
    }
}

// ---- proximity records (nbk_records_cloud_batch) -----------------------------------------------------------------------------------
// The clearance's winner with its witness and gradient row, one configuration per lane, in two phases.
//   1. the winner: cloud_core_clearance as k_cloud_clearance calls it, which also keeps the winner's slot in the sorted arrays and
//      (here) the device index of its shape.  PER_SHAPE = false runs k_cloud_clearance's shape loop; PER_SHAPE = true has the grid
//      (ceil(B / 64), selected shapes) of k_cloud_edge_ca -- a wave holds ONE shape, every item starts from a fresh `best` -- and
//      writes column `col` of [B][n_sel]: the rank of the shape's caller's index among the selected ones.
//   2. the record, for the lanes that hold a winner and only when a witness or a row is asked for: the winner shape's joint chain
//      once more (the joint_apply sequence of cloud_shape_frame, so the same frame bits), with joint_frame_rows into the
//      [J][6][64] LDS rows when rows are asked for; build_core; cores_distance<true, true> and epa_refine<true> on (shape core,
//      point core) -- item_distance's statements for a (robot shape, sphere world shape) pair; prox_row_masks with the shape's mask
//      and 0.  The hull's scalar-cache path only where every lane with a winner holds the same shape.  The distance this phase
//      finds is the one reported where it runs: the bits of phase 1, as tests/test_gpu_cloud_records.py checks against both.
// Nothing nearer than d_max: +inf, -1, -1, NaN witness, a row of +0.0 (the gradient of a hinge cost).  A non-finite configuration
// or a set status: NaN, -1, -1, NaN, NaN.  LDS: PairItemsLds -- [64][n_q] q rows | [J][6][64] joint rows when rows are asked for.
template <bool PER_SHAPE>
__global__ __launch_bounds__(64) void k_cloud_records(DevModel m, CloudDev cd, CloudSel sel, const int* __restrict__ rs_user,
                                                      const double* __restrict__ q, int64_t B, double d_max, int n_sel,
                                                      double* __restrict__ out_d, int32_t* __restrict__ out_s, int32_t* __restrict__ out_p,
                                                      double* __restrict__ out_w, double* __restrict__ out_j) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * WAVE + lane;
    const bool active = b < B;
    const PairItemsLds L(m.n_q);
    double* myq = L.q(lds) + lane * m.n_q;
    double* lds_jz = out_j != nullptr ? L.jz(lds) : nullptr;
    // per shape: the blockIdx.y-th selected shape, device order, and its column
    int only = -1, col = 0;
    if constexpr (PER_SHAPE) {
        for (int i = 0, k = 0; i < m.n_rshapes; ++i) {
            if (!cloud_selected(sel, i)) continue;
            if (k == (int)blockIdx.y) { only = i; break; }
            ++k;
        }
        if (only < 0) return;
        for (int i = 0; i < m.n_rshapes; ++i)
            if (cloud_selected(sel, i) && rs_user[i] < rs_user[only]) ++col;
    }
    const int status = cd.hdr->status;
    const int n = cd.hdr->n;
    const double radius = cd.hdr->radius;
    bool ok = false;
    if (active) ok = cloud_stage_q(q, b, m.n_q, myq) && status == 0;
    double best = NBK_INF;
    int bs = -1, bi = -1, bdev = 0;
    unsigned slot = 0u;
    Core P;
    cloud_point_core(radius, P);
    if (n > 0 && status == 0 && __builtin_amdgcn_ballot_w64(ok) != 0ull) {
        Xf T;
        int cur_frame = -2;
        for (int s = PER_SHAPE ? only : 0; s < (PER_SHAPE ? only + 1 : m.n_rshapes); ++s) {
            if (!cloud_selected(sel, s)) continue;
            Core A;
            cloud_core_init(A);
            if (ok) {
                if (m.rs_frame[s] != cur_frame) cloud_shape_frame(m, s, myq, T);
                build_core(m, s, T, A);
                if (A.kind == K_HULL) A.rad = -1.0;
            }
            cur_frame = m.rs_frame[s];
            cloud_core_clearance(cd, A, P, radius, ok, rs_user[s], d_max, best, bs, bi, &slot);
            if (bs == rs_user[s]) bdev = s;              // (a caller's index names one shape: bs equals it only once set here)
        }
    }
    const bool win = ok && bs >= 0;
    double wit[9];
    if ((out_w != nullptr || out_j != nullptr) && __builtin_amdgcn_ballot_w64(win) != 0ull) {
        const unsigned mask = win ? m.rs_mask[bdev] : 0u;
        Xf T;
        xf_from12(m.base_pose, T);
        for (int k = 0; k < m.n_joints; ++k) {
            if (((mask >> k) & 1u) == 0u) continue;
            Xf nxt;
            joint_apply(m, k, T, myq[m.joint_qidx[k]], nxt);
            if (lds_jz != nullptr) joint_frame_rows(m, k, nxt, lds_jz + 6 * k * WAVE + lane);
            T = nxt;
        }
        // the hull support's scalar-cache path (rad < 0) needs every working lane to hold the same hull, as item_distance has it
        const unsigned long long wm = __builtin_amdgcn_ballot_w64(win);
        const int s0 = __shfl(bdev, __builtin_ctzll(wm));
        const bool uniform = __builtin_amdgcn_ballot_w64(win && bdev != s0) == 0ull;
        if (win) {
            Core A;
            cloud_core_init(A);
            build_core(m, bdev, T, A);
            if (uniform && A.kind == K_HULL) A.rad = -1.0;
            const double* p = cd.pts + 3 * (size_t)slot;
            P.c[0] = p[0]; P.c[1] = p[1]; P.c[2] = p[2];
            double fam = -1.0;
            double d = cores_distance<true, true>(A, P, wit, &fam);
            if (fam >= 0.0) epa_refine<true>(A, P, fam, d, wit);
            best = d;
        }
    }
    if (!active) return;
    const int64_t o = PER_SHAPE ? b * n_sel + col : b;
    const double nan = __builtin_nan("");
    out_d[o] = ok ? best : nan;
    if (out_s != nullptr) out_s[o] = ok ? bs : -1;
    if (out_p != nullptr) out_p[o] = ok ? bi : -1;
    if (out_w != nullptr) {
#pragma unroll
        for (int e = 0; e < 9; ++e) out_w[o * 9 + e] = win ? wit[e] : nan;
    }
    if (out_j != nullptr) {
        if (win) prox_row_masks(m, lds_jz, lane, m.rs_mask[bdev], 0u, wit, out_j + o * m.n_q);
        else for (int c = 0; c < m.n_q; ++c) out_j[o * m.n_q + c] = ok ? 0.0 : nan;
    }
}

// ---- certified continuous edges against the cloud (nbk_edge_cloud_continuous_batch) --------------------------------------------
// ca_walk (nbk.hip) as it is, on one (edge e, selected robot shape s) item per lane; keys, ranks, the per-edge reduction and the
// kernels around the walk (k_edge_ca_init, k_ca_final) are those of nbk_edge_continuous_batch.  The grid is (ceil(E / 64), selected shapes): a wave holds ONE shape, so Core.kind and the hull are
// wave-uniform as the cloud routines above need them (a pair-major flat index would straddle shapes).  LDS: [64][n_q] q rows.
//
// The item's motion bound is mu_s = shape_motion_bound (every joint on the shape's path counts: the cloud stands still), and its
// distance at t the clearance of shape s ALONE against the cloud at q(t), cut at
//     D = min(D_end, D_cap),   D_end = (thr + slack) + mu_s (T_f - t),   D_cap = (thr + slack) + look_ahead:
// the smallest distance below D where there is one; else +inf when D == D_end, else D_cap.  Soundness:
//   * every point of shape s moves at most mu_s |t' - t| between q(t) and q(t'), and the points of the cloud stand still;
//   * so no point within D_end at t means that the distance stays above thr + slack up to T_f: the item may stop FREE at T_f, which
//     is what ca_walk makes of +inf (gap is infinite, the advance reaches hi = T_f) -- no new branch;
//   * a distance >= D_cap reported as D_cap is a lower bound of it, and advancing on a lower bound is conservative.
// look_ahead bounds the ball a step walks, and so the points a lane meets: without it the first step of a long edge walks the whole
// cloud.  k_edge_ca_init (nbk.hip) gives CA_KEEP_KEY to the edges whose items do not run and whose result is 0 / UNDECIDED / NaN:
// every non-degenerate edge while the cloud's status is set, and -- accumulating into what nbk_edge_continuous_batch wrote for these
// edges -- those that come in with a NaN t_free.

// the linear edge of EdgeLane for one robot shape against the cloud (pu: the shape's caller's index, p: its device index)
struct CloudEdgeLane {
    const double* s;
    const double* g;
    double Tf;
    const CloudDev& cd;
    double radius;            // of the cloud's points
    double* myq;              // the lane's LDS row
    double d_base, d_cap;     // thr + slack; (thr + slack) + look_ahead
    double mu;
    NBK_DEV double end() const { return Tf; }
    NBK_DEV double span_end() const { return Tf; }
    NBK_DEV double enter(const DevModel& m, int pu, double) { mu = shape_motion_bound(m.mt, pu, EdgeMotion{s, g}); return mu; }
    NBK_DEV double distance(const DevModel& m, bool run, int p, int, double t, double*) {
        bool ok = false;
        if (run) {
            const double omt = 1.0 - t;
            for (int c = 0; c < m.n_q; ++c) { const double a = omt * s[c]; const double b = t * g[c]; myq[c] = a + b; }
            ok = !row_nonfinite(myq, m.n_q, 1);
        }
        Core P;
        cloud_point_core(radius, P);
        Core A;
        cloud_core_init(A);
        double D_end = 0.0, D = 0.0;
        if (ok) {
            Xf T;
            cloud_shape_frame(m, p, myq, T);
            build_core(m, p, T, A);
            if (A.kind == K_HULL) A.rad = -1.0;
            D_end = d_base + mu * (Tf - t);
            D = D_end < d_cap ? D_end : d_cap;
        }
        double best = NBK_INF;
        int bs = -1, bi = -1;
        cloud_core_clearance(cd, A, P, radius, ok, 0, D, best, bs, bi);
        if (!ok) return __builtin_nan("");
        if (best < D) return best;
        return D == D_end ? NBK_INF : d_cap;
    }
};

__global__ __launch_bounds__(64) void k_cloud_edge_ca(DevModel m, CloudDev cd, CloudSel sel, const int* __restrict__ rs_user,
                                                      const double* __restrict__ starts, const double* __restrict__ goals,
                                                      const double* __restrict__ dist, int64_t E, double max_distance, int mode, double thr,
                                                      int max_iter, double slack, double look_ahead, unsigned long long* __restrict__ key) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    // the blockIdx.y-th selected shape, device order
    int p = -1;
    for (int i = 0, k = 0; i < m.n_rshapes; ++i) {
        if (!cloud_selected(sel, i)) continue;
        if (k == (int)blockIdx.y) { p = i; break; }
        ++k;
    }
    if (p < 0) return;
    const int n = cd.hdr->n;
    const int64_t i = (int64_t)blockIdx.x * WAVE + lane;
    const bool live = i < E;
    const int64_t e = live ? i : 0;
    const double base = thr + slack;
    CloudEdgeLane tr{starts + e * m.n_q, goals + e * m.n_q, 0.0, cd, cd.hdr->radius, lds + lane * m.n_q, base, base + look_ahead, 0.0};
    double d_edge = 0.0;
    // (an empty cloud stops every item FREE at T_f, which is where its key stands; the keys of a cloud whose status is set are all reserved)
    const bool run = live && n > 0 && edge_span(m.n_q, tr.s, tr.g, dist, e, max_distance, mode, d_edge, tr.Tf) &&
                     __hip_atomic_load(key + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != CA_KEEP_KEY;
    ca_walk(m, tr, run, rs_user[p], p, lane, thr, max_iter, slack, key + e);
}

// ---- sampled B-spline trajectories against the cloud (nbk_spline_cloud_validity_batch) -------------------------------------------
// Per trajectory s the workspace holds a 64-bit first-hit key, lowered with atomicMin while the sample kernel runs:
//   j + 1 (1 .. 2^31)   sample j collides and no smaller colliding sample is known: only samples below j are still looked at
//   SPC_NONE            open: every sample is looked at, none has collided
//   above SPC_NONE      closed: no sample is looked at, and k_cloud_spline_final reports what the code says
constexpr unsigned long long SPC_NONE = 1ull << 62;
constexpr unsigned long long SPC_KEEP = SPC_NONE + 1ull;          // accumulating: the entry came in 0 without a t_hit to lower; it stays as it is
constexpr unsigned long long SPC_EMPTY = SPC_NONE + 2ull;         // no samples (the degenerate trajectory; bad knots): 0 / NaN / 0
constexpr unsigned long long SPC_TOO_MANY = SPC_NONE + 3ull;      // more than 2^31 - 1 samples: 0 / NaN / -1
constexpr unsigned long long SPC_MAX_SAMPLES = 0x7fffffffull;

// one wave per trajectory, BEFORE the scan: the starting key.  Knots that break the rules (spline_knots_bad, the rule of
// k_spline_ca_init) close every trajectory; a set status word (hold, nullable: the cloud's status; for the held object's entry the
// world status of a movable descriptor) hits every trajectory that has samples at its first one; accumulating,
// an entry that is 0 and has no finite t_hit to lower is closed (t_prev: the caller's t_hit, null when it gave none or does not
// accumulate).  A trajectory closed as SPC_EMPTY or SPC_TOO_MANY gets the count 0, so the flat sample range holds no sample of it
// and the sample kernel's run time is bounded by the samples that can be looked at (k_cloud_spline_final reads 0 / -1 off the key).
__global__ __launch_bounds__(64) void k_cloud_spline_init(int n, int k, const double* __restrict__ knots,
                                                          unsigned long long* __restrict__ cnt, const int* __restrict__ hold,
                                                          int accumulate, const uint8_t* __restrict__ valid,
                                                          const double* __restrict__ t_prev, unsigned long long* __restrict__ first) {
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const bool bad = spline_knots_bad(knots, n, k, lane);
    if (lane != 0) return;
    const unsigned long long c = cnt[s];
    unsigned long long key = SPC_NONE;
    if (bad || c == 0ull) key = SPC_EMPTY;
    else if (c > SPC_MAX_SAMPLES) key = SPC_TOO_MANY;
    else if (hold != nullptr && *hold != 0) key = 1ull;
    else if (accumulate && valid[s] == 0 && (t_prev == nullptr || t_prev[s] != t_prev[s])) key = SPC_KEEP;
    if (key == SPC_EMPTY || key == SPC_TOO_MANY) cnt[s] = 0ull;
    first[s] = key;
}

// One sample per lane, FLAT across the trajectories, as k_cloud_edges: sample f of [0, total) belongs to the largest trajectory s with
// offs[s] <= f (trajectories without samples fall out by themselves: equal offsets) and is sample j = f - offs[s] of it; t_j, the
// span and de Boor are k_spline_expand's expressions, with the row going to the lane's LDS row instead of a slab.  The grid has a
// fixed size (SPLINE_CLOUD_WAVES_PER_CU); a workgroup strides over 64-sample blocks until `total`, read here, never by the host.
// A lane skips its sample when the trajectory's key says so (closed, or a hit at or below j is known), or -- accumulating with a
// t_hit -- when t_j is not below the t_hit the entry came in with (a NaN there: the entry came in valid, every sample counts).
template <int K>
__global__ __launch_bounds__(64) void k_cloud_spline(DevModel m, CloudDev cd, CloudSel sel, const double* __restrict__ ctrl, int n,
                                                     const double* __restrict__ knots, const double* __restrict__ plan,
                                                     const unsigned long long* __restrict__ offs, int64_t S, double thr,
                                                     const double* __restrict__ t_prev, unsigned long long* first) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    double* myq = lds + lane * m.n_q;
    const unsigned long long total = offs[S];
    const int ncl = cd.hdr->n;
    const double radius = cd.hdr->radius;
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
                    work = !row_nonfinite(myq, m.n_q, 1);
                    hit = !work;                             // a non-finite sample collides
                }
            }
        }
        if (ncl > 0 && __builtin_amdgcn_ballot_w64(work) != 0ull) cloud_row_hits(m, cd, sel, radius, thr, myq, work, hit);
        if (hit) atomicMin(first + s, j + 1ull);
    }
}

// key -> valid / t_hit / n_samples.  Accumulating, an open trajectory without a hit keeps what it came in with (1 / NaN, or 0 and
// the scene's t_hit); t_j by the expression of k_spline_reduce.
__global__ __launch_bounds__(256) void k_cloud_spline_final(int64_t S, const double* __restrict__ plan, const unsigned long long* __restrict__ cnt,
                                                            const unsigned long long* __restrict__ first, int accumulate,
                                                            uint8_t* __restrict__ valid, double* __restrict__ t_hit,
                                                            int32_t* __restrict__ n_samples) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const unsigned long long key = first[s];
    if (n_samples != nullptr) n_samples[s] = key == SPC_EMPTY ? 0 : (key == SPC_TOO_MANY ? -1 : (int32_t)cnt[s]);
    if (key == SPC_EMPTY || key == SPC_TOO_MANY) {
        valid[s] = 0;
        if (t_hit != nullptr) t_hit[s] = __builtin_nan("");
    } else if (key == SPC_KEEP) valid[s] = 0;
    else if (key == SPC_NONE) {
        if (!accumulate) { valid[s] = 1; if (t_hit != nullptr) t_hit[s] = __builtin_nan(""); }
    } else {
        valid[s] = 0;
        const double j = (double)(key - 1ull);
        if (t_hit != nullptr) t_hit[s] = j < plan[2 * s + 1] ? j * plan[2 * s] : 1.0;
    }
}

// ---- certified continuous B-splines against the cloud (nbk_spline_cloud_continuous_batch) ----------------------------------------
// ca_walk as it is, on one (trajectory, selected robot shape) item per lane, grid (ceil(S / 64), selected shapes) as k_cloud_edge_ca;
// init is nbk.hip's k_spline_ca_init (hold = the cloud's status, prev when accumulating), final its k_ca_final.  The lane is
// SplineLane's trajectory with CloudEdgeLane's distance: entering a span gives mu = shape_motion_bound on that span, q(t) goes by
// de_boor into the lane's LDS row, and the distance is the shape's clearance from the cloud cut at
//     D = min(D_end, D_cap),   D_end = (thr + slack) + mu_max (1 - t),   D_cap = (thr + slack) + look_ahead,
// the smallest distance below D where there is one; else +inf when D == D_end; else D_cap.  mu_max is the LARGEST span bound of the
// trajectory over its non-empty spans, not the current span's.  Soundness of the +inf:
//   * ca_walk carries an infinite gap across ALL remaining spans without another evaluation (gap - mu (hi - t) stays infinite), so
//     +inf at t stops the item FREE at 1: it may only be reported when no point can be reached on the whole remainder [t, 1];
//   * each span's mu bounds the speed of every point of the shape on that span, so mu_max bounds it on every span, and no point of
//     the shape travels further than mu_max (1 - t) between q(t) and any q(t'), t' in [t, 1]; the cloud stands still;
//   * so no point within D_end at t means that the distance stays above thr + slack up to 1;
//   * D_cap is a lower bound of a distance that is not below it, and advancing on a lower bound is conservative, span by span with
//     each span's own mu, as for the scene's pairs.
// With n = 2, K = 1 and the knots [0, 0, 1, 1] there is one span, mu_max = mu and T_f = 1: CloudEdgeLane's bits in connect mode.
template <int K>
struct CloudSplineLane {
    const double* c;          // control points of the trajectory, [n][nq]
    const double* knots;
    int n, nq, ell;
    const CloudDev& cd;
    double radius;            // of the cloud's points
    double* myq;              // the lane's LDS row
    double d_base, d_cap;     // thr + slack; (thr + slack) + look_ahead
    double mu_max;
    NBK_DEV double end() const { return 1.0; }
    NBK_DEV double span_end() const { return knots[ell + 1]; }
    NBK_DEV double span_bound(const DevModel& m, int pu, int span) const {
        return shape_motion_bound(m.mt, pu, SplineSpanMotion{c + (size_t)(span - K) * nq, knots + (span - K + 1), nq, K});
    }
    NBK_DEV double enter(const DevModel& m, int pu, double t) {
        ell = spline_span<K>(knots, n, t);
        return span_bound(m, pu, ell);
    }
    // the largest bound over the non-empty spans: what D_end may use (see above)
    NBK_DEV void bound_all(const DevModel& m, int pu) {
        mu_max = 0.0;
        for (int span = K; span < n; ++span) {
            if (!(knots[span] < knots[span + 1])) continue;
            const double mu = span_bound(m, pu, span);
            mu_max = mu > mu_max ? mu : mu_max;
        }
    }
    NBK_DEV double distance(const DevModel& m, bool run, int p, int, double t, double*) {
        bool ok = false;
        if (run) {
            double* r = myq;
            de_boor<K>(nq, c + (size_t)(ell - K) * nq, knots, ell, t, [&](int j, double v) { r[j] = v; });
            ok = !row_nonfinite(myq, nq, 1);
        }
        Core P;
        cloud_point_core(radius, P);
        Core A;
        cloud_core_init(A);
        double D_end = 0.0, D = 0.0;
        if (ok) {
            Xf T;
            cloud_shape_frame(m, p, myq, T);
            build_core(m, p, T, A);
            if (A.kind == K_HULL) A.rad = -1.0;
            // mu_max, NOT the current span's mu: +inf frees the item up to 1 across every later span (ca_walk evaluates nothing
            // there), and a later span may be faster than this one -- a per-span D_end would free a trajectory that sweeps into a
            // point after a slow start
            D_end = d_base + mu_max * (1.0 - t);
            D = D_end < d_cap ? D_end : d_cap;
        }
        double best = NBK_INF;
        int bs = -1, bi = -1;
        cloud_core_clearance(cd, A, P, radius, ok, 0, D, best, bs, bi);
        if (!ok) return __builtin_nan("");
        if (best < D) return best;
        return D == D_end ? NBK_INF : d_cap;
    }
};

template <int K>
__global__ __launch_bounds__(64) void k_cloud_spline_ca(DevModel m, CloudDev cd, CloudSel sel, const int* __restrict__ rs_user,
                                                        const double* __restrict__ ctrl, int64_t S, int n,
                                                        const double* __restrict__ knots, double thr, int max_iter, double slack,
                                                        double look_ahead, unsigned long long* __restrict__ key) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    // the blockIdx.y-th selected shape, device order
    int p = -1;
    for (int i = 0, k = 0; i < m.n_rshapes; ++i) {
        if (!cloud_selected(sel, i)) continue;
        if (k == (int)blockIdx.y) { p = i; break; }
        ++k;
    }
    if (p < 0) return;
    const int ncl = cd.hdr->n;
    const int64_t i = (int64_t)blockIdx.x * WAVE + lane;
    const bool live = i < S;
    const int64_t s = live ? i : 0;
    const double base = thr + slack;
    CloudSplineLane<K> tr{ctrl + (size_t)s * (size_t)n * m.n_q, knots, n, m.n_q, K, cd, cd.hdr->radius, lds + lane * m.n_q, base,
                          base + look_ahead, 0.0};
    // (an empty cloud stops every item FREE at 1, which is where its key stands; the keys of a cloud whose status is set are all reserved)
    bool run = false;
    if (live && ncl > 0) {
        const unsigned long long k0 = __hip_atomic_load(key + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        run = k0 != CA_DEGENERATE_KEY && k0 != CA_KEEP_KEY;
    }
    const int pu = rs_user[p];
    if (run) tr.bound_all(m, pu);
    ca_walk(m, tr, run, pu, p, lane, thr, max_iter, slack, key + s);
}

}  // namespace nbk

struct nbk_cloud {
    nbk::CloudGrid g;
    int64_t capacity;
    int cells;
    int device;
    void* blob;
    nbk::CloudHdr* hdr;
    unsigned* fill;
    unsigned* start;
    int* cell_of;
    int* idx;
    double* pts;
    hipEvent_t updated;            // recorded after each update issued outside a capture: nbk_cloud_status waits for it (an event of
    bool last_set;                 // the cloud's own, so a caller may destroy the stream of an update before asking for the status)
};

namespace nbk {

static int32_t cloud_check_device(const nbk_cloud* c) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != c->device) {
        snprintf(g_err, sizeof(g_err), "cloud belongs to device %d, the current device is %d", c->device, dev);
        return NBK_ERR_INVALID;
    }
    return NBK_OK;
}

static CloudDev cloud_dev(const nbk_cloud* c) { return CloudDev{c->g, c->hdr, c->pts, c->idx, c->start}; }
// the status word of the cloud (device memory: an address, not a read), which holds the trajectory calls while it is set
static const int* cloud_status_word(const nbk_cloud* c) { return &c->hdr->status; }

// the caller's selection (bit s of shape_bits = robot shape s of the descriptor it passed to nbk_model_create) in device order
static CloudSel cloud_selection(const nbk_model* m, const uint64_t* shape_bits) {
    CloudSel sel{{0ull, 0ull, 0ull, 0ull}, shape_bits == nullptr ? 1 : 0};
    if (shape_bits != nullptr)
        for (size_t i = 0; i < m->h_rs_user.size(); ++i) {
            const int u = m->h_rs_user[i];
            if ((shape_bits[u >> 6] >> (u & 63)) & 1ull) sel.w[i >> 6] |= 1ull << (i & 63);
        }
    return sel;
}

// the selected shapes of a call, counted
static int cloud_selected_count(const nbk_model* m, const CloudSel& sel) {
    if (sel.all) return m->d.n_rshapes;
    int n_sel = 0;
    for (int k = 0; k < 4; ++k) n_sel += __builtin_popcountll(sel.w[k]);
    return n_sel;
}

// What every query entry answers once its own argument rules are through (they come first: INVALID is answered without a device), in
// this order: a selection on a model of more than 256 robot shapes is UNSUPPORTED (CloudSel holds 256 bits); the model's device and
// the cloud's must be the current one; then `sel` is the selection.  n_sel (the certified entries, whose grid has one row of
// workgroups per selected shape): their count, UNSUPPORTED above the 65535 rows a grid has.  -> the first code that fails
// Its sibling for a call that has a descriptor and no cloud (nbk_frame_cloud_self_filter) is the same without the cloud's device:
// cloud_model_begin.
static int32_t cloud_model_begin(const nbk_model* m, const uint64_t* shape_bits, CloudSel& sel) {
    if (shape_bits != nullptr && m->d.n_rshapes > 256) return NBK_ERR_UNSUPPORTED;
    NBK_DEVICE(m);
    sel = cloud_selection(m, shape_bits);
    return NBK_OK;
}
static int32_t cloud_call_begin(const nbk_model* m, const nbk_cloud* c, const uint64_t* shape_bits, CloudSel& sel, int* n_sel = nullptr) {
    { const int32_t rc = cloud_model_begin(m, shape_bits, sel); if (rc != NBK_OK) return rc; }
    { const int32_t rc = cloud_check_device(c); if (rc != NBK_OK) return rc; }
    if (n_sel != nullptr && (*n_sel = cloud_selected_count(m, sel)) > 65535) return NBK_ERR_UNSUPPORTED;
    return NBK_OK;
}

// the caller's workspace of the sampled entries: at least `need` bytes (a layout's) at a 64-byte boundary
static bool cloud_workspace_ok(const void* workspace, int64_t workspace_bytes, size_t need) {
    return workspace_bytes >= (int64_t)need && (reinterpret_cast<uintptr_t>(workspace) & 63) == 0;
}

// the workspace sizes of the sampled entries (the cloud's, the held object's, the held object's against a cloud: one layout each)
static int64_t edge_workspace_bytes(int64_t E) { return E < 0 || E > EDGE_CLOUD_MAX_E ? -1 : (int64_t)EdgeCloudLayout(E).bytes; }
// (a spline entry takes fewer than SPLINE_MAX_S trajectories)
static int64_t spline_workspace_bytes(int64_t S) { return S < 0 || S >= SPLINE_MAX_S ? -1 : (int64_t)SplineCloudLayout(S).bytes; }

// ---- One call path per entry kind.  The trajectory entries of the three families -- the cloud's here, the held object's and the held
// object's against a cloud in nbk_held.hpp -- are, kind by kind, one sequence of statements: the routines below.  An entry checks
// its handles for null and passes what is its own: begin(), the family's *_call_begin (run once the argument rules, "nothing to do"
// and the size limit are through: those are answered without a device and before the handles are looked at); hold, the status word
// that holds the call (the cloud's, or a movable descriptor's world status, or null); launch_walk, which launches the family's walk
// kernel.  Callables, not std::function: nothing allocates on the call path, and these entries are capturable.

// sampled edges: k_edge_plan -> k_scan -> k_cloud_edges_init -> launch_walk(grid, lds, st, es, offs)
template <class Begin, class Walk>
static int32_t sampled_edges_call(const nbk_model* m, const double* starts, const double* goals, const double* dist, int64_t E,
                                  double resolution, double max_distance, int32_t mode, double threshold, int32_t accumulate,
                                  uint8_t* valid, double* end, int32_t* n_samples, void* workspace, int64_t workspace_bytes, void* stream,
                                  Begin&& begin, Walk&& launch_walk) {
    if (E < 0) return NBK_ERR_INVALID;
    if (E > 0 && (starts == nullptr || goals == nullptr || valid == nullptr || workspace == nullptr)) return NBK_ERR_INVALID;
    if (!edge_args_ok(RULE_RESOLUTION | RULE_THRESHOLD, resolution, max_distance, mode, threshold)) return NBK_ERR_INVALID;
    if (E > 0 && E <= EDGE_CLOUD_MAX_E &&
        !cloud_workspace_ok(workspace, workspace_bytes, EdgeCloudLayout(E).bytes)) return NBK_ERR_INVALID;
    if (E == 0) return NBK_OK;
    if (E > 0x7fffffffLL) return NBK_ERR_UNSUPPORTED;
    { const int32_t rc = begin(); if (rc != NBK_OK) return rc; }
    hipStream_t st = (hipStream_t)stream;
    const EdgeCloudLayout::View v = EdgeCloudLayout(E).view(workspace);
    const unsigned eblocks = (unsigned)((E + 255) / 256);
    hipLaunchKernelGGL(k_edge_plan, dim3(eblocks), dim3(256), 0, st, m->n_q, starts, goals, dist, E, resolution, max_distance, (int)mode,
                       v.plan, v.cnt, end, n_samples);
    NBK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, v.cnt, E, v.offs);
    NBK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cloud_edges_init, dim3(eblocks), dim3(256), 0, st, v.cnt, E, (int)accumulate, valid);
    NBK_HIP(hipGetLastError());
    // the grid covers the static bound; what lies beyond it is reached by the kernel's stride
    const EdgeSrc es{starts, goals, v.plan, nullptr, v.offs + E, 0, nullptr};
    launch_walk(dim3((unsigned)(edge_capacity(E, resolution, max_distance) / WAVE)), QSlabLds(m->n_q).bytes(), st, es, v.offs);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

// sampled splines: k_spline_plan -> k_cloud_spline_init (hold) -> k_scan -> launch_walk(K, grid, lds, st, v, t_prev) ->
// k_cloud_spline_final
template <class Begin, class Walk>
static int32_t sampled_splines_call(const nbk_model* m, const double* ctrl, int64_t S, int32_t n_ctrl, int32_t degree, const double* knots,
                                    double resolution, double threshold, const int* hold, int32_t accumulate, uint8_t* valid,
                                    double* t_hit, int32_t* n_samples, void* workspace, int64_t workspace_bytes, void* stream,
                                    Begin&& begin, Walk&& launch_walk) {
    if (S < 0) return NBK_ERR_INVALID;
    if (S > 0 && (ctrl == nullptr || knots == nullptr || valid == nullptr || workspace == nullptr)) return NBK_ERR_INVALID;
    if (!spline_args_ok(n_ctrl, degree, nullptr)) return NBK_ERR_INVALID;      // (the knots are on the device)
    if (!(resolution > 0.0 && resolution <= 1.7976931348623157e308) || threshold != threshold) return NBK_ERR_INVALID;
    if (S > 0 && S < SPLINE_MAX_S &&
        !cloud_workspace_ok(workspace, workspace_bytes, SplineCloudLayout(S).bytes)) return NBK_ERR_INVALID;
    if (S == 0) return NBK_OK;
    if (S >= SPLINE_MAX_S) return NBK_ERR_UNSUPPORTED;
    { const int32_t rc = begin(); if (rc != NBK_OK) return rc; }
    int cus = 0;                                    // (begin() has found the descriptor's device to be the current one, and the handles')
    NBK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m->device));
    hipStream_t st = (hipStream_t)stream;
    const SplineCloudLayout::View v = SplineCloudLayout(S).view(workspace);
    hipLaunchKernelGGL(k_spline_plan, dim3((unsigned)S), dim3(WAVE), 0, st, m->n_q, ctrl, (int)n_ctrl, (int)degree, knots, resolution, v.plan, v.cnt);
    NBK_HIP(hipGetLastError());
    const double* t_prev = accumulate ? t_hit : nullptr;
    hipLaunchKernelGGL(k_cloud_spline_init, dim3((unsigned)S), dim3(WAVE), 0, st, (int)n_ctrl, (int)degree, knots, v.cnt, hold, (int)accumulate,
                       (const uint8_t*)valid, t_prev, v.first);
    NBK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, v.cnt, S, v.offs);
    NBK_HIP(hipGetLastError());
    // a grid of fixed size: the sample total is the device's to know, the kernel strides to it
    const dim3 grid((unsigned)((cus > 0 ? cus : 1) * SPLINE_CLOUD_WAVES_PER_CU));
    const size_t lds = QSlabLds(m->n_q).bytes();
    with_degree(degree, [&](auto K) { launch_walk(K, grid, lds, st, v, t_prev); });
    NBK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cloud_spline_final, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, S, (const double*)v.plan,
                       (const unsigned long long*)v.cnt, (const unsigned long long*)v.first, (int)accumulate, valid, t_hit, n_samples);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

// What the two certified routines take besides: look_ahead, null for the held object's own entries, which have none; *items, the
// family's items per trajectory, read once begin() is through (the walk is skipped at 0); flat: the family's grid is flat, n x *items
// lanes, which the size limit then counts -- with *items read BEFORE begin(), as the held object's own entries have it; grasp_status
// and grasp: launch_held_ca_hold's, both null for the cloud's own entries.

// certified edges: k_edge_ca_init (hold, prev when accumulating) -> the grasp hold -> launch_walk(st) -> k_ca_final
template <class Begin, class Walk>
static int32_t certified_edges_call(const nbk_model* m, const double* starts, const double* goals, const double* dist, int64_t E,
                                    double max_distance, int32_t mode, double threshold, int32_t max_iter, double slack,
                                    const double* look_ahead, const int* items, bool flat, const int* hold, const int* grasp_status,
                                    const double* grasp, int32_t accumulate, uint8_t* valid, double* end, double* t_free,
                                    int32_t* status, void* stream, Begin&& begin, Walk&& launch_walk) {
    if (E < 0) return NBK_ERR_INVALID;
    if (E > 0 && (starts == nullptr || goals == nullptr || valid == nullptr || t_free == nullptr || status == nullptr)) return NBK_ERR_INVALID;
    if (!edge_args_ok(RULE_CERTIFIED | RULE_THRESHOLD, 0.0, max_distance, mode, threshold, max_iter, slack)) return NBK_ERR_INVALID;
    if (look_ahead != nullptr && !(*look_ahead > 0.0)) return NBK_ERR_INVALID;                  // NaN included; +inf is served
    if (E == 0) return NBK_OK;
    if (E > 0x7fffffffLL || (flat && (E * (int64_t)*items + WAVE - 1) / WAVE > 0x7fffffffLL)) return NBK_ERR_UNSUPPORTED;
    { const int32_t rc = begin(); if (rc != NBK_OK) return rc; }
    hipStream_t st = (hipStream_t)stream;
    { const int32_t rc = launch_edge_ca_init(m, st, starts, goals, dist, E, max_distance, mode, hold, accumulate ? status : nullptr, end, t_free);
      if (rc != NBK_OK) return rc; }
    { const int32_t rc = launch_held_ca_hold(st, grasp_status, grasp, E, t_free); if (rc != NBK_OK) return rc; }
    if (*items > 0) {
        launch_walk(st);
        NBK_HIP(hipGetLastError());
    }
    return launch_ca_final(st, E, valid, t_free, status);
}

// certified splines: k_spline_ca_init (hold, prev when accumulating) -> the grasp hold -> launch_walk(K, lds, st) -> k_ca_final
template <class Begin, class Walk>
static int32_t certified_splines_call(const nbk_model* m, const double* ctrl, int64_t S, int32_t n_ctrl, int32_t degree, const double* knots,
                                      double threshold, int32_t max_iter, double slack, const double* look_ahead, const int* items,
                                      bool flat, const int* hold, const int* grasp_status, const double* grasp, int32_t accumulate,
                                      uint8_t* valid, double* t_free, int32_t* status, void* stream, Begin&& begin, Walk&& launch_walk) {
    if (S < 0) return NBK_ERR_INVALID;
    if (S > 0 && (ctrl == nullptr || knots == nullptr || valid == nullptr || t_free == nullptr || status == nullptr)) return NBK_ERR_INVALID;
    if (!spline_args_ok(n_ctrl, degree, nullptr)) return NBK_ERR_INVALID;      // (the knots are on the device)
    if (max_iter < 1 || !(slack >= 0.0) || threshold != threshold) return NBK_ERR_INVALID;
    if (look_ahead != nullptr && !(*look_ahead > 0.0)) return NBK_ERR_INVALID;                  // NaN included; +inf is served
    if (S == 0) return NBK_OK;
    if (S > 0x7fffffffLL || (flat && (S * (int64_t)*items + WAVE - 1) / WAVE > 0x7fffffffLL)) return NBK_ERR_UNSUPPORTED;
    { const int32_t rc = begin(); if (rc != NBK_OK) return rc; }
    hipStream_t st = (hipStream_t)stream;
    { const int32_t rc = launch_spline_ca_init(m, st, ctrl, S, n_ctrl, degree, knots, hold, accumulate ? status : nullptr, t_free);
      if (rc != NBK_OK) return rc; }
    { const int32_t rc = launch_held_ca_hold(st, grasp_status, grasp, S, t_free); if (rc != NBK_OK) return rc; }
    if (*items > 0) {
        const size_t lds = QSlabLds(m->n_q).bytes();
        with_degree(degree, [&](auto K) { launch_walk(K, lds, st); });
        NBK_HIP(hipGetLastError());
    }
    return launch_ca_final(st, S, valid, t_free, status);
}

}  // namespace nbk

extern "C" {

int32_t nbk_cloud_cells_host(const double lo[3], double cell, const int32_t dims[3], const double* pts, int64_t N, int32_t* cell_out) {
    if (!cloud_grid_valid(lo, cell, dims) || N < 0 || (N > 0 && (pts == nullptr || cell_out == nullptr))) return NBK_ERR_INVALID;
    const CloudGrid g{{lo[0], lo[1], lo[2]}, cell, {dims[0], dims[1], dims[2]}};
    for (int64_t i = 0; i < N; ++i) cell_out[i] = cloud_cell(g, pts + 3 * i);
    return NBK_OK;
}

int32_t nbk_cloud_create(int64_t capacity, const double lo[3], double cell, const int32_t dims[3], nbk_cloud** out) {
    if (out == nullptr) return NBK_ERR_INVALID;
    *out = nullptr;
    if (capacity < 1 || capacity > CLOUD_MAX_POINTS || !cloud_grid_valid(lo, cell, dims)) return NBK_ERR_INVALID;
    if (nbk_device_count() <= 0) return NBK_ERR_NO_DEVICE;
    std::unique_ptr<nbk_cloud> c(new nbk_cloud());
    c->g = CloudGrid{{lo[0], lo[1], lo[2]}, cell, {dims[0], dims[1], dims[2]}};
    c->capacity = capacity;
    c->cells = dims[0] * dims[1] * dims[2];
    auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
    const size_t o_fill = sizeof(CloudHdr);
    const size_t o_start = up(o_fill + sizeof(unsigned) * (size_t)c->cells);
    const size_t o_cell = up(o_start + sizeof(unsigned) * ((size_t)c->cells + 1));
    const size_t o_idx = up(o_cell + sizeof(int) * (size_t)capacity);
    const size_t o_pts = up(o_idx + sizeof(int) * (size_t)capacity);
    const size_t bytes = o_pts + sizeof(double) * 3 * (size_t)capacity;
    hipError_t e = hipMalloc(&c->blob, bytes);
    if (e != hipSuccess) { hip_fail(e, "hipMalloc(cloud)"); return NBK_ERR_ALLOC; }
    char* base = static_cast<char*>(c->blob);
    c->hdr = reinterpret_cast<CloudHdr*>(base);
    c->fill = reinterpret_cast<unsigned*>(base + o_fill);
    c->start = reinterpret_cast<unsigned*>(base + o_start);
    c->cell_of = reinterpret_cast<int*>(base + o_cell);
    c->idx = reinterpret_cast<int*>(base + o_idx);
    c->pts = reinterpret_cast<double*>(base + o_pts);
    // an empty cloud until the first update: status 0, N 0, every cell empty
    e = hipMemset(c->blob, 0, o_cell);
    if (e != hipSuccess) { (void)hipFree(c->blob); return hip_fail(e, "hipMemset(cloud)"); }
    e = hipEventCreateWithFlags(&c->updated, hipEventDisableTiming);
    if (e != hipSuccess) { (void)hipFree(c->blob); return hip_fail(e, "hipEventCreate(cloud)"); }
    (void)hipGetDevice(&c->device);
    c->last_set = false;
    *out = c.release();
    return NBK_OK;
}

void nbk_cloud_destroy(nbk_cloud* c) {
    if (c == nullptr) return;
    if (c->blob) (void)hipFree(c->blob);
    (void)hipEventDestroy(c->updated);
    delete c;
}

int32_t nbk_frame_cloud_set_points(nbk_cloud* c, const double* pts, const uint8_t* keep, int64_t N, double radius, void* stream) {
    if (c == nullptr || N < 0 || N > c->capacity || !(radius >= 0.0) || (N > 0 && pts == nullptr)) return NBK_ERR_INVALID;
    { const int32_t rc = cloud_check_device(c); if (rc != NBK_OK) return rc; }
    hipStream_t st = (hipStream_t)stream;
    NBK_HIP(hipMemsetAsync(c->hdr, 0, sizeof(CloudHdr) + sizeof(unsigned) * (size_t)c->cells, st));
    const unsigned blocks = (unsigned)((N + 255) / 256);
    if (N > 0) {
        hipLaunchKernelGGL(k_cloud_count, dim3(blocks), dim3(256), 0, st, c->g, pts, (int)N, keep, c->cell_of, c->fill, &c->hdr->status);
        NBK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_cloud_scan, dim3(1), dim3(1024), 0, st, c->fill, c->start, c->cells, c->hdr, radius);
    NBK_HIP(hipGetLastError());
    if (N > 0) {
        hipLaunchKernelGGL(k_cloud_scatter, dim3(blocks), dim3(256), 0, st, pts, (int)N, keep, (const int*)c->cell_of, c->fill, c->pts,
                           c->idx, (unsigned)c->capacity);
        NBK_HIP(hipGetLastError());
    }
    if (!stream_capturing(st)) { NBK_HIP(hipEventRecord(c->updated, st)); c->last_set = true; }
    return NBK_OK;
}

int32_t nbk_cloud_set_points(nbk_cloud* c, const double* pts, int64_t N, double radius, void* stream) {
    return nbk_frame_cloud_set_points(c, pts, nullptr, N, radius, stream);
}

int32_t nbk_frame_cloud_count(const nbk_cloud* c, int64_t* n) {
    if (c == nullptr || n == nullptr) return NBK_ERR_INVALID;
    { const int32_t rc = cloud_check_device(c); if (rc != NBK_OK) return rc; }
    if (c->last_set) NBK_HIP(hipEventSynchronize(c->updated));
    int v = 0;
    NBK_HIP(hipMemcpy(&v, &c->hdr->n, sizeof(int), hipMemcpyDeviceToHost));
    *n = v;
    return NBK_OK;
}

int32_t nbk_cloud_status(const nbk_cloud* c, int32_t* status) {
    if (c == nullptr || status == nullptr) return NBK_ERR_INVALID;
    { const int32_t rc = cloud_check_device(c); if (rc != NBK_OK) return rc; }
    if (c->last_set) NBK_HIP(hipEventSynchronize(c->updated));
    int v = 0;
    NBK_HIP(hipMemcpy(&v, &c->hdr->status, sizeof(int), hipMemcpyDeviceToHost));
    *status = v;
    return NBK_OK;
}

// the image and camera rules every entry that takes a frame shares
static bool frame_args_ok(const void* depth, int32_t depth_type, int32_t H, int32_t W, const DepthCam& cam, const double* T) {
    if (H < 0 || W < 0 || (int64_t)H * (int64_t)W > CLOUD_MAX_POINTS) return false;
    if ((depth_type != 0 && depth_type != 1) || !depth_cam_valid(cam) || T == nullptr) return false;
    return (int64_t)H * (int64_t)W == 0 || depth != nullptr;
}

// the argument rules the two back-projection entries share: the frame's and the two outputs
static bool backproject_args_ok(const void* depth, int32_t depth_type, int32_t H, int32_t W, const DepthCam& cam, const double* T,
                                const double* pts, const uint8_t* keep) {
    return frame_args_ok(depth, depth_type, H, W, cam, T) && ((int64_t)H * (int64_t)W == 0 || (pts != nullptr && keep != nullptr));
}

int32_t nbk_frame_cloud_backproject_host(const void* depth, int32_t depth_type, int32_t H, int32_t W, double depth_scale, double fx, double fy,
                                   double cx, double cy, const double* T, double z_min, double z_max, double* pts, uint8_t* keep) {
    const DepthCam cam{depth_scale, fx, fy, cx, cy, z_min, z_max};
    if (!backproject_args_ok(depth, depth_type, H, W, cam, T, pts, keep)) return NBK_ERR_INVALID;
    const int64_t n = (int64_t)H * (int64_t)W;
    for (int64_t i = 0; i < n; ++i)
        keep[i] = depth_backproject_pixel(cam, T, (int)(i % W), (int)(i / W), depth_pixel_value(depth, depth_type, i), pts + 3 * i) ? 1 : 0;
    return NBK_OK;
}

int32_t nbk_frame_cloud_backproject(const void* depth, int32_t depth_type, int32_t H, int32_t W, double depth_scale, double fx, double fy,
                              double cx, double cy, const double* T, double z_min, double z_max, double* pts, uint8_t* keep,
                              void* stream) {
    const DepthCam cam{depth_scale, fx, fy, cx, cy, z_min, z_max};
    if (!backproject_args_ok(depth, depth_type, H, W, cam, T, pts, keep)) return NBK_ERR_INVALID;
    if (nbk_device_count() <= 0) return NBK_ERR_NO_DEVICE;
    const int n = H * W;
    if (n == 0) return NBK_OK;
    hipLaunchKernelGGL(k_cloud_backproject, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth, (int)depth_type,
                       (int)W, n, cam, T, pts, keep);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int64_t nbk_frame_cloud_self_filter_lds_bytes(int32_t n_shapes) {
    if (n_shapes < 0 || !SelfFilterLds(n_shapes).fits()) return -1;
    return (int64_t)SelfFilterLds(n_shapes).bytes();
}

int32_t nbk_frame_cloud_self_filter(const nbk_model* m, const double* q0, const double* pts, int64_t N, double radius, double padding,
                              const uint64_t* shape_bits, uint8_t* keep, void* stream) {
    if (m == nullptr || q0 == nullptr || N < 0 || N > CLOUD_MAX_POINTS || !(radius >= 0.0) || padding != padding ||
        (N > 0 && (pts == nullptr || keep == nullptr))) return NBK_ERR_INVALID;
    CloudSel sel;
    { const int32_t rc = cloud_model_begin(m, shape_bits, sel); if (rc != NBK_OK) return rc; }
    const int n_sel = cloud_selected_count(m, sel);
    const SelfFilterLds L(n_sel);
    if (!L.fits()) return NBK_ERR_UNSUPPORTED;
    if (N == 0 || n_sel == 0) return NBK_OK;
    int dev = 0, cus = 0;
    NBK_HIP(hipGetDevice(&dev));
    NBK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // a bounded grid: every workgroup pays the preamble (the selected shapes' cores at q0) once and then strides over the points
    const int64_t want = (N + 255) / 256, most = (int64_t)(cus > 0 ? cus : 1) * SELF_FILTER_WGS_PER_CU;
    hipLaunchKernelGGL(k_cloud_self_filter, dim3((unsigned)(want < most ? want : most)), dim3(256), L.bytes(), (hipStream_t)stream, m->d, sel,
                       n_sel, q0, pts, (int)N, radius, padding, keep);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int64_t nbk_render_depth_lds_bytes(int32_t n_shapes) {
    if (n_shapes < 0 || !RenderLds(n_shapes, n_shapes).fits()) return -1;
    return (int64_t)RenderLds(n_shapes, n_shapes).bytes();
}

// the camera and range rules the two rendering entries share
static bool render_cam_ok(int32_t H, int32_t W, double fx, double fy, const double* T, double z_near, double z_far) {
    return H >= 0 && W >= 0 && fx > 0.0 && fy > 0.0 && T != nullptr && z_near >= 0.0 && z_far > z_near;
}

int32_t nbk_render_ray_spans_host(int32_t H, int32_t W, double fx, double fy, double cx, double cy, const double* T, const double* centres,
                                  const double* radii, int32_t S, double z_near, double z_far, double* span, uint8_t* hit) {
    if (!render_cam_ok(H, W, fx, fy, T, z_near, z_far) || S < 0) return NBK_ERR_INVALID;
    const int64_t n = (int64_t)H * (int64_t)W;
    if (n * S > 0 && (centres == nullptr || radii == nullptr || span == nullptr || hit == nullptr)) return NBK_ERR_INVALID;
    const DepthCam cam{1.0, fx, fy, cx, cy, z_near, z_far};
    for (int64_t i = 0; i < n; ++i)
        for (int32_t s = 0; s < S; ++s) {
            double z0 = 0.0, z1 = 0.0;
            const bool h = depth_ray_sphere_span(cam, T, (int)(i % W), (int)(i / W), centres + 3 * (size_t)s, radii[s], z_near, z_far, &z0, &z1);
            span[2 * (i * S + s)] = h ? z0 : 0.0;
            span[2 * (i * S + s) + 1] = h ? z1 : 0.0;
            hit[i * S + s] = h ? 1 : 0;
        }
    return NBK_OK;
}

int32_t nbk_render_depth_batch(const nbk_model* m, const double* q, int64_t Bq, const double* T, int64_t Bt, int64_t B, int32_t H, int32_t W,
                               double fx, double fy, double cx, double cy, double z_near, double z_far, double eps, int32_t max_steps,
                               const uint64_t* shape_bits, int32_t draw_world, float miss, float* depth, int32_t* label, int64_t* counts,
                               void* stream) {
    if (m == nullptr || B < 0 || !render_cam_ok(H, W, fx, fy, T, z_near, z_far) || !(eps > 0.0) || max_steps < 1 || max_steps > 4096 ||
        !(cx - cx == 0.0) || !(cy - cy == 0.0))
        return NBK_ERR_INVALID;
    if ((Bq != 1 && Bq != B) || (Bt != 1 && Bt != B)) return NBK_ERR_INVALID;
    const int64_t hw = (int64_t)H * (int64_t)W;
    if (hw > 0 && B > (((int64_t)1 << 31) - 1) / hw) return NBK_ERR_INVALID;      // B * H * W >= 2^31
    if (hw * B > 0 && (depth == nullptr || (q == nullptr && m->d.n_q > 0))) return NBK_ERR_INVALID;
    CloudSel sel;
    { const int32_t rc = cloud_model_begin(m, shape_bits, sel); if (rc != NBK_OK) return rc; }
    const int n_sel = cloud_selected_count(m, sel);
    const int n_list = n_sel + (draw_world != 0 ? m->d.n_wshapes : 0);
    const RenderLds L(n_sel, n_list);
    if (!L.fits()) return NBK_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (counts != nullptr) NBK_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st));
    if (hw * B == 0) return NBK_OK;
    RenderArgs a;
    a.H = H; a.W = W; a.bx = (W + 15) / 16; a.by = (H + 15) / 16;
    a.cam = DepthCam{1.0, fx, fy, cx, cy, z_near, z_far};
    a.eps = eps; a.max_steps = max_steps; a.draw_world = draw_world != 0 ? 1 : 0;
    a.q_one = (Bq == 1 && B != 1) ? 1 : 0; a.t_one = (Bt == 1 && B != 1) ? 1 : 0;
    a.miss = miss;
    const int64_t blocks = (int64_t)a.bx * a.by * B;         // (< 2^31: a block holds a pixel at least)
    hipLaunchKernelGGL(k_render_depth, dim3((unsigned)blocks), dim3(256), L.bytes(), st, m->d, sel, n_sel, m->rs_user,
                       m->movable ? (const int*)m->world_status : (const int*)nullptr, q, T, a, depth, label,
                       reinterpret_cast<unsigned long long*>(counts));
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

// the argument rules the two carving entries share: the frame's, the store and the two parameters of the test
static bool carve_args_ok(const void* depth, int32_t depth_type, int32_t H, int32_t W, const DepthCam& cam, const double* T, double margin,
                          int32_t window, const double* store_pts, int64_t M, const uint8_t* store_keep) {
    if (!frame_args_ok(depth, depth_type, H, W, cam, T)) return false;
    if (!(margin - margin == 0.0) || window < 0 || window > DEPTH_CARVE_MAX_WINDOW) return false;
    return M >= 0 && M <= CLOUD_MAX_POINTS && (M == 0 || (store_pts != nullptr && store_keep != nullptr));
}

int32_t nbk_frame_cloud_carve_host(const void* depth, int32_t depth_type, int32_t H, int32_t W, double depth_scale, double fx, double fy,
                                   double cx, double cy, const double* T, double z_min, double z_max, double margin, int32_t window,
                                   const double* store_pts, int64_t M, uint8_t* store_keep) {
    const DepthCam cam{depth_scale, fx, fy, cx, cy, z_min, z_max};
    if (!carve_args_ok(depth, depth_type, H, W, cam, T, margin, window, store_pts, M, store_keep)) return NBK_ERR_INVALID;
    for (int64_t i = 0; i < M; ++i)
        if (store_keep[i] != 0 && depth_carve_point(cam, T, depth, depth_type, H, W, store_pts + 3 * i, margin, window)) store_keep[i] = 0;
    return NBK_OK;
}

int32_t nbk_frame_cloud_carve(const void* depth, int32_t depth_type, int32_t H, int32_t W, double depth_scale, double fx, double fy,
                              double cx, double cy, const double* T, double z_min, double z_max, double margin, int32_t window,
                              const double* store_pts, int64_t M, uint8_t* store_keep, void* stream) {
    const DepthCam cam{depth_scale, fx, fy, cx, cy, z_min, z_max};
    if (!carve_args_ok(depth, depth_type, H, W, cam, T, margin, window, store_pts, M, store_keep)) return NBK_ERR_INVALID;
    if (nbk_device_count() <= 0) return NBK_ERR_NO_DEVICE;
    if (M == 0 || (int64_t)H * (int64_t)W == 0) return NBK_OK;           // (no image: no window fits, nothing is seen through)
    hipLaunchKernelGGL(k_cloud_carve, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth, (int)depth_type, (int)H,
                       (int)W, cam, T, margin, (int)window, store_pts, (int)M, store_keep);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int32_t nbk_frame_cloud_novel(const nbk_cloud* c, const double* pts, int64_t N, double merge, const uint8_t* held, uint8_t* keep,
                              void* stream) {
    if (c == nullptr || N < 0 || N > CLOUD_MAX_POINTS || merge != merge || (N > 0 && (pts == nullptr || keep == nullptr))) return NBK_ERR_INVALID;
    { const int32_t rc = cloud_check_device(c); if (rc != NBK_OK) return rc; }
    if (N == 0 || !(merge > 0.0)) return NBK_OK;
    hipLaunchKernelGGL(k_cloud_novel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cloud_dev(c), held, pts, (int)N,
                       merge, keep);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int64_t nbk_frame_cloud_append_workspace_bytes(int64_t M, int64_t N) {
    if (M < 1 || M > CLOUD_MAX_POINTS || N < 0 || N > CLOUD_MAX_POINTS) return -1;
    return (int64_t)CloudAppendLayout(M, N).bytes;
}

int32_t nbk_frame_cloud_append(double* store_pts, uint8_t* store_keep, int64_t M, const double* new_pts, const uint8_t* new_keep, int64_t N,
                               int64_t* counts, int32_t* slot_of, void* workspace, int64_t workspace_bytes, void* stream) {
    if (store_pts == nullptr || store_keep == nullptr || counts == nullptr || workspace == nullptr) return NBK_ERR_INVALID;
    if (M < 1 || M > CLOUD_MAX_POINTS || N < 0 || N > CLOUD_MAX_POINTS || (N > 0 && (new_pts == nullptr || new_keep == nullptr))) return NBK_ERR_INVALID;
    const CloudAppendLayout L(M, N);
    if (!cloud_workspace_ok(workspace, workspace_bytes, L.bytes)) return NBK_ERR_INVALID;
    if (nbk_device_count() <= 0) return NBK_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    const CloudAppendLayout::View v = L.view(workspace);
    const int bf = (int)L.bf, ba = (int)L.ba;
    hipLaunchKernelGGL(k_cloud_append_count, dim3((unsigned)(bf + ba)), dim3(256), 0, st, (const uint8_t*)store_keep, (int)M, new_keep, (int)N,
                       bf, v.cnt);
    NBK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, (const unsigned long long*)v.cnt, (int64_t)(bf + ba), v.offs);
    NBK_HIP(hipGetLastError());
    if (N > 0) {
        hipLaunchKernelGGL(k_cloud_append_slots, dim3((unsigned)bf), dim3(256), 0, st, (const uint8_t*)store_keep, (int)M, (int)N,
                           (const unsigned long long*)v.offs, v.slot);
        NBK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_cloud_append_write, dim3((unsigned)(ba > 0 ? ba : 1)), dim3(256), 0, st, new_pts, new_keep, (int)N, (int)M, bf, ba,
                       (const unsigned long long*)v.offs, (const int*)v.slot, store_pts, store_keep, slot_of, reinterpret_cast<long long*>(counts));
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int32_t nbk_cloud_validity_batch(const nbk_model* m, const nbk_cloud* c, const double* q, int64_t B, double threshold,
                                 const uint64_t* shape_bits, int32_t accumulate, uint64_t* mask_bits, uint8_t* mask_bytes, void* stream) {
    if (m == nullptr || c == nullptr || B < 0 || (B > 0 && (q == nullptr || (mask_bits == nullptr && mask_bytes == nullptr)))) return NBK_ERR_INVALID;
    CloudSel sel;
    { const int32_t rc = cloud_call_begin(m, c, shape_bits, sel); if (rc != NBK_OK) return rc; }
    if (B == 0) return NBK_OK;
    if ((B + WAVE - 1) / WAVE > 0x7fffffffLL) return NBK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_cloud_validity, dim3(blocks_for(B)), dim3(WAVE), QSlabLds(m->n_q).bytes(), (hipStream_t)stream, m->d,
                       cloud_dev(c), sel, q, B, threshold, (int)accumulate,
                       reinterpret_cast<unsigned long long*>(mask_bits), mask_bytes);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int32_t nbk_cloud_clearance_batch(const nbk_model* m, const nbk_cloud* c, const double* q, int64_t B, double d_max,
                                  const uint64_t* shape_bits, double* min_dist, int32_t* shape, int32_t* point, void* stream) {
    if (m == nullptr || c == nullptr || B < 0 || !(d_max - d_max == 0.0) || (B > 0 && (q == nullptr || min_dist == nullptr))) return NBK_ERR_INVALID;
    CloudSel sel;
    { const int32_t rc = cloud_call_begin(m, c, shape_bits, sel); if (rc != NBK_OK) return rc; }
    if (B == 0) return NBK_OK;
    if ((B + WAVE - 1) / WAVE > 0x7fffffffLL) return NBK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_cloud_clearance, dim3(blocks_for(B)), dim3(WAVE), QSlabLds(m->n_q).bytes(), (hipStream_t)stream, m->d,
                       cloud_dev(c), sel, m->rs_user, q, B, d_max, min_dist, shape, point);
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int32_t nbk_records_cloud_batch(const nbk_model* m, const nbk_cloud* c, const double* q, int64_t B, double d_max,
                                const uint64_t* shape_bits, int32_t per_shape, double* dist, int32_t* shape, int32_t* point,
                                double* witness, double* jrows, void* stream) {
    // (nothing below dereferences m or c before the argument rules are through and B is known to be positive)
    if (m == nullptr || c == nullptr || B < 0 || !(d_max - d_max == 0.0) || (B > 0 && (q == nullptr || dist == nullptr))) return NBK_ERR_INVALID;
    if (B == 0) return NBK_OK;
    CloudSel sel;
    int n_sel = 0;
    { const int32_t rc = cloud_call_begin(m, c, shape_bits, sel, &n_sel); if (rc != NBK_OK) return rc; }
    if ((B + WAVE - 1) / WAVE > 0x7fffffffLL) return NBK_ERR_UNSUPPORTED;
    const size_t lds = PairItemsLds(m->n_q, jrows != nullptr ? m->n_joints : 0).bytes();
    if (per_shape) {
        if (n_sel == 0) return NBK_OK;                       // no column: nothing is written
        hipLaunchKernelGGL(k_cloud_records<true>, dim3(blocks_for(B), (unsigned)n_sel), dim3(WAVE), lds, (hipStream_t)stream, m->d,
                           cloud_dev(c), sel, m->rs_user, q, B, d_max, n_sel, dist, shape, point, witness, jrows);
    } else {
        hipLaunchKernelGGL(k_cloud_records<false>, dim3(blocks_for(B)), dim3(WAVE), lds, (hipStream_t)stream, m->d, cloud_dev(c), sel,
                           m->rs_user, q, B, d_max, n_sel, dist, shape, point, witness, jrows);
    }
    NBK_HIP(hipGetLastError());
    return NBK_OK;
}

int64_t nbk_edge_cloud_workspace_bytes(int64_t E) { return edge_workspace_bytes(E); }

int32_t nbk_edge_cloud_validity_batch(const nbk_model* m, const nbk_cloud* c, const double* starts, const double* goals, const double* dist,
                                      int64_t E, double resolution, double max_distance, int32_t mode, double threshold,
                                      const uint64_t* shape_bits, int32_t accumulate, uint8_t* valid, double* end, int32_t* n_samples,
                                      void* workspace, int64_t workspace_bytes, void* stream) {
    if (m == nullptr || c == nullptr) return NBK_ERR_INVALID;
    CloudSel sel;
    return sampled_edges_call(
        m, starts, goals, dist, E, resolution, max_distance, mode, threshold, accumulate, valid, end, n_samples, workspace, workspace_bytes,
        stream, [&] { return cloud_call_begin(m, c, shape_bits, sel); },
        [&](dim3 grid, size_t lds, hipStream_t st, const EdgeSrc& es, const unsigned long long* offs) {
            hipLaunchKernelGGL(k_cloud_edges, grid, dim3(WAVE), lds, st, m->d, cloud_dev(c), sel, es, offs, E, threshold, valid);
        });
}

int32_t nbk_edge_cloud_continuous_batch(const nbk_model* m, const nbk_cloud* c, const double* starts, const double* goals, const double* dist,
                                        int64_t E, double max_distance, int32_t mode, double threshold, int32_t max_iter, double slack,
                                        double look_ahead, const uint64_t* shape_bits, int32_t accumulate, uint8_t* valid, double* end,
                                        double* t_free, int32_t* status, void* stream) {
    if (m == nullptr || c == nullptr) return NBK_ERR_INVALID;
    CloudSel sel;
    int n_sel = 0;                                  // one row of workgroups per selected shape
    return certified_edges_call(
        m, starts, goals, dist, E, max_distance, mode, threshold, max_iter, slack, &look_ahead, &n_sel, false, cloud_status_word(c), nullptr,
        nullptr, accumulate, valid, end, t_free, status, stream, [&] { return cloud_call_begin(m, c, shape_bits, sel, &n_sel); },
        [&](hipStream_t st) {
            hipLaunchKernelGGL(k_cloud_edge_ca, dim3(blocks_for(E), (unsigned)n_sel), dim3(WAVE), QSlabLds(m->n_q).bytes(), st, m->d, cloud_dev(c),
                               sel, m->rs_user, starts, goals, dist, E, max_distance, (int)mode, threshold, (int)max_iter, slack, look_ahead,
                               ca_keys(t_free));
        });
}

int64_t nbk_spline_cloud_workspace_bytes(int64_t S) { return spline_workspace_bytes(S); }

int32_t nbk_spline_cloud_validity_batch(const nbk_model* m, const nbk_cloud* c, const double* ctrl, int64_t S, int32_t n_ctrl, int32_t degree,
                                        const double* knots, double resolution, double threshold, const uint64_t* shape_bits,
                                        int32_t accumulate, uint8_t* valid, double* t_hit, int32_t* n_samples, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
    if (m == nullptr || c == nullptr) return NBK_ERR_INVALID;
    CloudSel sel;
    return sampled_splines_call(
        m, ctrl, S, n_ctrl, degree, knots, resolution, threshold, cloud_status_word(c), accumulate, valid, t_hit, n_samples, workspace,
        workspace_bytes, stream, [&] { return cloud_call_begin(m, c, shape_bits, sel); },
        [&](auto K, dim3 grid, size_t lds, hipStream_t st, const SplineCloudLayout::View& v, const double* t_prev) {
            hipLaunchKernelGGL(k_cloud_spline<decltype(K)::value>, grid, dim3(WAVE), lds, st, m->d, cloud_dev(c), sel, ctrl, (int)n_ctrl, knots,
                               (const double*)v.plan, (const unsigned long long*)v.offs, S, threshold, t_prev, v.first);
        });
}

int32_t nbk_spline_cloud_continuous_batch(const nbk_model* m, const nbk_cloud* c, const double* ctrl, int64_t S, int32_t n_ctrl,
                                          int32_t degree, const double* knots, double threshold, int32_t max_iter, double slack,
                                          double look_ahead, const uint64_t* shape_bits, int32_t accumulate, uint8_t* valid,
                                          double* t_free, int32_t* status, void* stream) {
    if (m == nullptr || c == nullptr) return NBK_ERR_INVALID;
    CloudSel sel;
    int n_sel = 0;
    return certified_splines_call(
        m, ctrl, S, n_ctrl, degree, knots, threshold, max_iter, slack, &look_ahead, &n_sel, false, cloud_status_word(c), nullptr, nullptr,
        accumulate, valid, t_free, status, stream, [&] { return cloud_call_begin(m, c, shape_bits, sel, &n_sel); },
        [&](auto K, size_t lds, hipStream_t st) {
            hipLaunchKernelGGL(k_cloud_spline_ca<decltype(K)::value>, dim3(blocks_for(S), (unsigned)n_sel), dim3(WAVE), lds, st, m->d,
                               cloud_dev(c), sel, m->rs_user, ctrl, S, (int)n_ctrl, knots, threshold, (int)max_iter, slack, look_ahead,
                               ca_keys(t_free));
        });
}

}  // extern "C"
