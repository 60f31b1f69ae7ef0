// nbk_cloud_grid.hpp -- the cell arithmetic of the point-cloud grid (nbk_cloud.hpp; DESIGN.md 3, "Point clouds"), shared by the device
// kernels, the host entry nbk_cloud_cells_host and tests/cloud_grid_check.cpp, which includes this file alone: no kernel, no device
// type or call, nothing of the project.  Every function carries NBK_GRID_FN, which the includer may define before the include (the
// library makes the functions callable from both sides with it); alone it is `inline`.
//
// A grid is lo[3], cell > 0 and dims[3] (each >= 1, product <= 2^22).  The coordinate of x on an axis is
//     floor((x - lo) / cell)      in float64, clamped to [0, dim - 1]
// so points outside the box land in the border cells; none is dropped.  (A NaN x has coordinate 0: the cloud's status is set for such
// a point and nothing is read from the grid while it is.)  Cells are numbered x fastest: (z * dims[1] + y) * dims[0] + x.
//
// The range of a ball, and why it is sound.  A query visits, per axis, the cells cloud_coord(L) .. cloud_coord(H) with
//     pad = R + 2^-40 (R + |c|),   L = c - pad,   H = c + pad          (every operation rounded to float64)
// Claim: a point p whose float64 difference d = fl(c - p) (or fl(p - c): the same magnitude) satisfies |d| < R on this axis has
// L <= p <= H.  Proof for L: suppose p < L.  Rounding is monotone and R is a float64, so it suffices that the exact c - p exceeds R:
//     c - p > c - L = c - fl(c - pad) >= pad - 2^-53 |c - pad| >= pad - 2^-53 (|c| + pad),
// and pad >= R + (2^-40 - 2^-51)(R + |c|) after its own three roundings, so c - p > R + (2^-41 - 2^-52)(R + |c|) > R: then
// fl(c - p) >= R, a contradiction.  H likewise.  The pair predicate's bounding-sphere step (nbk_device.hpp, item 2) lets a point pass
// only when fl(|cA - p|^2) < fl(R^2) with the sum of squares accumulated from non-negative terms by fused multiply-adds: the
// accumulated value is at least fl(d^2) of any one axis, and fl(d^2) < fl(R^2) implies |d| < R because squaring and rounding are
// monotone on non-negative numbers -- overflow and underflow included.  So every point that step does not answer "free" lies in
// [L, H] on every axis; and x -> cloud_coord(x) is nondecreasing (subtraction of lo, division by a positive cell, floor and the clamp
// all are, with their roundings), so its cell lies in the range.  The same holds for every p with |p - c| <= R in exact arithmetic.
// R <= 0 or NaN gives an empty range (lo > hi); an infinite or huge R gives 0 .. dim - 1; a NaN centre gives cell 0 alone: the walk
// over a range is always bounded by the grid, and the points it meets by N.
#ifndef NBK_CLOUD_GRID_HPP
#define NBK_CLOUD_GRID_HPP
#include <math.h>
#include <stdint.h>

#ifndef NBK_GRID_FN
#define NBK_GRID_FN inline
#endif

namespace nbk {

constexpr int64_t CLOUD_MAX_CELLS = int64_t(1) << 22;
constexpr int64_t CLOUD_MAX_POINTS = int64_t(1) << 24;

struct CloudGrid {
    double lo[3];
    double cell;
    int dims[3];
};

// the argument rules of nbk_cloud_create for the grid: a finite lo, a positive cell (not NaN), dims >= 1 with a product of at
// most CLOUD_MAX_CELLS
NBK_GRID_FN bool cloud_grid_valid(const double* lo, double cell, const int* dims) {
    if (lo == nullptr || dims == nullptr) return false;
    if (!(cell > 0.0)) return false;
    int64_t n = 1;
    for (int a = 0; a < 3; ++a) {
        if (!(lo[a] - lo[a] == 0.0)) return false;          // NaN or infinite
        if (dims[a] < 1) return false;
        n *= (int64_t)dims[a];
        if (n > CLOUD_MAX_CELLS) return false;
    }
    return true;
}

NBK_GRID_FN int cloud_coord(double x, double lo, double cell, int dim) {
    const double f = floor((x - lo) / cell);
    if (!(f >= 0.0)) return 0;                              // below the box, or NaN
    if (f >= (double)(dim - 1)) return dim - 1;
    return (int)f;
}

NBK_GRID_FN int cloud_cell(const CloudGrid& g, const double* p) {
    const int x = cloud_coord(p[0], g.lo[0], g.cell, g.dims[0]);
    const int y = cloud_coord(p[1], g.lo[1], g.cell, g.dims[1]);
    const int z = cloud_coord(p[2], g.lo[2], g.cell, g.dims[2]);
    return (z * g.dims[1] + y) * g.dims[0] + x;
}

// clamped inclusive cell range of the ball |x - centre| <= R, padded as argued above; returns false (and lo > hi) when it is empty
NBK_GRID_FN bool cloud_cell_range(const CloudGrid& g, const double* centre, double R, int* lo_out, int* hi_out) {
    if (!(R > 0.0)) {
        for (int a = 0; a < 3; ++a) { lo_out[a] = 0; hi_out[a] = -1; }
        return false;
    }
    for (int a = 0; a < 3; ++a) {
        const double c = centre[a];
        const double pad = R + 0x1p-40 * (R + fabs(c));
        lo_out[a] = cloud_coord(c - pad, g.lo[a], g.cell, g.dims[a]);
        hi_out[a] = cloud_coord(c + pad, g.lo[a], g.cell, g.dims[a]);
        if (hi_out[a] < lo_out[a]) hi_out[a] = lo_out[a];   // a NaN centre: both ends are cell 0 already; kept for the reader
    }
    return true;
}

}  // namespace nbk
#endif
