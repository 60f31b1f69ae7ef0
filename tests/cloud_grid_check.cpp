// Stand-alone check of numbotics_amd/csrc/nbk_cloud_grid.hpp (the cell arithmetic of the point-cloud grid), built by
// tests/test_cloud_grid_host.py with g++ -fsanitize=address,undefined and run as a child process.  It includes that header alone.
//
// What it sweeps (random grids: cell sizes 1e-3 .. 1e3 log-uniform, dims 1 .. 64 per axis, lo anywhere in +-1e3 cells) and holds:
//   - cloud_coord is clamped to [0, dim - 1], nondecreasing in x, and equals the unclamped floor((x - lo) / cell) inside the box;
//     coordinates exactly lo + k * cell land in cell k;
//   - every point p with |p - c| <= R (float64 per-axis differences, and points that pass the predicate's sum-of-squares test
//     fl(|c - p|^2) < fl(R^2)) lies in cloud_cell_range(c, R) -- points outside the box and points on cell boundaries included;
//   - R = 0, negative or NaN gives an empty range; R = 1e300 or infinite the whole grid; a NaN centre one cell;
//   - every range is clamped (0 <= lo <= hi <= dim - 1 when not empty);
//   - cloud_grid_valid refuses what nbk_cloud_create must refuse.
// Last line of the output: "<checks> checks, <failed> failed".
#include "../numbotics_amd/csrc/nbk_cloud_grid.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <random>

using namespace nbk;

static long long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        ++g_checks;                                              \
        if (!(cond)) {                                           \
            if (++g_failed <= 20) { printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                        \
    } while (0)

static bool in_range(const CloudGrid& g, const double* p, const int* lo, const int* hi) {
    for (int a = 0; a < 3; ++a) {
        const int c = cloud_coord(p[a], g.lo[a], g.cell, g.dims[a]);
        if (c < lo[a] || c > hi[a]) return false;
    }
    return true;
}

int main() {
    std::mt19937_64 rng(20240611);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    for (int trial = 0; trial < 400; ++trial) {
        CloudGrid g;
        g.cell = pow(10.0, -3.0 + 6.0 * U(rng));
        for (int a = 0; a < 3; ++a) {
            g.dims[a] = 1 + (int)(U(rng) * 64.0);
            g.lo[a] = (trial % 7 == 0) ? 0.0 : (2.0 * U(rng) - 1.0) * 1e3 * g.cell;
        }
        if (trial % 11 == 0) g.dims[0] = g.dims[1] = g.dims[2] = 1;
        CHECK(cloud_grid_valid(g.lo, g.cell, g.dims), "grid");
        const double ext[3] = {g.cell * g.dims[0], g.cell * g.dims[1], g.cell * g.dims[2]};

        // the coordinate rule
        for (int a = 0; a < 3; ++a) {
            for (int k = 0; k < 40; ++k) {
                const double x = g.lo[a] + (U(rng) * 1.5 - 0.25) * ext[a];
                const int c = cloud_coord(x, g.lo[a], g.cell, g.dims[a]);
                CHECK(c >= 0 && c < g.dims[a], "coord %d of %d", c, g.dims[a]);
                const double f = floor((x - g.lo[a]) / g.cell);
                if (f >= 0.0 && f <= (double)(g.dims[a] - 1)) CHECK(c == (int)f, "inside: %d vs %g", c, f);
                else CHECK(c == (f < 0.0 ? 0 : g.dims[a] - 1), "clamped: %d for %g", c, f);
                const double x2 = x + U(rng) * g.cell;
                CHECK(cloud_coord(x2, g.lo[a], g.cell, g.dims[a]) >= c, "monotone");
            }
            // monotone on a sorted ladder that straddles both borders, with the exact multiples of the cell in it
            int last = 0;
            for (int k = -3; k <= g.dims[a] + 3; ++k) {
                const double x = g.lo[a] + (double)k * g.cell;
                const int c = cloud_coord(x, g.lo[a], g.cell, g.dims[a]);
                CHECK(c >= last, "ladder %d: %d after %d", k, c, last);
                last = c;
                if (g.lo[a] == 0.0) {        // x = k * cell exactly: (x - 0) / cell is k or its correctly rounded neighbour's floor
                    const double f = floor(x / g.cell);
                    const int want = f < 0.0 ? 0 : (f > (double)(g.dims[a] - 1) ? g.dims[a] - 1 : (int)f);
                    CHECK(c == want, "multiple %d: %d vs %d", k, c, want);
                }
                const double xm = nextafter(x, -inf), xp = nextafter(x, inf);
                CHECK(cloud_coord(xm, g.lo[a], g.cell, g.dims[a]) <= c && cloud_coord(xp, g.lo[a], g.cell, g.dims[a]) >= c, "neighbours of a boundary");
            }
            CHECK(cloud_coord(-inf, g.lo[a], g.cell, g.dims[a]) == 0, "-inf");
            CHECK(cloud_coord(inf, g.lo[a], g.cell, g.dims[a]) == g.dims[a] - 1, "+inf");
            CHECK(cloud_coord(nan, g.lo[a], g.cell, g.dims[a]) == 0, "NaN");
        }

        // ranges
        for (int k = 0; k < 30; ++k) {
            double c[3];
            for (int a = 0; a < 3; ++a) c[a] = g.lo[a] + (U(rng) * 1.6 - 0.3) * ext[a];      // centres inside and outside the box
            if (k % 5 == 0) for (int a = 0; a < 3; ++a) c[a] = g.lo[a] + (double)(int)(U(rng) * (g.dims[a] + 1)) * g.cell;   // on boundaries
            const double R = g.cell * pow(10.0, -2.0 + 3.5 * U(rng));
            int lo[3], hi[3];
            CHECK(cloud_cell_range(g, c, R, lo, hi), "non-empty");
            for (int a = 0; a < 3; ++a) CHECK(0 <= lo[a] && lo[a] <= hi[a] && hi[a] <= g.dims[a] - 1, "clamped range [%d, %d] of %d", lo[a], hi[a], g.dims[a]);
            CHECK(in_range(g, c, lo, hi), "the centre itself");
            for (int j = 0; j < 12; ++j) {
                double p[3];
                // a direction and a length up to R: the extremes (axis-aligned, exactly R) every third time
                double d[3] = {2.0 * U(rng) - 1.0, 2.0 * U(rng) - 1.0, 2.0 * U(rng) - 1.0};
                if (j % 3 == 0) { d[0] = d[1] = d[2] = 0.0; d[(j / 3) % 3] = (j & 4) ? 1.0 : -1.0; }
                const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                if (!(n > 0.0)) continue;
                const double len = (j % 3 == 0) ? R : R * U(rng);
                for (int a = 0; a < 3; ++a) p[a] = c[a] + d[a] / n * len;
                if (j % 4 == 1) for (int a = 0; a < 3; ++a) p[a] = g.lo[a] + floor((p[a] - g.lo[a]) / g.cell) * g.cell;    // snapped to a cell boundary
                // is p within R of c, by the per-axis float64 differences and by the predicate's own accumulation?
                const double e0 = c[0] - p[0], e1 = c[1] - p[1], e2 = c[2] - p[2];
                const bool axes = fabs(e0) <= R && fabs(e1) <= R && fabs(e2) <= R && sqrt(e0 * e0 + e1 * e1 + e2 * e2) <= R;
                const bool pred = fma(e2, e2, fma(e1, e1, e0 * e0)) < R * R;
                if (axes || pred) CHECK(in_range(g, p, lo, hi), "point (%.17g %.17g %.17g) of ball (%.17g %.17g %.17g; %.17g), cell %.17g", p[0], p[1], p[2], c[0], c[1], c[2], R, g.cell);
            }
            // degenerate radii
            const double bad[4] = {0.0, -R, nan, -inf};
            for (double r : bad) {
                CHECK(!cloud_cell_range(g, c, r, lo, hi), "R = %g is empty", r);
                for (int a = 0; a < 3; ++a) CHECK(lo[a] > hi[a], "empty range");
            }
            const double huge[2] = {1e300, inf};
            for (double r : huge) {
                CHECK(cloud_cell_range(g, c, r, lo, hi), "R = %g", r);
                for (int a = 0; a < 3; ++a) CHECK(lo[a] == 0 && hi[a] == g.dims[a] - 1, "whole grid: [%d, %d] of %d", lo[a], hi[a], g.dims[a]);
            }
            const double cn[3] = {nan, c[1], nan};
            CHECK(cloud_cell_range(g, cn, R, lo, hi), "NaN centre");
            for (int a = 0; a < 3; ++a) CHECK(0 <= lo[a] && lo[a] <= hi[a] && hi[a] <= g.dims[a] - 1, "NaN centre: bounded");
            CHECK(lo[0] == 0 && hi[0] == 0 && lo[2] == 0 && hi[2] == 0, "NaN centre: one cell on its axes");
        }
    }

    // what nbk_cloud_create refuses
    {
        const double lo[3] = {0, 0, 0};
        const int d1[3] = {4, 4, 4}, d0[3] = {4, 0, 4}, dbig[3] = {256, 256, 65}, dmax[3] = {256, 256, 64}, dneg[3] = {-1, 4, 4};
        const double lnan[3] = {0, nan, 0}, linf[3] = {inf, 0, 0};
        CHECK(cloud_grid_valid(lo, 0.1, d1), "plain");
        CHECK(cloud_grid_valid(lo, 0.1, dmax), "2^22 cells");
        CHECK(!cloud_grid_valid(lo, 0.1, dbig), "more than 2^22 cells");
        CHECK(!cloud_grid_valid(lo, 0.1, d0) && !cloud_grid_valid(lo, 0.1, dneg), "dims below 1");
        CHECK(!cloud_grid_valid(lo, 0.0, d1) && !cloud_grid_valid(lo, -1.0, d1) && !cloud_grid_valid(lo, nan, d1), "cell");
        CHECK(!cloud_grid_valid(lnan, 0.1, d1) && !cloud_grid_valid(linf, 0.1, d1), "lo");
        CHECK(!cloud_grid_valid(nullptr, 0.1, d1) && !cloud_grid_valid(lo, 0.1, nullptr), "null");
        const CloudGrid g{{0, 0, 0}, 0.5, {3, 4, 5}};
        const double p[3] = {1.2, 0.1, 2.4};     // x 2, y 0, z 4
        CHECK(cloud_cell(g, p) == (4 * 4 + 0) * 3 + 2, "cell index, x fastest");
    }

    printf("%lld checks, %lld failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
