// nbk_cloud_depth.hpp -- one pixel of a depth image to a world point (nbk_cloud.hpp, k_cloud_backproject; DESIGN.md 3, "Point clouds"),
// shared by the device kernel and the host entry nbk_frame_cloud_backproject_host, as nbk_cloud_grid.hpp shares the cell arithmetic: no
// kernel, no device type or call, nothing of the project.  Every function carries NBK_GRID_FN (see nbk_cloud_grid.hpp).
//
// The camera is a pinhole in its OPTICAL frame (z forward, x right, y down): pixel (u, v) of depth z -- the metric depth along the
// view axis, not the range along the ray -- is the camera point ((u - cx) z / fx, (v - cy) z / fy, z).  T[3][4] is the optical
// frame's pose in the world.  The arithmetic contract, in float64 without contraction (the library is built with -ffp-contract=off),
// every operation rounded once, in exactly this order:
//     z  = (double)d * depth_scale                    d: the float32 value or the uint16 raw units of the pixel
//     xc = (((double)u - cx) * z) / fx
//     yc = (((double)v - cy) * z) / fy
//     w[e] = ((T[e][0] * xc + T[e][1] * yc) + T[e][2] * z) + T[e][3]
// A pixel is valid iff z - z == 0 (finite), z > z_min and z <= z_max; an invalid pixel (a hole: 0, NaN, out of range) has no point.
//
// The way back, for free-space carving (k_cloud_carve, nbk_frame_cloud_carve_host; DESIGN.md 3, "Fused frames"): a stored world point p
// is SEEN THROUGH by a frame when the frame measures a surface behind it at every pixel around its projection.  Same contract:
//     d[e] = p[e] - T[e][3]
//     xc = (T[0][0] * d[0] + T[1][0] * d[1]) + T[2][0] * d[2]       (R^T d: T's rotation is taken to be orthonormal, not checked;
//     yc, zc likewise with columns 1 and 2                            columns 0, 1, 2 of T give xc, yc, zc)
//     u = floor(((xc * fx) / zc + cx) + 0.5)      v = floor(((yc * fy) / zc + cy) + 0.5)                   (kept as doubles)
// p is seen through iff zc > z_min, the window u - w .. u + w, v - w .. v + w lies in the image (compared as doubles: NaN and huge
// values fall out) and every pixel of it is valid by the test above with (z - zc) > margin.  A hole in the window is no evidence.
//
// The ray side, for rendered frames (k_render_depth, nbk_render_ray_spans_host; DESIGN.md 3, "Rendered frames").  The point at depth z
// on pixel (u, v) is depth_backproject_pixel with depth_scale = 1 and no range (depth_ray_point): what a renderer tests at z is the
// point the back-projection later makes from that depth.  Per unit of depth the ray is L long (T's rotation taken as orthonormal, as
// above); the depths at which the pixel's ray is inside the ball (c, R), clipped to [z_near, z_far] (depth_ray_sphere_span):
//     ax = ((double)u - cx) / fx      ay = ((double)v - cy) / fy
//     A = (ax * ax + ay * ay) + 1     L = sqrt(A)
//     d[e] = c[e] - T[e][3];  xc, yc, zc = R^T d as for carving
//     B = (ax * xc + ay * yc) + zc    C = ((xc * xc + yc * yc) + zc * zc) - R * R
//     D = B * B - A * C               empty unless D >= 0 (a NaN is empty)
//     s = sqrt(D)     z0 = (B - s) / A     z1 = (B + s) / A
//     z0 = z0 > z_near ? z0 : z_near       z1 = z1 < z_far ? z1 : z_far       the span is [z0, z1], empty unless z0 <= z1
#ifndef NBK_CLOUD_DEPTH_HPP
#define NBK_CLOUD_DEPTH_HPP
#include <math.h>
#include <stdint.h>

#ifndef NBK_GRID_FN
#define NBK_GRID_FN inline
#endif

namespace nbk {

struct DepthCam { double depth_scale, fx, fy, cx, cy, z_min, z_max; };

// the argument rules of the back-projection entries for the camera: positive (not NaN) focal lengths and depth scale
NBK_GRID_FN bool depth_cam_valid(const DepthCam& k) { return k.fx > 0.0 && k.fy > 0.0 && k.depth_scale > 0.0; }

// the depth of pixel i of an image of `depth_type` 0 (float32) or 1 (uint16 raw units), as a double (exact either way)
NBK_GRID_FN double depth_pixel_value(const void* depth, int depth_type, int64_t i) {
    return depth_type == 0 ? (double)static_cast<const float*>(depth)[i] : (double)static_cast<const uint16_t*>(depth)[i];
}

// the validity test of a metric depth z: finite and in (z_min, z_max]
NBK_GRID_FN bool depth_z_valid(const DepthCam& k, double z) { return (z - z == 0.0) && z > k.z_min && z <= k.z_max; }

// pixel (u, v) of raw depth d -> its world point in w and true, or (0, 0, 0) and false for a hole
NBK_GRID_FN bool depth_backproject_pixel(const DepthCam& k, const double* T, int u, int v, double d, double* w) {
    const double z = d * k.depth_scale;
    const bool valid = depth_z_valid(k, z);
    if (!valid) {
        w[0] = 0.0; w[1] = 0.0; w[2] = 0.0;
        return false;
    }
    const double xc = (((double)u - k.cx) * z) / k.fx;
    const double yc = (((double)v - k.cy) * z) / k.fy;
    for (int e = 0; e < 3; ++e) w[e] = ((T[4 * e] * xc + T[4 * e + 1] * yc) + T[4 * e + 2] * z) + T[4 * e + 3];
    return true;
}

// the march point of pixel (u, v) at depth z: depth_backproject_pixel's point for depth_scale 1, whatever the range (k: fx, fy, cx, cy)
NBK_GRID_FN void depth_ray_point(const DepthCam& k, const double* T, int u, int v, double z, double* w) {
    const double xc = (((double)u - k.cx) * z) / k.fx;
    const double yc = (((double)v - k.cy) * z) / k.fy;
    for (int e = 0; e < 3; ++e) w[e] = ((T[4 * e] * xc + T[4 * e + 1] * yc) + T[4 * e + 2] * z) + T[4 * e + 3];
}

// the length of pixel (u, v)'s ray per unit of depth
NBK_GRID_FN double depth_ray_length(const DepthCam& k, int u, int v) {
    const double ax = ((double)u - k.cx) / k.fx, ay = ((double)v - k.cy) / k.fy;
    return sqrt((ax * ax + ay * ay) + 1.0);
}

// the depths [z0, z1] within [z_near, z_far] at which pixel (u, v)'s ray is inside the ball (c, R); false (z0, z1 untouched): none
NBK_GRID_FN bool depth_ray_sphere_span(const DepthCam& k, const double* T, int u, int v, const double* c, double R, double z_near,
                                       double z_far, double* z0, double* z1) {
    const double ax = ((double)u - k.cx) / k.fx, ay = ((double)v - k.cy) / k.fy;
    const double A = (ax * ax + ay * ay) + 1.0;
    const double d0 = c[0] - T[3], d1 = c[1] - T[7], d2 = c[2] - T[11];
    const double xc = (T[0] * d0 + T[4] * d1) + T[8] * d2;
    const double yc = (T[1] * d0 + T[5] * d1) + T[9] * d2;
    const double zc = (T[2] * d0 + T[6] * d1) + T[10] * d2;
    const double B = (ax * xc + ay * yc) + zc;
    const double C = ((xc * xc + yc * yc) + zc * zc) - R * R;
    const double D = B * B - A * C;
    if (!(D >= 0.0)) return false;
    const double s = sqrt(D);
    double a = (B - s) / A, b = (B + s) / A;
    a = a > z_near ? a : z_near;
    b = b < z_far ? b : z_far;
    if (!(a <= b)) return false;
    *z0 = a; *z1 = b;
    return true;
}

constexpr int DEPTH_CARVE_MAX_WINDOW = 8;

// is the world point p seen through by the (H, W) image at pose T?  (0 <= window <= DEPTH_CARVE_MAX_WINDOW: the caller's rule; every
// pixel read lies in the image by the window test, whatever p holds)
NBK_GRID_FN bool depth_carve_point(const DepthCam& k, const double* T, const void* depth, int depth_type, int H, int W, const double* p,
                                   double margin, int window) {
    const double d0 = p[0] - T[3], d1 = p[1] - T[7], d2 = p[2] - T[11];
    const double xc = (T[0] * d0 + T[4] * d1) + T[8] * d2;
    const double yc = (T[1] * d0 + T[5] * d1) + T[9] * d2;
    const double zc = (T[2] * d0 + T[6] * d1) + T[10] * d2;
    if (!(zc > k.z_min)) return false;
    const double u = floor(((xc * k.fx) / zc + k.cx) + 0.5);
    const double v = floor(((yc * k.fy) / zc + k.cy) + 0.5);
    const double w = (double)window;
    if (!(u - w >= 0.0 && u + w <= (double)(W - 1) && v - w >= 0.0 && v + w <= (double)(H - 1))) return false;
    const int u0 = (int)u - window, v0 = (int)v - window, side = 2 * window + 1;
    for (int b = 0; b < side; ++b)
        for (int a = 0; a < side; ++a) {
            const double z = depth_pixel_value(depth, depth_type, (int64_t)(v0 + b) * W + (u0 + a)) * k.depth_scale;
            if (!depth_z_valid(k, z) || !((z - zc) > margin)) return false;
        }
    return true;
}

}  // namespace nbk
#endif
