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
#ifndef NBK_CLOUD_DEPTH_HPP
#define NBK_CLOUD_DEPTH_HPP
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

// pixel (u, v) of raw depth d -> its world point in w and true, or (0, 0, 0) and false for a hole
NBK_GRID_FN bool depth_backproject_pixel(const DepthCam& k, const double* T, int u, int v, double d, double* w) {
    const double z = d * k.depth_scale;
    const bool valid = (z - z == 0.0) && z > k.z_min && z <= k.z_max;
    if (!valid) {
        w[0] = 0.0; w[1] = 0.0; w[2] = 0.0;
        return false;
    }
    const double xc = (((double)u - k.cx) * z) / k.fx;
    const double yc = (((double)v - k.cy) * z) / k.fy;
    for (int e = 0; e < 3; ++e) w[e] = ((T[4 * e] * xc + T[4 * e + 1] * yc) + T[4 * e + 2] * z) + T[4 * e + 3];
    return true;
}

}  // namespace nbk
#endif
