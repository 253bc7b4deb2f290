// vrt_temporal.h -- the arguments of the temporal pass's kernel (vrt_temporal.hip.h, include/vrt.h vrt_temporal_hdr), shared by the
// host side (vrt_temporal.cpp) and the launch file (vrt_launch_temporal.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vrt {
namespace temporal {

// A history: three row-major planes of 16-byte words in one buffer, plane k at word k * W * H (include/vrt.h), so that a wave's
// taps and stores move whole words.
//   plane 0  r, g, b, N
//   plane 1  m1, m2, Z, coverage
//   plane 2  nx, ny, nz, +0 (vrt_temporal_hdr) or V, the measured variance of the integrated mean (vrt_temporal_hdr_mom, T7)
constexpr size_t kHistoryBytes = 48;

struct Args {
    const float *rgb;           // this frame's image, 3 floats per pixel
    const float *normal;        // 3
    const float *depth;         // 1
    const float *coverage;      // 1
    const float4 *history_in;   // null: the first frame, no pixel has a history and prev_* are not read
    float4 *history_out;
    float *out_rgb;             // the integrated colour, 3 floats per pixel; may be null
    float *out_variance;        // T6's variance; may be null
    int width, height;
    float inv_proj[16], inv_view[16], cam_pos[3];   // this frame's camera block
    float prev_view_proj[16], prev_cam_pos[3];      // the previous frame's
    float offset_x, offset_y;
    float max_history;          // (float)vrt_temporal::max_history, exact up to 32768
    float alpha_min, alpha_moments_min, normal_min, depth_tol;
};

// vrt_temporal_hdr_mom's: the same, then T7's input and T6m's and T3s's switches
struct ArgsMom : Args {
    const float *variance_in;   // this frame's measured variance, 1 float per pixel; null: unknown, 65504^2 everywhere
    float measured_below;       // (float)vrt_temporal_mom::measured_below, exact up to 32769
    int search;                 // 0 or 1
};

}  // namespace temporal
}  // namespace vrt
