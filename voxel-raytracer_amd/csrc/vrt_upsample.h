// vrt_upsample.h -- the arguments of the upsampling pass's kernel (vrt_upsample.hip.h, include/vrt.h vrt_upsample_hdr), shared by the
// host side (vrt_upsample.cpp) and the launch file (vrt_launch_upsample.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vrt {
namespace upsample {

struct Args {
    // the LOW image and its planes, width x height
    const float *rgb;        // 3 floats per pixel
    const float *normal;     // 3
    const float *albedo;     // 4
    const float *depth;      // 1
    const float *coverage;   // 1
    // the HIGH planes, (factor * width) x (factor * height)
    const float *hi_normal, *hi_albedo, *hi_depth, *hi_coverage;
    float *out_rgb;            // high, 3 floats per pixel; may be null
    uint32_t *out_rgba;        // high, the tone-mapped bytes; may be null
    uint8_t *out_unresolved;   // high, one byte per pixel; may be null
    int width, height;         // LOW
    int factor;                // r, the same in every lane
    uint32_t demodulate;       // 0 or 1
    float kn, ka;              // 1 / sigma_normal^2, 1 / sigma_albedo^2, from the host
    float sigma_depth, min_weight;
    float offset_lo_x, offset_lo_y, offset_hi_x, offset_hi_y;
    int op;                    // VRT_TONEMAP_*
    float exposure;
};

}  // namespace upsample
}  // namespace vrt
