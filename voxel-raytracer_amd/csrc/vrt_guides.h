// vrt_guides.h -- the arguments of the guide-plane kernels (vrt_guides.hip.h), shared by the host side (vrt_guides.cpp) and the
// launch file (vrt_launch_guides.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/vrt.h"   // VRT_GUIDE_MAX_SURFACES

namespace vrt {
namespace guides {

// The guide state of an accumulation (include/vrt.h vrt_accum_guides), 40 bytes per pixel in three row-major planes of one buffer,
// so that a wave reads and writes whole 16- and 8-byte words side by side:
//   albedo  uint32[4] per pixel   the sums of the surface colour's R, G, B, A bytes
//   normal  int32[3] + uint32     the signed sums of the normal's three components, then the number of hits
//   depth   double                the sum of h(depth), one add per sample in sample order
// 255 * 2^24 < 2^32: every integer sum is exact up to the accumulation's 2^24 samples.
constexpr size_t kStateBytes = 40;
struct State {
    uint4 *albedo;
    int4 *normal;
    double *depth;
};
inline State state_of(void *base, size_t pixels) {
    char *p = static_cast<char *>(base);
    return State{reinterpret_cast<uint4 *>(p), reinterpret_cast<int4 *>(p + pixels * 16), reinterpret_cast<double *>(p + pixels * 32)};
}

// One launch of guide_kernel over a frame: samples first .. first + n - 1 of every pixel go into the state
struct Args {
    State st;
    uint32_t first, n;
};

// guide_resolve_kernel: the state of n samples -> the four float planes (any may be null)
struct Resolve {
    State st;
    float *normal;       // 3 floats per pixel
    float *albedo;       // 4 floats per pixel
    float *depth;        // 1
    float *coverage;     // 1
    uint32_t n;          // samples in the state (>= 1)
    uint32_t pixels;
};

// guide_kernel over a caller's ray batch (include/vrt.h vrt_guide_rays): the rays and the mapping of rays::Args (vrt_rays.h), one
// march per ray, the planes of one sample stored by the lane (any output may be null)
struct RayArgs {
    const float *origins;     // n x 3, or one origin when origin_stride == 0
    const float *dirs;        // n x 3
    float *out_normal;        // n x 3
    float *out_albedo;        // n x 4
    float *out_depth;         // n
    uint8_t *out_hit;         // n
    uint32_t n;
    int origin_stride;        // floats between origins: 0 or 3
    uint32_t width;           // the batch as an image of this width (the mapping only: a guide draws no random number)
    uint32_t tiles_x;         // rays::plan()
};

}  // namespace guides
}  // namespace vrt
