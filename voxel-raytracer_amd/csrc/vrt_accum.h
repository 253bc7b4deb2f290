// vrt_accum.h -- the arguments of the progressive-accumulation kernels (vrt_accum.hip.h, vrt_jitter.hip.h, vrt_lens.hip.h), shared by the host side (vrt_accum.cpp,
// vrt_dispatch.cpp) and the launch file (vrt_launch_accum.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vrt {
namespace accum {

// Samples per accumulation: 255 * kMaxSamples + kMaxSamples / 2 stays below 2^32, so a uint32 sum per channel is exact.
constexpr uint32_t kMaxSamples = 1u << 24;

// One launch of the sample-looped bounce kernel (opaque scenes) or of the general kernel (everything else).
struct Args {
    uint32_t *sums;              // 4 words per pixel, row-major over the frame: R, G, B sums of unorm8 bytes, the fourth unused
    const uint32_t *pass1_rgba;  // bounce kernel: pass 1's rgba8 image (what pixels without a bounce show in every sample)
    int2 *out_id;                // general kernel: where the frame's (voxel ID, dist) goes (the same for every sample)
    uint32_t first;              // initRNG sampleIndex of the first sample of this launch
    uint32_t n;                  // samples this launch adds (the general kernel: always 1)
};

// The resolve: sums -> rgba8 = (sum + n / 2) / n per channel, alpha 255.
struct Resolve {
    const uint32_t *sums;
    uint32_t *out_rgba;
    uint32_t n;                  // samples in the sums (>= 1)
    uint32_t pixels;
};

// A mode without jitter (vrt_jitter.hip.h repeat_kernel): n more samples that are all the frame in frame_rgba.
struct Repeat {
    const uint32_t *frame_rgba;
    uint32_t *sums;
    uint32_t n;
    uint32_t pixels;
};

// A thin lens (vrt_lens.hip.h, include/vrt.h vrt_set_lens), the fourth argument of the lens kernels.
struct Lens {
    float aperture, focus;       // aperture > 0
    uint32_t jitter;             // 1: the accumulation's VRT_ACCUM_JITTER
    uint32_t lane_eye;           // 1: look the medium up at each sample's own origin; 0: View::eye0 / eye1 hold it for every origin
};

}  // namespace accum
}  // namespace vrt
