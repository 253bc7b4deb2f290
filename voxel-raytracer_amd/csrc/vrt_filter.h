// vrt_filter.h -- the arguments of the guided filter's kernels (vrt_filter.hip.h, include/vrt.h vrt_filter_hdr and
// vrt_filter_hdr_var), shared by the host side (vrt_filter.cpp) and the launch file (vrt_launch_filter.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vrt {
namespace filter {

// What every level re-reads of a pixel, sanitised once by the prepass: three row-major planes of 16-byte words in one buffer, so
// that a wave moves whole words side by side.
//   plane 0  g(normal) x, y, z; g(depth) -- or a NaN in the depth's place when the pixel is not live (g(depth) is never one), so
//            that a tap's first word says whether it counts
//   plane 1  g(albedo) R, G, B, A
//   plane 2  gx, gy (the centre's depth slopes), g(coverage), 0 -- read for the centre, and for a tap only where the first level
//            demodulates (m is two operations on plane 1 and the coverage: it is recomputed, not stored)
constexpr size_t kPackBytes = 48;
constexpr size_t kImageBytes = 16;   // a level image: u R, G, B and a zero per pixel

// the sanitised planes of the five steps' common inputs
struct Guides {
    const float *normal;      // 3 floats per pixel
    const float *albedo;      // 4
    const float *depth;       // 1
    const float *coverage;    // 1
};

struct Prepass {
    Guides g;
    float4 *pack;             // kPackBytes per pixel
    int width, height;
};

// One level: taps at `step` pixels. The first level reads the caller's image (h(c) / m), later ones `src`; the last level writes
// the outputs (either may be null), earlier ones `dst`.
struct Level {
    const float *rgb;         // the caller's image: the first level's taps, and the last level's pixels that are not live
    const float4 *pack;
    const float4 *src;
    float4 *dst;
    float *out_rgb;
    uint32_t *out_rgba;
    int width, height, step;
    float kn, ka, sigma_depth;
    uint32_t demodulate;
    int op;                   // VRT_TONEMAP_*
    float exposure;
};

// levels == 0: every pixel from the caller's planes, no prepass
struct Through {
    const float *rgb;
    Guides g;
    float *out_rgb;
    uint32_t *out_rgba;
    uint32_t pixels;
    uint32_t demodulate;
    int op;
    float exposure;
};

// ---- the variance-guided form (include/vrt.h vrt_filter_hdr_var) ----
// The variance of a pixel's luminance rides in the words the guide-only filter leaves unused: the initial one (V2) in plane 2's .w,
// a level's in its image's .w. No kernel loads or stages a word more than its guide-only form.

// V2: the initial variance of every live pixel into plane 2's .w, after the prepass
struct Variance {
    Level l;                  // rgb, pack, width, height, kn, ka, sigma_depth, demodulate; the rest unused
    float *pack_w;            // l.pack again, as floats: the kernel stores the one float, never the word
    const float *variance;    // the caller's plane, or null: the spatial estimate
    float *out_variance;      // levels == 0 only: the output plane (V4)
};

struct LevelVar {
    Level l;                  // src / dst carry the variance in .w
    float sigma_lum;
    float *out_variance;      // the last level's; may be null
};

// the guide-only arguments of either level struct
__host__ __device__ inline const Level &level_of(const Level &q) { return q; }
__host__ __device__ inline const Level &level_of(const LevelVar &q) { return q.l; }

}  // namespace filter
}  // namespace vrt
