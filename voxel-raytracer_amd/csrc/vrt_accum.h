// vrt_accum.h -- the arguments of the progressive-accumulation kernels (vrt_accum.hip.h), shared by the host side (vrt_accum.cpp)
// and the launch files (vrt_launch_accum.hip, vrt_launch_accum_hdr.hip, vrt_launch_accum_mom.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

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

// A mode without jitter or lens (vrt_accum.hip.h repeat_kernel): n more samples that are all the frame in frame_rgba.
struct Repeat {
    const uint32_t *frame_rgba;
    uint32_t *sums;
    uint32_t n;
    uint32_t pixels;
};

// ---- adaptive accumulation (include/vrt.h vrt_accum_begin_adaptive) ----
// Pixel state: the three sums, the pixel's own sample count n in the fourth word of the sums, and Q = sum of L^2 over its samples
// (L = R + G + B of one sample's bytes; Q < 765^2 * 2^24 < 2^44) in a 64-bit word of its own.

// The stopping rule, exact: a pixel with n samples, S = sum of L and Q = sum of L^2 takes the next round's sample iff
//     n < min  ||  (n < max  &&  256 * (n * Q - S^2) > tol^2 * n^2 * (n - 1))
// n * Q - S^2 >= 0 (Cauchy-Schwarz); every term is below 2^105, so 128-bit unsigned arithmetic is exact. Device and host (the
// test library's probe) evaluate this one function.
__host__ __device__ inline bool adaptive_active(uint32_t n, uint64_t s, uint64_t q, uint32_t min, uint32_t max, uint32_t tol) {
    if (n < min) return true;
    if (n >= max) return false;
    typedef unsigned __int128 u128;
    const u128 spread = (u128)n * q - (u128)s * s;
    const u128 bound = (u128)((uint64_t)tol * tol) * ((u128)((uint64_t)n * n) * (n - 1u));
    return (spread << 8) > bound;
}

// Samples a pixel holds after `rounds` more rounds whose every sample equals its earlier ones (its spread stays 0, so the rule
// stops it at min, and at once where it already has min): the repeat path, and sky pixels of the opaque bounce.
__host__ __device__ inline uint32_t adaptive_constant_count(uint32_t n, uint32_t rounds, uint32_t min) {
    return n < min ? (rounds < min - n ? n + rounds : min) : n;
}

// Args of an adaptive launch: the kernels' template parameter ADAPT picks this type (ArgsOf), so the plain kernels keep Args.
struct AdaptArgs : Args {
    uint64_t *sq;                // Q per pixel, row-major
    const uint32_t *tiles;       // one-sample kernels: the tiles compact_tiles_kernel listed for this round ...
    const uint32_t *n_tiles;     // ... and how many
    uint32_t min, max, tol;      // the rule
};

// ---- HDR accumulation (include/vrt.h vrt_accum_keep_hdr) ----
// Beside everything above, three float64 sums per pixel of the samples' unclamped float colours, h(c) = min(max(c, 0), kHdrMax)
// each, added in sample order. The kernels' template parameter HDR picks the argument type that carries them, so the other
// kernels keep their arguments (and their code).
constexpr float kHdrMax = 65504.0f;
template <class BASE>
struct HdrOf : BASE {
    double *hsum;                // 3 doubles per pixel, row-major: the R, G, B sums of h(c)
    const float *hframe;         // 3 floats per pixel: the corner frame's float colour (bounce kernel: pass 1's), where one was made
};
// ---- luminance moments (include/vrt.h vrt_accum_keep_moments) ----
// Beside the HDR sums, two float64 sums per pixel of the samples' luminance y = Y(h(c)) and its float32 square q = y * y (M1, M2),
// added where and when the colour sums are. The kernels' template parameter MOM (with HDR) picks the argument type that carries them,
// as HDR picks HdrOf<>: the HDR-only kernels keep their arguments and their code.
template <class BASE>
struct MomOf : BASE {
    double *msum;                // 2 doubles per pixel, row-major: S1 = sum of y, S2 = sum of q
};
template <bool ADAPT>
using PlainArgsOf = typename std::conditional<ADAPT, AdaptArgs, Args>::type;
template <bool ADAPT, bool HDR = false, bool MOM = false>
using ArgsOf = typename std::conditional<MOM, MomOf<HdrOf<PlainArgsOf<ADAPT>>>,
                                         typename std::conditional<HDR, HdrOf<PlainArgsOf<ADAPT>>, PlainArgsOf<ADAPT>>::type>::type;
using HdrArgs = HdrOf<AdaptArgs>;
using MomArgs = MomOf<HdrArgs>;     // what the dispatcher fills; the launch functions pass the kernel its own slice

// hdr_frame_kernel: where the corner frame's bytes, id_dist and float colour go
struct HdrFrame {
    uint32_t *out_rgba;
    int2 *out_id;
    float *hframe;
};

// The HDR resolve: mean = (float)(sum / (double)n_p), then the tone map and the byte pack, in one pass.
struct HdrResolve {
    const double *hsum;
    const uint32_t *sums;        // adaptive: the pixel's own count is its fourth word
    float *out_rgb;              // 3 floats per pixel, or null
    uint32_t *out_rgba;          // or null
    uint32_t n;                  // samples in the sums (not adaptive)
    uint32_t adaptive;
    uint32_t pixels;
    int32_t op;                  // VRT_TONEMAP_*
    float exposure;
};

// M3: the two moment sums -> the variance of the mean's luminance, one float per pixel
struct MomVariance {
    const double *msum;
    const uint32_t *sums;        // adaptive: the pixel's own count is its fourth word
    float *out;
    uint32_t n;                  // samples in the sums (not adaptive)
    uint32_t adaptive;
    uint32_t pixels;
};

// Before each round of a one-sample kernel: the 8 x 8 tiles of the frame that hold an active pixel -> tiles[0 .. *n_tiles)
struct Tiles {
    const uint32_t *sums;
    const uint64_t *sq;
    uint32_t *tiles;
    uint32_t *n_tiles;           // zeroed before the launch
    int width, height;
    uint32_t min, max, tol;
};

// vrt_accum_counts: the per-pixel counts -> out, the number of active pixels added to *n_active (zeroed before the launch)
struct Counts {
    const uint32_t *sums;
    const uint64_t *sq;
    uint32_t *out;
    uint32_t *n_active;
    uint32_t pixels;
    uint32_t min, max, tol;
};

// The repeat path of an adaptive accumulation: each pixel's count goes to adaptive_constant_count(n, n_rounds, min)
struct RepeatAdapt : Repeat {
    uint64_t *sq;
    uint32_t min;
};
// ... and of HDR accumulations: the frame's float colour beside its bytes
template <class BASE>
struct RepeatHdrOf : BASE {
    double *hsum;
    const float *hframe;
};
// ... and of those that keep moments (repeat_mom_kernel, a sibling of the HDR repeat kernels)
template <class BASE>
struct RepeatMomOf : RepeatHdrOf<BASE> {
    double *msum;
};

// Where a sample's ray comes from (vrt_accum.hip.h CornerSource, JitterSource, LensSource): the pixel's corner, the jittered ray
// of VRT_ACCUM_JITTER, or a thin lens (Lens).
enum class Source { kCorner, kJitter, kLens };

// A thin lens (vrt_lens.hip.h, include/vrt.h vrt_set_lens), the fourth argument of the lens kernels.
struct Lens {
    float aperture, focus;       // aperture > 0
    uint32_t jitter;             // 1: the accumulation's VRT_ACCUM_JITTER
    uint32_t lane_eye;           // 1: look the medium up at each sample's own origin; 0: View::eye0 / eye1 hold it for every origin
};

}  // namespace accum
}  // namespace vrt
