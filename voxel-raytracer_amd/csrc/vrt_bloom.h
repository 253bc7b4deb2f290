// vrt_bloom.h -- bloom (include/vrt.h vrt_bloom_hdr, points B0-B8): the sizes of the pyramid's levels and where each lies in the
// caller's workspace, as host/device inline functions, and the arguments of the two kernels (vrt_bloom.hip.h). One text of B0 serves
// vrt_bloom_workspace_bytes, the launches and tests/bloom_layout_main.cpp, which compiles this header alone under the host sanitizers:
// it needs include/vrt.h and the C headers below, nothing of HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/vrt.h"

#if defined(__HIPCC__)
#define VRT_BLOOM_FN __host__ __device__ inline
#else
#define VRT_BLOOM_FN inline
#endif

namespace vrt {
namespace bloom {

constexpr int kMaxLevels = VRT_BLOOM_MAX_LEVELS;
constexpr size_t kPixelBytes = 16;    // a pyramid pixel: (r, g, b, w)
constexpr size_t kLevelAlign = 256;   // every level starts at a multiple of it
constexpr uint64_t kMaxPixels = 1ull << 30;   // the frame-size rule's bound on W * H

// B0: the next level's extent
VRT_BLOOM_FN int half_up(int v) { return (v + 1) >> 1; }

// The pyramid of a frame: level l = 1..levels is w[l] x h[l] pixels at byte `offset[l]` of the workspace; level 0 is the frame
// itself (offset[0] is unused); `bytes` is the whole workspace.
struct Pyramid {
    int levels;
    int w[kMaxLevels + 1], h[kMaxLevels + 1];
    size_t offset[kMaxLevels + 1];
    size_t bytes;
};

VRT_BLOOM_FN size_t level_bytes(int w, int h) {
    const size_t b = (size_t)w * (size_t)h * kPixelBytes;
    return (b + kLevelAlign - 1) & ~(kLevelAlign - 1);
}

// false, and p untouched: a frame or a number of levels the calls refuse
VRT_BLOOM_FN bool pyramid(int width, int height, int levels, Pyramid &p) {
    if (width < 1 || height < 1 || (uint64_t)width * (uint64_t)height > kMaxPixels) return false;
    if (levels < 1 || levels > kMaxLevels) return false;
    p.levels = levels;
    p.w[0] = width;
    p.h[0] = height;
    p.offset[0] = 0;
    size_t at = 0;
    for (int l = 1; l <= kMaxLevels; ++l) {
        if (l > levels) {   // the entries no launch reads
            p.w[l] = p.h[l] = 0;
            p.offset[l] = at;
            continue;
        }
        p.w[l] = half_up(p.w[l - 1]);
        p.h[l] = half_up(p.h[l - 1]);
        p.offset[l] = at;
        at += level_bytes(p.w[l], p.h[l]);
    }
    p.bytes = at;
    return true;
}

// ---- the kernels' arguments ----

// B1-B3's parameters: the bright pass of the first down-sampling launch
struct Bright {
    const vrt_exposure *record;   // or null
    float exposure;               // tm->exposure
    float threshold, knee;
};

// One level of B4: the sw x sh source -> the dw x dh destination (dw = half_up(sw), dh = half_up(sh)). The first launch reads `rgb`
// (3 floats per pixel, 4-byte aligned) through B2 / B3, the others `src` (4 floats per pixel, 16-byte aligned).
struct DownArgs {
    const float *rgb;
    const float *src;
    float *dst;
    int sw, sh, dw, dh;
    Bright bright;
};

// One step of B6: dst (dw x dh, D_l on entry, U_l on return) += up(src), src being U_{l+1} of sw x sh. The last launch is B7 / B8
// instead: dst is unused, dw x dh is the frame, src is U_1, and rgb, the outputs (either may be null) and the rest are read.
struct UpArgs {
    const float *src;
    float *dst;
    int sw, sh, dw, dh;
    const float *rgb;
    float *out_rgb;
    uint32_t *out_rgba;
    const vrt_exposure *record;   // or null
    float exposure;               // tm->exposure
    int op;                       // VRT_TONEMAP_*
    float intensity, inv_levels;
};

}  // namespace bloom
}  // namespace vrt
