// vrt_accum_hdr.hip.h -- what only HDR accumulations run (include/vrt.h vrt_accum_keep_hdr; the sample kernels' HDR forms are in
// vrt_accum.hip.h): the corner frame with its float colour, and the resolve of the float64 sums with its tone map. Included by
// vrt_launch_accum_hdr.hip alone.
#pragma once
#include "vrt_accum.hip.h"

namespace vrt {
namespace accum {

// HDR accumulations from the corner: the frame with its float colour, one 8 x 8 tile per wave. MODE 0 / 1 without SEED: the mode's
// frame, which is every sample (repeat_kernel) -- bytes, id_dist and floats. SEED (MODE 1): pass 1 of the opaque path, what
// trace_kernel MODE 4 leaves (bytes, id_dist, the seeds in a.defer_rec) and the float colour of the pixels without a bounce.
// The march is trace_pixel's own: the miss-tile route of the frame kernels stores bytes only.
template <int MODE, class TRAV, int BLOCK, int WPE, bool SEED>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(WPE))) void hdr_frame_kernel(const KArgs a, const ViewSet vs, const HdrFrame q) {
    static_assert(!SEED || (MODE == 1 && BLOCK == 64), "pass 1: the primary + shadow kernel, one tile per workgroup");
    typename TRAV::Ctx tc_;
    TRAV::block_init(a, tc_);
    int px, py;
    if (!frame_pixel<BLOCK>(a, px, py)) return;
    uint32_t rgba;
    int2 idd;
    LateOut lo;
    float fc[3];
    uint32_t *seed = nullptr;
    if constexpr (SEED) seed = reinterpret_cast<uint32_t *>(a.defer_rec) + ((size_t)blockIdx.x * kSeedPlanes) * 64 + (threadIdx.x & 63);
    trace_pixel<MODE, TRAV, false, false, false, true>(a, vs.v[0], tc_, px, py, rgba, idd, lo, seed, nullptr, 0u, nullptr, 0u, fc);
    const size_t o = pixel_offset(a, px, py);
    q.out_rgba[o] = rgba;
    q.out_id[o] = idd;
    q.hframe[o * 3 + 0] = fc[0]; q.hframe[o * 3 + 1] = fc[1]; q.hframe[o * 3 + 2] = fc[2];
}

// The HDR resolve: the mean by the pixel's own count, its tone-mapped bytes
__global__ __launch_bounds__(256) void hdr_resolve_kernel(const HdrResolve q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= q.pixels) return;
    uint32_t n = q.n;
    if (q.adaptive) {
        const uint32_t w = q.sums[(size_t)i * 4 + 3];
        n = w > 0u ? w : 1u;
    }
    const HdrSum hs = load_hdr(q.hsum, i);
    const float m[3] = {(float)(hs.r / (double)n), (float)(hs.g / (double)n), (float)(hs.b / (double)n)};
    if (q.out_rgb) { q.out_rgb[(size_t)i * 3 + 0] = m[0]; q.out_rgb[(size_t)i * 3 + 1] = m[1]; q.out_rgb[(size_t)i * 3 + 2] = m[2]; }
    if (q.out_rgba)
        q.out_rgba[i] = unorm8(tone_map(m[0], q.op, q.exposure)) | (unorm8(tone_map(m[1], q.op, q.exposure)) << 8) |
                        (unorm8(tone_map(m[2], q.op, q.exposure)) << 16) | (255u << 24);
}

}  // namespace accum
}  // namespace vrt
