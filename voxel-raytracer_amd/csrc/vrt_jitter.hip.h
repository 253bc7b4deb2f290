// vrt_jitter.hip.h -- the progressive accumulation's jittered samples and its primary modes (include/vrt.h vrt_accum_begin_ex).
// Jittered sample k of a pixel is the frame of the accumulation's mode with the pixel's ray moved from its corner by
// (jitter_x(k), jitter_y(k)) (vrt_common.hip.h jittered_ray_dir()) and, in VRT_MODE_FULL, initRNG(pixel, k); sample 0 is the
// frame itself. Like vrt_accum.hip.h, every kernel adds each sample's unorm8 bytes to the per-pixel integer sums, one
// read-add-write of a pixel's sums per launch, one lane per pixel: no atomics. The frame's (voxel ID, dist) image, which the
// resolve hands out, is rendered once per accumulation by an ordinary frame (vrt_accum.cpp), so no kernel here writes it.
//   primary_jitter_kernel  VRT_MODE_PRIMARY / _SHADOW: each lane loops over the launch's samples of its pixel -- jittered ray,
//                          the traversal the frame kernel would take (trace_kernel's 8 x 8 tiles, its eye lookup and
//                          empty-octant proofs: the eye does not move), shadow ray in MODE 1 -- and sums the bytes in registers.
//   opaque_jitter_kernel   VRT_MODE_FULL, scenes the dispatcher proves opaque seen from empty space: MODE 6's chain per sample
//                          (pass 1 with the jittered ray, its seed in registers, bounce_pixel with initRNG's sample index),
//                          looped over the launch's samples. Pass 1 depends on the sample now, so it cannot be shared as
//                          bounce_accum_kernel shares it.
//   full_jitter_kernel     VRT_MODE_FULL, everything else: trace_pixel_full with the jittered ray, one sample per launch.
//   repeat_kernel          a mode without jitter: every sample is the frame, so n samples add n times its bytes.
// Every kernel but repeat_kernel has an adaptive form (template parameter ADAPT, vrt_accum.hip.h); repeat_adaptive_kernel is
// the repeat's.
#pragma once
#include "vrt_accum.hip.h"

namespace vrt {
namespace accum {

template <int BLOCK>
VRT_DEV bool jitter_pixel(const KArgs &a, int &px, int &py) {
    const int lane = threadIdx.x & 63;
    const int tiles_x = (a.width + 7) / 8;
    const int tile = (int)blockIdx.x * (BLOCK / 64) + (int)(threadIdx.x >> 6);
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    px = tx * 8 + (lane & 7);
    py = ty * 8 + (lane >> 3);
    return px < a.width && py < a.height;
}

// q.n samples q.first, q.first + 1, ... of MODE 0 or 1; whole frame (KArgs: row0 = 0, n_rows = height, compact = 0)
template <int MODE, class TRAV, int BLOCK, int WPE, bool ADAPT = false>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(WPE))) void primary_jitter_kernel(const KArgs a, const ViewSet vs, const ArgsOf<ADAPT> q) {
    typename TRAV::Ctx tc_;
    TRAV::block_init(a, tc_);
    int px, py;
    if (!jitter_pixel<BLOCK>(a, px, py)) return;
    uint32_t r = 0u, g = 0u, b = 0u;
    PixelState st{};
    if constexpr (ADAPT) st = load_state(q, (size_t)py * (size_t)a.width + (size_t)px);
    for (uint32_t k = 0; k < q.n; ++k) {
        if constexpr (ADAPT)
            if (!state_active(q.min, q.max, q.tol, st)) break;
        uint32_t rgba;
        int2 idd;
        LateOut lo;
        // the kernel's arguments re-read from the kernarg segment for every sample (late_args(), late_view()): held in scalar
        // registers across the loop's back edge they spill, into vector lanes and from there to scratch
#ifdef __HIP_DEVICE_COMPILE__
        const KArgs ak = *late_args();
        const View vk = *late_view();
#else
        const KArgs &ak = a;
        const View &vk = vs.v[0];
#endif
        trace_pixel<MODE, TRAV, true>(ak, vk, tc_, px, py, rgba, idd, lo, nullptr, nullptr, q.first + k);
        if constexpr (ADAPT) add_sample(rgba, st);
        else add_bytes(rgba, r, g, b);
    }
    if constexpr (ADAPT) store_state(q, (size_t)py * (size_t)a.width + (size_t)px, st);
    else store_sums(q.sums, (size_t)py * (size_t)a.width + (size_t)px, r, g, b);
}

// MODE 6's two stages per sample, the seed in registers; 64 lanes, one 8 x 8 tile per wave
template <class TRAV, int WPE, bool ADAPT = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE))) void opaque_jitter_kernel(const KArgs a, const ViewSet vs, const ArgsOf<ADAPT> q) {
    typename TRAV::Ctx tc_;
    TRAV::block_init(a, tc_);
    int px, py;
    if (!jitter_pixel<64>(a, px, py)) return;
    uint32_t r = 0u, g = 0u, b = 0u;
    PixelState st{};
    if constexpr (ADAPT) st = load_state(q, (size_t)py * (size_t)a.width + (size_t)px);
    for (uint32_t k = 0; k < q.n; ++k) {
        if constexpr (ADAPT)
            if (!state_active(q.min, q.max, q.tol, st)) break;
        const uint32_t sample = q.first + k;
        uint32_t rgba, both;
        int2 idd;
        LateOut lo;
        Seed seed;
        seed.word = 0u;
#ifdef __HIP_DEVICE_COMPILE__   // re-read for every sample, as in primary_jitter_kernel
        const KArgs ak = *late_args();
        const View vk = *late_view();
#else
        const KArgs &ak = a;
        const View &vk = vs.v[0];
#endif
        trace_pixel<1, TRAV, true>(ak, vk, tc_, px, py, rgba, idd, lo, nullptr, &seed, sample);
        if (full::bounce_pixel<TRAV>(ak, tc_, px, py, seed, both, sample)) rgba = both;
        if constexpr (ADAPT) add_sample(rgba, st);
        else add_bytes(rgba, r, g, b);
    }
    if constexpr (ADAPT) store_state(q, (size_t)py * (size_t)a.width + (size_t)px, st);
    else store_sums(q.sums, (size_t)py * (size_t)a.width + (size_t)px, r, g, b);
}

// the general full path tracer, jittered sample q.first (q.n == 1): trace_kernel<2>'s tiles, one pixel per lane
// (ADAPT: the round's listed tiles, active lanes only)
template <class TRAV, int BLOCK, int WPE, bool ADAPT = false>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(WPE))) void full_jitter_kernel(const KArgs a, const ViewSet vs, const ArgsOf<ADAPT> q) {
    typename TRAV::Ctx tc_;
    TRAV::block_init(a, tc_);
    int px, py;
    if constexpr (ADAPT) {
        if (!listed_pixel<BLOCK>(a, q, px, py)) return;
    } else {
        if (!jitter_pixel<BLOCK>(a, px, py)) return;
    }
    PixelState st{};
    if constexpr (ADAPT) {
        st = load_state(q, (size_t)py * (size_t)a.width + (size_t)px);
        if (!state_active(q.min, q.max, q.tol, st)) return;
    }
    uint32_t rgba;
    int2 idd;
    LateOut lo;
    full::trace_pixel_full<TRAV, true>(a, vs.v[0], tc_, px, py, rgba, idd, lo, q.first);
    if constexpr (ADAPT) {
        add_sample(rgba, st);
        store_state(q, (size_t)py * (size_t)a.width + (size_t)px, st);
    } else {
        uint32_t r = 0u, g = 0u, b = 0u;
        add_bytes(rgba, r, g, b);
        store_sums(q.sums, (size_t)py * (size_t)a.width + (size_t)px, r, g, b);
    }
}

__global__ __launch_bounds__(256) void repeat_kernel(const Repeat q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= q.pixels) return;
    uint32_t r = 0u, g = 0u, b = 0u;
    add_bytes(q.frame_rgba[i], r, g, b);
    store_sums(q.sums, i, r * q.n, g * q.n, b * q.n);
}

// the same for an adaptive accumulation: q.n rounds of a sample that never changes take each pixel to
// adaptive_constant_count(), with no trace at all
__global__ __launch_bounds__(256) void repeat_adaptive_kernel(const RepeatAdapt q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= q.pixels) return;
    AdaptArgs s{};
    s.sums = q.sums;
    s.sq = q.sq;
    PixelState st = load_state(s, i);
    add_repeat(q.frame_rgba[i], adaptive_constant_count(st.n, q.n, q.min) - st.n, st);
    store_state(s, i, st);
}

}  // namespace accum
}  // namespace vrt
