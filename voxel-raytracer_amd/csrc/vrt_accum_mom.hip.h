// vrt_accum_mom.hip.h -- what only HDR accumulations that keep moments run (include/vrt.h vrt_accum_keep_moments; the sample kernels'
// MOM forms are in vrt_accum.hip.h): the repeat of a frame's float colour with its luminance moments, siblings of the HDR repeat
// kernels whose arguments have no room for the third pointer, and M3, the resolve of the two moment sums to the variance of the
// mean's luminance. Included by vrt_launch_accum_mom.hip alone.
#pragma once
#include "vrt_accum.hip.h"

namespace vrt {
namespace accum {

// repeat_kernel<true> / repeat_adaptive_kernel<true> with the moments: k samples equal to the frame's float colour add (double)y * k
// and (double)q * k (M2), k being what the colour sums take
template <bool ADAPT>
__global__ __launch_bounds__(256) void repeat_mom_kernel(const RepeatMomOf<typename std::conditional<ADAPT, RepeatAdapt, Repeat>::type> q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= q.pixels) return;
    uint32_t more = q.n;
    if constexpr (ADAPT) {
        AdaptArgs s{};
        s.sums = q.sums;
        s.sq = q.sq;
        PixelState st = load_state(s, i);
        more = adaptive_constant_count(st.n, q.n, q.min) - st.n;
        add_repeat(q.frame_rgba[i], more, st);
        store_state(s, i, st);
    } else {
        uint32_t r = 0u, g = 0u, b = 0u;
        add_bytes(q.frame_rgba[i], r, g, b);
        store_sums(q.sums, i, r * q.n, g * q.n, b * q.n);
    }
    HdrSum hs = load_hdr(q.hsum, i);
    add_hdr_repeat(q.hframe + (size_t)i * 3, more, hs);
    store_hdr(q.hsum, i, hs);
    MomSum ms = load_mom(q.msum, i);
    add_mom_repeat(q.hframe + (size_t)i * 3, more, ms);
    store_mom(q.msum, i, ms);
}

// M3 of include/vrt.h: the variance of the mean's luminance by the pixel's own count. The square of the mean is a float32 product,
// as a sample's q is, so that a pixel of equal samples gets exactly +0. (max(0, d) with the zero first: a NaN d goes to +0.)
__global__ __launch_bounds__(256) void mom_variance_kernel(const MomVariance q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= q.pixels) return;
    const uint32_t n = q.adaptive ? q.sums[(size_t)i * 4 + 3] : q.n;
    float var = kHdrMax * kHdrMax;   // n < 2: unknown
    if (n >= 2u) {
        const MomSum ms = load_mom(q.msum, i);
        const double m1 = ms.s1 / (double)n, m2 = ms.s2 / (double)n;
        const float m1f = (float)m1;
        const float sq = m1f * m1f;
        const double d = m2 - (double)sq;
        const double d0 = 0.0 < d ? d : 0.0;
        var = fmin_c(fmax_c(0.0f, (float)(d0 / (double)(n - 1u))), kHdrMax * kHdrMax);
    }
    q.out[i] = var;
}

}  // namespace accum
}  // namespace vrt
