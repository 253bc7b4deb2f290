// vrt_launch_accum.hip -- the progressive accumulation's kernels (vrt_accum.hip.h): one launch function per shape -- the primary
// modes and the opaque chain looped in the lanes, one sample of the general full path tracer, the bounce over pass 1's seeds --
// each for the ray source and the adaptive form asked for; then the repeat of a frame, the resolves, the round's tile list and
// vrt_accum_counts' kernel.
#include <hip/hip_runtime.h>

#include "vrt_launch.h"
#include "vrt_kernels.hip.h"
#include "vrt_kernels_v1.hip.h"
#include "vrt_kernels_wide.hip.h"
#include "vrt_kernels_v4.hip.h"
#include "vrt_accum.hip.h"

namespace vrt {
namespace launch {

namespace {
template <class K, class... P>
hipError_t go(K kernel, int grid, int block, hipStream_t s, const P &...p) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, p...);
    return hipGetLastError();
}

// A kernel's traversal, workgroup, waves per SIMD and form: f(Shape<...>{}) for the variant's traversal and `adaptive`
template <class TRAV, int BLOCK, int WPE, bool ADAPT>
struct Shape {
    using Trav = TRAV;
    static constexpr int kBlock = BLOCK, kWpe = WPE;
    static constexpr bool kAdapt = ADAPT;
};
template <class TRAV, int BLOCK, int WPE, class F>
hipError_t shape(bool adaptive, F &&f) {
    return adaptive ? f(Shape<TRAV, BLOCK, WPE, true>{}) : f(Shape<TRAV, BLOCK, WPE, false>{});
}
// the general full path tracer: the shapes trace_full() launches trace_kernel<2> in
template <class F>
hipError_t full_shapes(const Variant &v, bool adaptive, F &&f) {
    if (v.trav == 4) return shape<v4::TravAny, 64, 5>(adaptive, f);
    if (v.trav == 3) return shape<v3::Trav, 64, 5>(adaptive, f);
    if (v.trav == 2) return shape<v2::Trav, 256, 1>(adaptive, f);
    if (v.trav == 1) return shape<v1::Trav, 256, 1>(adaptive, f);
    return hipErrorInvalidValue;
}
// the primary modes: the variants the dispatcher normalises an accumulation to
template <class F>
hipError_t primary_shapes(const Variant &v, bool adaptive, F &&f) {
    if (v.trav == 4) return shape<v4::Trav, 64, 7>(adaptive, f);
    if (v.trav == 3) return shape<v3::Trav, 64, 6>(adaptive, f);
    if (v.trav == 2) return shape<v2::Trav, 256, 1>(adaptive, f);
    if (v.trav == 1) return shape<v1::Trav, 256, 1>(adaptive, f);
    return hipErrorInvalidValue;
}
}  // namespace

hipError_t accum_primary(int mode, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q,
                         bool adaptive, const accum::Lens &l, int grid, hipStream_t s) {
    if (mode != VRT_MODE_PRIMARY && mode != VRT_MODE_PRIMARY_SHADOW) return hipErrorInvalidValue;
    const bool shadow = mode == VRT_MODE_PRIMARY_SHADOW;
    return primary_shapes(v, adaptive, [&](auto sh) {
        using S = decltype(sh);
        const accum::ArgsOf<S::kAdapt> &qs = q;
        if (src == accum::Source::kJitter)
            return shadow ? go(accum::primary_accum_kernel<accum::JitterSource, 1, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt>, grid, S::kBlock, s, a, vs, qs)
                          : go(accum::primary_accum_kernel<accum::JitterSource, 0, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt>, grid, S::kBlock, s, a, vs, qs);
        if (src == accum::Source::kLens)
            return shadow ? go(accum::primary_accum_kernel<accum::LensSource, 1, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, accum::Lens>, grid, S::kBlock, s, a, vs, qs, l)
                          : go(accum::primary_accum_kernel<accum::LensSource, 0, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, accum::Lens>, grid, S::kBlock, s, a, vs, qs, l);
        return hipErrorInvalidValue;   // the corner's samples of these modes are the frame: accum_repeat
    });
}

hipError_t accum_opaque(accum::Source src, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive, const accum::Lens &l,
                        int grid, hipStream_t s) {
    return shape<v4::Trav, 64, 6>(adaptive, [&](auto sh) {
        using S = decltype(sh);
        const accum::ArgsOf<S::kAdapt> &qs = q;
        if (src == accum::Source::kJitter) return go(accum::opaque_accum_kernel<accum::JitterSource, typename S::Trav, S::kWpe, S::kAdapt>, grid, 64, s, a, vs, qs);
        if (src == accum::Source::kLens) return go(accum::opaque_accum_kernel<accum::LensSource, typename S::Trav, S::kWpe, S::kAdapt, accum::Lens>, grid, 64, s, a, vs, qs, l);
        return hipErrorInvalidValue;   // the corner's: pass 1 once, then accum_bounce
    });
}

hipError_t accum_full(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive,
                      const accum::Lens &l, int grid, hipStream_t s) {
    return full_shapes(v, adaptive, [&](auto sh) {
        using S = decltype(sh);
        const accum::ArgsOf<S::kAdapt> &qs = q;
        if (src == accum::Source::kCorner)
            return go(accum::full_accum_kernel<accum::CornerSource, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt>, grid, S::kBlock, s, a, vs, qs);
        if (src == accum::Source::kJitter)
            return go(accum::full_accum_kernel<accum::JitterSource, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt>, grid, S::kBlock, s, a, vs, qs);
        return go(accum::full_accum_kernel<accum::LensSource, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, accum::Lens>, grid, S::kBlock, s, a, vs, qs, l);
    });
}

hipError_t accum_bounce(const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive, int grid, hipStream_t s) {
    if (adaptive) return go(accum::bounce_accum_kernel<v4::TravAny, true>, grid, 64, s, a, vs, q);
    return go(accum::bounce_accum_kernel<v4::TravAny, false>, grid, 64, s, a, vs, static_cast<const accum::Args &>(q));
}

hipError_t accum_repeat(const accum::Repeat &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::repeat_kernel, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t accum_repeat(const accum::RepeatAdapt &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::repeat_adaptive_kernel, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t accum_resolve(const accum::Resolve &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::accum_resolve_kernel, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t adaptive_resolve(const accum::Resolve &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::adaptive_resolve_kernel, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t adaptive_tiles(const accum::Tiles &t, hipStream_t s) {
    const uint32_t n = (uint32_t)((t.width + 7) / 8) * (uint32_t)((t.height + 7) / 8);
    hipError_t e = hipMemsetAsync(t.n_tiles, 0, sizeof(uint32_t), s);
    if (e != hipSuccess || n == 0u) return e;
    hipLaunchKernelGGL(accum::compact_tiles_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, t);
    return hipGetLastError();
}

hipError_t adaptive_counts(const accum::Counts &c, hipStream_t s) {
    hipError_t e = hipMemsetAsync(c.n_active, 0, sizeof(uint32_t), s);
    if (e != hipSuccess || c.pixels == 0u) return e;
    const uint32_t blocks = (c.pixels + 255u) / 256u;
    hipLaunchKernelGGL(accum::adaptive_counts_kernel, dim3(blocks < 1024u ? blocks : 1024u), dim3(256), 0, s, c);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace vrt
