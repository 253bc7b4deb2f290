// vrt_launch_accum.hip -- progressive accumulation of VRT_MODE_FULL (vrt_accum.hip.h): the sample-looped bounce kernel of opaque
// scenes, the general kernel with a sample index in the shapes trace_full() launches trace_kernel<2> in, and the resolve. Then the
// jittered samples and the primary modes (vrt_jitter.hip.h): the sample-looped primary / primary + shadow kernel in the
// traversals a frame of those modes takes, the looped opaque full path tracer, the general full path tracer with a jittered ray
// in the shapes of accum_full, and the repeat of a frame. Last, the thin-lens samples (vrt_lens.hip.h) in the shapes of their
// jittered forms. Every accumulation kernel also in its adaptive form (template parameter ADAPT; AdaptArgs overloads), with the
// adaptive resolve, the round's tile list and vrt_accum_counts' kernel.
#include <hip/hip_runtime.h>

#include "vrt_launch.h"
#include "vrt_kernels.hip.h"
#include "vrt_kernels_v1.hip.h"
#include "vrt_kernels_wide.hip.h"
#include "vrt_kernels_v4.hip.h"
#include "vrt_accum.hip.h"
#include "vrt_jitter.hip.h"
#include "vrt_lens.hip.h"

namespace vrt {
namespace launch {

namespace {
template <bool A>
hipError_t bounce(const KArgs &a, const ViewSet &vs, const accum::ArgsOf<A> &q, int grid, hipStream_t s) {
    hipLaunchKernelGGL((accum::bounce_accum_kernel<v4::TravAny, A>), dim3(grid), dim3(64), 0, s, a, vs, q);
    return hipGetLastError();
}

template <bool A>
hipError_t full(const Variant &v, const KArgs &a, const ViewSet &vs, const accum::ArgsOf<A> &q, int grid, hipStream_t s) {
    if (v.trav == 4) hipLaunchKernelGGL((accum::full_accum_kernel<v4::TravAny, 64, 5, A>), dim3(grid), dim3(64), 0, s, a, vs, q);
    else if (v.trav == 3) hipLaunchKernelGGL((accum::full_accum_kernel<v3::Trav, 64, 5, A>), dim3(grid), dim3(64), 0, s, a, vs, q);
    else if (v.trav == 2) hipLaunchKernelGGL((accum::full_accum_kernel<v2::Trav, 256, 1, A>), dim3(grid), dim3(256), 0, s, a, vs, q);
    else if (v.trav == 1) hipLaunchKernelGGL((accum::full_accum_kernel<v1::Trav, 256, 1, A>), dim3(grid), dim3(256), 0, s, a, vs, q);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
}  // namespace

hipError_t accum_bounce(const KArgs &a, const ViewSet &vs, const accum::Args &q, int grid, hipStream_t s) { return bounce<false>(a, vs, q, grid, s); }
hipError_t accum_bounce(const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, int grid, hipStream_t s) { return bounce<true>(a, vs, q, grid, s); }
hipError_t accum_full(const Variant &v, const KArgs &a, const ViewSet &vs, const accum::Args &q, int grid, hipStream_t s) { return full<false>(v, a, vs, q, grid, s); }
hipError_t accum_full(const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, int grid, hipStream_t s) { return full<true>(v, a, vs, q, grid, s); }

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

namespace {
template <int MODE, bool A>
hipError_t primary(const Variant &v, const KArgs &a, const ViewSet &vs, const accum::ArgsOf<A> &q, int grid, hipStream_t s) {
    if (v.trav == 4) hipLaunchKernelGGL((accum::primary_jitter_kernel<MODE, v4::Trav, 64, 7, A>), dim3(grid), dim3(64), 0, s, a, vs, q);
    else if (v.trav == 3) hipLaunchKernelGGL((accum::primary_jitter_kernel<MODE, v3::Trav, 64, 6, A>), dim3(grid), dim3(64), 0, s, a, vs, q);
    else if (v.trav == 2) hipLaunchKernelGGL((accum::primary_jitter_kernel<MODE, v2::Trav, 256, 1, A>), dim3(grid), dim3(256), 0, s, a, vs, q);
    else if (v.trav == 1) hipLaunchKernelGGL((accum::primary_jitter_kernel<MODE, v1::Trav, 256, 1, A>), dim3(grid), dim3(256), 0, s, a, vs, q);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <bool A>
hipError_t jprimary(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::ArgsOf<A> &q, int grid, hipStream_t s) {
    if (mode == VRT_MODE_PRIMARY) return primary<0, A>(v, a, vs, q, grid, s);
    if (mode == VRT_MODE_PRIMARY_SHADOW) return primary<1, A>(v, a, vs, q, grid, s);
    return hipErrorInvalidValue;
}

template <bool A>
hipError_t jopaque(const KArgs &a, const ViewSet &vs, const accum::ArgsOf<A> &q, int grid, hipStream_t s) {
    hipLaunchKernelGGL((accum::opaque_jitter_kernel<v4::Trav, 6, A>), dim3(grid), dim3(64), 0, s, a, vs, q);
    return hipGetLastError();
}

template <bool A>
hipError_t jfull(const Variant &v, const KArgs &a, const ViewSet &vs, const accum::ArgsOf<A> &q, int grid, hipStream_t s) {
    if (v.trav == 4) hipLaunchKernelGGL((accum::full_jitter_kernel<v4::TravAny, 64, 5, A>), dim3(grid), dim3(64), 0, s, a, vs, q);
    else if (v.trav == 3) hipLaunchKernelGGL((accum::full_jitter_kernel<v3::Trav, 64, 5, A>), dim3(grid), dim3(64), 0, s, a, vs, q);
    else if (v.trav == 2) hipLaunchKernelGGL((accum::full_jitter_kernel<v2::Trav, 256, 1, A>), dim3(grid), dim3(256), 0, s, a, vs, q);
    else if (v.trav == 1) hipLaunchKernelGGL((accum::full_jitter_kernel<v1::Trav, 256, 1, A>), dim3(grid), dim3(256), 0, s, a, vs, q);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
}  // namespace

hipError_t jitter_primary(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::Args &q, int grid, hipStream_t s) {
    return jprimary<false>(mode, v, a, vs, q, grid, s);
}
hipError_t jitter_primary(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, int grid, hipStream_t s) {
    return jprimary<true>(mode, v, a, vs, q, grid, s);
}
hipError_t jitter_opaque(const KArgs &a, const ViewSet &vs, const accum::Args &q, int grid, hipStream_t s) { return jopaque<false>(a, vs, q, grid, s); }
hipError_t jitter_opaque(const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, int grid, hipStream_t s) { return jopaque<true>(a, vs, q, grid, s); }
hipError_t jitter_full(const Variant &v, const KArgs &a, const ViewSet &vs, const accum::Args &q, int grid, hipStream_t s) { return jfull<false>(v, a, vs, q, grid, s); }
hipError_t jitter_full(const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, int grid, hipStream_t s) { return jfull<true>(v, a, vs, q, grid, s); }

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

// ---- thin lens (vrt_lens.hip.h) ----
namespace {
template <int MODE, bool A>
hipError_t lens_primary_mode(const Variant &v, const KArgs &a, const ViewSet &vs, const accum::ArgsOf<A> &q, const accum::Lens &l, int grid, hipStream_t s) {
    if (v.trav == 4) hipLaunchKernelGGL((accum::primary_lens_kernel<MODE, v4::Trav, 64, 7, A>), dim3(grid), dim3(64), 0, s, a, vs, q, l);
    else if (v.trav == 3) hipLaunchKernelGGL((accum::primary_lens_kernel<MODE, v3::Trav, 64, 6, A>), dim3(grid), dim3(64), 0, s, a, vs, q, l);
    else if (v.trav == 2) hipLaunchKernelGGL((accum::primary_lens_kernel<MODE, v2::Trav, 256, 1, A>), dim3(grid), dim3(256), 0, s, a, vs, q, l);
    else if (v.trav == 1) hipLaunchKernelGGL((accum::primary_lens_kernel<MODE, v1::Trav, 256, 1, A>), dim3(grid), dim3(256), 0, s, a, vs, q, l);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <bool A>
hipError_t lprimary(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::ArgsOf<A> &q, const accum::Lens &l, int grid, hipStream_t s) {
    if (mode == VRT_MODE_PRIMARY) return lens_primary_mode<0, A>(v, a, vs, q, l, grid, s);
    if (mode == VRT_MODE_PRIMARY_SHADOW) return lens_primary_mode<1, A>(v, a, vs, q, l, grid, s);
    return hipErrorInvalidValue;
}

template <bool A>
hipError_t lopaque(const KArgs &a, const ViewSet &vs, const accum::ArgsOf<A> &q, const accum::Lens &l, int grid, hipStream_t s) {
    hipLaunchKernelGGL((accum::opaque_lens_kernel<v4::Trav, 6, A>), dim3(grid), dim3(64), 0, s, a, vs, q, l);
    return hipGetLastError();
}

template <bool A>
hipError_t lfull(const Variant &v, const KArgs &a, const ViewSet &vs, const accum::ArgsOf<A> &q, const accum::Lens &l, int grid, hipStream_t s) {
    if (v.trav == 4) hipLaunchKernelGGL((accum::full_lens_kernel<v4::TravAny, 64, 5, A>), dim3(grid), dim3(64), 0, s, a, vs, q, l);
    else if (v.trav == 3) hipLaunchKernelGGL((accum::full_lens_kernel<v3::Trav, 64, 5, A>), dim3(grid), dim3(64), 0, s, a, vs, q, l);
    else if (v.trav == 2) hipLaunchKernelGGL((accum::full_lens_kernel<v2::Trav, 256, 1, A>), dim3(grid), dim3(256), 0, s, a, vs, q, l);
    else if (v.trav == 1) hipLaunchKernelGGL((accum::full_lens_kernel<v1::Trav, 256, 1, A>), dim3(grid), dim3(256), 0, s, a, vs, q, l);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
}  // namespace

hipError_t lens_primary(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::Args &q, const accum::Lens &l, int grid, hipStream_t s) {
    return lprimary<false>(mode, v, a, vs, q, l, grid, s);
}
hipError_t lens_primary(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, const accum::Lens &l, int grid, hipStream_t s) {
    return lprimary<true>(mode, v, a, vs, q, l, grid, s);
}
hipError_t lens_opaque(const KArgs &a, const ViewSet &vs, const accum::Args &q, const accum::Lens &l, int grid, hipStream_t s) { return lopaque<false>(a, vs, q, l, grid, s); }
hipError_t lens_opaque(const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, const accum::Lens &l, int grid, hipStream_t s) { return lopaque<true>(a, vs, q, l, grid, s); }
hipError_t lens_full(const Variant &v, const KArgs &a, const ViewSet &vs, const accum::Args &q, const accum::Lens &l, int grid, hipStream_t s) {
    return lfull<false>(v, a, vs, q, l, grid, s);
}
hipError_t lens_full(const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, const accum::Lens &l, int grid, hipStream_t s) {
    return lfull<true>(v, a, vs, q, l, grid, s);
}

}  // namespace launch
}  // namespace vrt
