// vrt_launch_rays_paths.hip.h -- the launch of the ray batches' VRT_MODE_FULL kernel (vrt_rays.hip.h shade_rays_full_kernel) over one
// family of path tracer kernels (vrt_launch.h PathFamily), plain or HDR: vrt_launch.h RayPaths<HDR, F>::full. Each of the objects
// vrt_launch_rays{,_hdr}{,_deep,_sun,_emit,_emitp,_emitm}.hip instantiates its own and so holds that family's kernels. The plain
// family launches the traversal the dispatcher's variant names; every other family gives the same bytes in every traversal, so a
// launch is normalised to one of two: v4's general loop for the wide variants, v1 (right for any tree) for the others.
#pragma once
#include <hip/hip_ext.h>

#include "vrt_launch_accum.hip.h"
#include "vrt_rays.hip.h"

namespace vrt {
namespace launch {
namespace rays_impl {

// ev0 / ev1: events attached to this dispatch packet (vrt_launch.h trace_primary)
template <class K, class Q, class... ARG>
hipError_t go(K kernel, const KArgs &a, const ViewSet &vs, const Q &q, uint32_t grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1,
              const ARG &...arg) {
    if (ev0 || ev1) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, s, ev0, ev1, 0, a, vs, q, arg...);
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, s, a, vs, q, arg...);
    return hipGetLastError();
}

template <bool HDR, PathFamily F, bool LOOP, class... ARG>
hipError_t full(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::ArgsOf<HDR> &q, uint32_t grid, hipStream_t s, hipEvent_t ev0,
                hipEvent_t ev1, const ARG &...arg) {
    if constexpr (F != PathFamily::kPlain) {
        if (v.trav >= 3) return go(rays::shade_rays_full_kernel<Paths<F, v4::TravAny>, 5, LOOP, HDR, ARG...>, a, vs, q, grid, s, ev0, ev1, arg...);
        if (v.trav >= 1) return go(rays::shade_rays_full_kernel<Paths<F, v1::Trav>, 1, LOOP, HDR, ARG...>, a, vs, q, grid, s, ev0, ev1, arg...);
    } else {
        if (v.trav == 4) return go(rays::shade_rays_full_kernel<v4::TravAny, 5, LOOP, HDR>, a, vs, q, grid, s, ev0, ev1);
        if (v.trav == 3) return go(rays::shade_rays_full_kernel<v3::Trav, 5, LOOP, HDR>, a, vs, q, grid, s, ev0, ev1);
        if (v.trav == 2) return go(rays::shade_rays_full_kernel<v2::Trav, 1, LOOP, HDR>, a, vs, q, grid, s, ev0, ev1);
        if (v.trav == 1) return go(rays::shade_rays_full_kernel<v1::Trav, 1, LOOP, HDR>, a, vs, q, grid, s, ev0, ev1);
    }
    return hipErrorInvalidValue;
}

}  // namespace rays_impl

template <bool HDR, PathFamily F>
hipError_t RayPaths<HDR, F>::full(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, const PathArgs &pa, uint32_t grid,
                                  hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (q.n == 0u) return hipSuccess;
    return with_arg<F>(pa, [&](const auto &...arg) {
        return q.n_samples > 1u ? rays_impl::full<HDR, F, true>(v, a, vs, q, grid, s, ev0, ev1, arg...)
                                : rays_impl::full<HDR, F, false>(v, a, vs, q, grid, s, ev0, ev1, arg...);
    });
}

}  // namespace launch
}  // namespace vrt
