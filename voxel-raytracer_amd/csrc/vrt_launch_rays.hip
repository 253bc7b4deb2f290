// vrt_launch_rays.hip -- the ray-batch kernels (vrt_rays.hip.h): pathTrace for the caller's own rays, one lane per ray, in the
// traversal the dispatcher's variant names. Every traversal here is right for a ray that starts in any medium: v4's general loop
// (TravAny; the EYE85 loop of the frame kernels is not instantiated), v3, and the record-array traversals.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "vrt_launch.h"
#include "vrt_kernels.hip.h"
#include "vrt_kernels_v1.hip.h"
#include "vrt_kernels_wide.hip.h"
#include "vrt_kernels_v4.hip.h"
#include "vrt_rays.hip.h"

namespace vrt {
namespace launch {

namespace {
hipError_t go(void (*kernel)(const KArgs, const ViewSet, const rays::Args), const KArgs &a, const ViewSet &vs, const rays::Args &q, uint32_t grid,
              hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0 || ev1) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, s, ev0, ev1, 0, a, vs, q);
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, s, a, vs, q);
    return hipGetLastError();
}

template <int MODE>
hipError_t primary(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, uint32_t grid, hipStream_t s, hipEvent_t ev0,
                   hipEvent_t ev1) {
    if (v.trav == 4) return go(rays::shade_rays_kernel<MODE, v4::TravAny, 6>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 3) return go(rays::shade_rays_kernel<MODE, v3::Trav, 6>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 2) return go(rays::shade_rays_kernel<MODE, v2::Trav, 1>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 1) return go(rays::shade_rays_kernel<MODE, v1::Trav, 1>, a, vs, q, grid, s, ev0, ev1);
    return hipErrorInvalidValue;
}

template <bool LOOP>
hipError_t full(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, uint32_t grid, hipStream_t s, hipEvent_t ev0,
                hipEvent_t ev1) {
    if (v.trav == 4) return go(rays::shade_rays_full_kernel<v4::TravAny, 5, LOOP>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 3) return go(rays::shade_rays_full_kernel<v3::Trav, 5, LOOP>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 2) return go(rays::shade_rays_full_kernel<v2::Trav, 1, LOOP>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 1) return go(rays::shade_rays_full_kernel<v1::Trav, 1, LOOP>, a, vs, q, grid, s, ev0, ev1);
    return hipErrorInvalidValue;
}
}  // namespace

hipError_t shade_rays(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, uint32_t grid, hipStream_t s,
                      hipEvent_t ev0, hipEvent_t ev1) {
    if (q.n == 0u) return hipSuccess;
    if (mode == VRT_MODE_PRIMARY) return primary<0>(v, a, vs, q, grid, s, ev0, ev1);
    if (mode == VRT_MODE_PRIMARY_SHADOW) return primary<1>(v, a, vs, q, grid, s, ev0, ev1);
    if (mode != VRT_MODE_FULL) return hipErrorInvalidValue;
    return q.n_samples > 1u ? full<true>(v, a, vs, q, grid, s, ev0, ev1) : full<false>(v, a, vs, q, grid, s, ev0, ev1);
}

}  // namespace launch
}  // namespace vrt
