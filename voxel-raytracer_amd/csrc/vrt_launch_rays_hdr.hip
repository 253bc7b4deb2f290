// vrt_launch_rays_hdr.hip -- the ray-batch kernels' HDR forms (vrt_rays.hip.h with HDR = true; include/vrt.h vrt_shade_rays_hdr):
// the traversals and the starting waves-per-EU of vrt_launch_rays.hip, in an object of their own so that the plain kernels keep
// their device code. Resource usage: profiles/shade_rays_hdr_resource_usage.txt.
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
hipError_t go(void (*kernel)(const KArgs, const ViewSet, const rays::HdrArgs), const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q,
              uint32_t grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0 || ev1) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, s, ev0, ev1, 0, a, vs, q);
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, s, a, vs, q);
    return hipGetLastError();
}

template <int MODE>
hipError_t primary(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, uint32_t grid, hipStream_t s, hipEvent_t ev0,
                   hipEvent_t ev1) {
    if (v.trav == 4) return go(rays::shade_rays_kernel<MODE, v4::TravAny, 6, true>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 3) return go(rays::shade_rays_kernel<MODE, v3::Trav, 6, true>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 2) return go(rays::shade_rays_kernel<MODE, v2::Trav, 1, true>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 1) return go(rays::shade_rays_kernel<MODE, v1::Trav, 1, true>, a, vs, q, grid, s, ev0, ev1);
    return hipErrorInvalidValue;
}

template <bool LOOP>
hipError_t full(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, uint32_t grid, hipStream_t s, hipEvent_t ev0,
                hipEvent_t ev1) {
    if (v.trav == 4) return go(rays::shade_rays_full_kernel<v4::TravAny, 5, LOOP, true>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 3) return go(rays::shade_rays_full_kernel<v3::Trav, 5, LOOP, true>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 2) return go(rays::shade_rays_full_kernel<v2::Trav, 1, LOOP, true>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 1) return go(rays::shade_rays_full_kernel<v1::Trav, 1, LOOP, true>, a, vs, q, grid, s, ev0, ev1);
    return hipErrorInvalidValue;
}
}  // namespace

hipError_t shade_rays_hdr(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, uint32_t grid, hipStream_t s,
                          hipEvent_t ev0, hipEvent_t ev1) {
    if (q.n == 0u) return hipSuccess;
    if (mode == VRT_MODE_PRIMARY) return primary<0>(v, a, vs, q, grid, s, ev0, ev1);
    if (mode == VRT_MODE_PRIMARY_SHADOW) return primary<1>(v, a, vs, q, grid, s, ev0, ev1);
    if (mode != VRT_MODE_FULL) return hipErrorInvalidValue;
    return q.n_samples > 1u ? full<true>(v, a, vs, q, grid, s, ev0, ev1) : full<false>(v, a, vs, q, grid, s, ev0, ev1);
}

}  // namespace launch
}  // namespace vrt
