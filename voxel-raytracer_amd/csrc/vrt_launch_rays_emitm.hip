// vrt_launch_rays_emitm.hip -- vrt_launch_rays.hip's VRT_MODE_FULL kernels with emitter sampling in VRT_EMIT_POWER and vrt_set_emitter_mis
// (include/vrt.h): shade_rays_full_emitm_kernel over EmitMisPaths<...>, which takes the EmitMis (the EmitPower and
// 1 / Wtot) as its fourth argument and reads KArgs::path_depth (every depth 1..8, any sun radius), in an object of its own. v4's general loop
// for the wide variants, v1 (right for any tree) for the others.
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
hipError_t go(void (*kernel)(const KArgs, const ViewSet, const rays::Args, const EmitMis), const KArgs &a, const ViewSet &vs, const rays::Args &q,
              const EmitMis &em, uint32_t grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0 || ev1) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, s, ev0, ev1, 0, a, vs, q, em);
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, s, a, vs, q, em);
    return hipGetLastError();
}

template <bool LOOP>
hipError_t full(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, const EmitMis &em, uint32_t grid, hipStream_t s,
                hipEvent_t ev0, hipEvent_t ev1) {
    if (v.trav >= 3) return go(rays::shade_rays_full_emitm_kernel<EmitMisPaths<v4::TravAny>, 5, LOOP, false>, a, vs, q, em, grid, s, ev0, ev1);
    if (v.trav >= 1) return go(rays::shade_rays_full_emitm_kernel<EmitMisPaths<v1::Trav>, 1, LOOP, false>, a, vs, q, em, grid, s, ev0, ev1);
    return hipErrorInvalidValue;
}
}  // namespace

hipError_t shade_rays_emitm(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, const EmitMis &em, uint32_t grid, hipStream_t s,
                          hipEvent_t ev0, hipEvent_t ev1) {
    if (q.n == 0u) return hipSuccess;
    return q.n_samples > 1u ? full<true>(v, a, vs, q, em, grid, s, ev0, ev1) : full<false>(v, a, vs, q, em, grid, s, ev0, ev1);
}

}  // namespace launch
}  // namespace vrt
