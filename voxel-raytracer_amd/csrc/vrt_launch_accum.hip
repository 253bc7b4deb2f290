// vrt_launch_accum.hip -- progressive accumulation of VRT_MODE_FULL (vrt_accum.hip.h): the sample-looped bounce kernel of opaque
// scenes, the general kernel with a sample index in the shapes trace_full() launches trace_kernel<2> in, and the resolve.
#include <hip/hip_runtime.h>

#include "vrt_launch.h"
#include "vrt_kernels.hip.h"
#include "vrt_kernels_v1.hip.h"
#include "vrt_kernels_wide.hip.h"
#include "vrt_kernels_v4.hip.h"
#include "vrt_accum.hip.h"

namespace vrt {
namespace launch {

hipError_t accum_bounce(const KArgs &a, const ViewSet &vs, const accum::Args &q, int grid, hipStream_t s) {
    hipLaunchKernelGGL(accum::bounce_accum_kernel<v4::TravAny>, dim3(grid), dim3(64), 0, s, a, vs, q);
    return hipGetLastError();
}

hipError_t accum_full(const Variant &v, const KArgs &a, const ViewSet &vs, const accum::Args &q, int grid, hipStream_t s) {
    if (v.trav == 4) hipLaunchKernelGGL((accum::full_accum_kernel<v4::TravAny, 64, 5>), dim3(grid), dim3(64), 0, s, a, vs, q);
    else if (v.trav == 3 && v.block == 64) hipLaunchKernelGGL((accum::full_accum_kernel<v3::Trav, 64, 5>), dim3(grid), dim3(64), 0, s, a, vs, q);
    else if (v.trav == 2 && v.block == 256) hipLaunchKernelGGL((accum::full_accum_kernel<v2::Trav<false>, 256, 1>), dim3(grid), dim3(256), 0, s, a, vs, q);
    else if (v.trav == 1 && v.block == 256) hipLaunchKernelGGL((accum::full_accum_kernel<v1::Trav<false>, 256, 1>), dim3(grid), dim3(256), 0, s, a, vs, q);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t accum_resolve(const accum::Resolve &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::accum_resolve_kernel, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace vrt
