// vrt_launch_query.hip -- the world queries (vrt_query.hip.h): octree_ray_cast + get_placement_coord per ray, octree_find
// per point.
#include <hip/hip_runtime.h>

#include "vrt_launch.h"
#include "vrt_query.hip.h"

namespace vrt {
namespace launch {

hipError_t cast_rays(const KArgs &a, const query::RayArgs &q, hipStream_t s) {
    if (q.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(query::cast_rays_kernel, dim3((q.n + 63u) / 64u), dim3(64), 0, s, a, q);
    return hipGetLastError();
}

hipError_t find_voxels(const KArgs &a, const query::PointArgs &q, hipStream_t s) {
    if (q.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(query::find_voxels_kernel, dim3((q.n + 63u) / 64u), dim3(64), 0, s, a, q);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace vrt
