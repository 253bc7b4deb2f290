// vrt_launch_rays_hdr.hip -- the ray-batch kernels' HDR forms (vrt_rays.hip.h with HDR = true; include/vrt.h vrt_shade_rays_hdr):
// the traversals and the starting waves-per-EU of vrt_launch_rays.hip, in an object of their own so that the plain kernels keep
// their device code. Resource usage: profiles/shade_rays_hdr_resource_usage.txt.
#include "vrt_launch_rays_paths.hip.h"

namespace vrt {
namespace launch {

namespace {
using rays_impl::go;

template <int MODE>
hipError_t primary(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, uint32_t grid, hipStream_t s, hipEvent_t ev0,
                   hipEvent_t ev1) {
    if (v.trav == 4) return go(rays::shade_rays_kernel<MODE, v4::TravAny, 6, true>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 3) return go(rays::shade_rays_kernel<MODE, v3::Trav, 6, true>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 2) return go(rays::shade_rays_kernel<MODE, v2::Trav, 1, true>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 1) return go(rays::shade_rays_kernel<MODE, v1::Trav, 1, true>, a, vs, q, grid, s, ev0, ev1);
    return hipErrorInvalidValue;
}
}  // namespace

hipError_t shade_rays_hdr(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, uint32_t grid, hipStream_t s,
                          hipEvent_t ev0, hipEvent_t ev1) {
    if (q.n == 0u) return hipSuccess;
    if (mode == VRT_MODE_PRIMARY) return primary<0>(v, a, vs, q, grid, s, ev0, ev1);
    if (mode == VRT_MODE_PRIMARY_SHADOW) return primary<1>(v, a, vs, q, grid, s, ev0, ev1);
    return hipErrorInvalidValue;   // VRT_MODE_FULL: RayPaths<...>::full
}

// VRT_MODE_FULL, the plain family's kernels (the other families: objects of their own)
template struct RayPaths<true, PathFamily::kPlain>;

}  // namespace launch
}  // namespace vrt
