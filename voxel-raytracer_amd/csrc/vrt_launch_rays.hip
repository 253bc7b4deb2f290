// vrt_launch_rays.hip -- the ray-batch kernels (vrt_rays.hip.h): pathTrace for the caller's own rays, one lane per ray, in the
// traversal the dispatcher's variant names. Every traversal here is right for a ray that starts in any medium: v4's general loop
// (TravAny; the EYE85 loop of the frame kernels is not instantiated), v3, and the record-array traversals.
#include "vrt_launch_rays_paths.hip.h"

namespace vrt {
namespace launch {

namespace {
using rays_impl::go;

template <int MODE>
hipError_t primary(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, uint32_t grid, hipStream_t s, hipEvent_t ev0,
                   hipEvent_t ev1) {
    if (v.trav == 4) return go(rays::shade_rays_kernel<MODE, v4::TravAny, 6>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 3) return go(rays::shade_rays_kernel<MODE, v3::Trav, 6>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 2) return go(rays::shade_rays_kernel<MODE, v2::Trav, 1>, a, vs, q, grid, s, ev0, ev1);
    if (v.trav == 1) return go(rays::shade_rays_kernel<MODE, v1::Trav, 1>, a, vs, q, grid, s, ev0, ev1);
    return hipErrorInvalidValue;
}
}  // namespace

hipError_t shade_rays(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, uint32_t grid, hipStream_t s,
                      hipEvent_t ev0, hipEvent_t ev1) {
    if (q.n == 0u) return hipSuccess;
    if (mode == VRT_MODE_PRIMARY) return primary<0>(v, a, vs, q, grid, s, ev0, ev1);
    if (mode == VRT_MODE_PRIMARY_SHADOW) return primary<1>(v, a, vs, q, grid, s, ev0, ev1);
    return hipErrorInvalidValue;   // VRT_MODE_FULL: RayPaths<...>::full
}

// VRT_MODE_FULL, the plain family's kernels (the other families: objects of their own)
template struct RayPaths<false, PathFamily::kPlain>;

}  // namespace launch
}  // namespace vrt
