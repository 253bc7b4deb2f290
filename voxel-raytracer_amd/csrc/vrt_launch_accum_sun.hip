// vrt_launch_accum_sun.hip -- the progressive accumulation's kernels of VRT_MODE_FULL with a sun disc (include/vrt.h
// vrt_set_sun_disc): the forms of vrt_accum.hip.h over SunPaths<...>, which draw a light direction per shadowing vertex from the Sun
// they take as their last argument and read KArgs::path_depth (one family for every depth 1..8), in an object of their own so that
// the kernels of vrt_launch_accum.hip and vrt_launch_accum_deep.hip keep their device code. The general full path tracer in two
// traversals, the opaque chain looped in the lanes, the bounce over pass 1's seeds (which casts the depth-0 shadow ray itself). The
// HDR forms: vrt_launch_accum_hdr_sun.hip.
#include "vrt_launch_accum.hip.h"

namespace vrt {
namespace launch {

hipError_t accum_opaque_sun(accum::Source src, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive, const accum::Lens &l,
                            const Sun &sun, int grid, hipStream_t s) {
    return accum_impl::opaque<false, true>(src, a, vs, q, adaptive, l, grid, s, sun);
}

hipError_t accum_full_sun(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive,
                          const accum::Lens &l, const Sun &sun, int grid, hipStream_t s) {
    return accum_impl::full<false, true>(src, v, a, vs, q, adaptive, l, grid, s, sun);
}

hipError_t accum_bounce_sun(const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive, const Sun &sun, int grid, hipStream_t s) {
    return accum_impl::bounce<false, true>(a, vs, q, adaptive, grid, s, sun);
}

}  // namespace launch
}  // namespace vrt
