// vrt_launch_accum_deep.hip -- the progressive accumulation's kernels of VRT_MODE_FULL at a path depth above 1 (include/vrt.h
// vrt_set_path_depth): the forms of vrt_accum.hip.h over DeepPaths<...>, which read KArgs::path_depth, in an object of their own so
// that the kernels of vrt_launch_accum.hip keep their device code and `make -j` compiles the two side by side. The general full
// path tracer in two traversals (vrt_launch_accum.hip.h full_shapes<true>), the opaque chain looped in the lanes, the depth-looped
// bounce over pass 1's seeds. The HDR forms: vrt_launch_accum_hdr_deep.hip.
#include "vrt_launch_accum.hip.h"

namespace vrt {
namespace launch {

hipError_t accum_opaque_deep(accum::Source src, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive, const accum::Lens &l,
                             int grid, hipStream_t s) {
    return accum_impl::opaque<false, true>(src, a, vs, q, adaptive, l, grid, s);
}

hipError_t accum_full_deep(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive,
                           const accum::Lens &l, int grid, hipStream_t s) {
    return accum_impl::full<false, true>(src, v, a, vs, q, adaptive, l, grid, s);
}

hipError_t accum_bounce_deep(const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive, int grid, hipStream_t s) {
    return accum_impl::bounce<false, true>(a, vs, q, adaptive, grid, s);
}

}  // namespace launch
}  // namespace vrt
