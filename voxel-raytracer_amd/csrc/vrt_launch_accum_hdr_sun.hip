// vrt_launch_accum_hdr_sun.hip -- vrt_launch_accum_sun.hip's kernels for HDR accumulations (include/vrt.h vrt_accum_keep_hdr):
// the sample kernels over SunPaths<...> with HDR = true, an object of their own.
#include "vrt_launch_accum.hip.h"

namespace vrt {
namespace launch {

hipError_t accum_opaque_hdr_sun(accum::Source src, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive, const accum::Lens &l,
                            const Sun &sun, int grid, hipStream_t s) {
    return accum_impl::opaque<true, true>(src, a, vs, q, adaptive, l, grid, s, sun);
}

hipError_t accum_full_hdr_sun(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive,
                          const accum::Lens &l, const Sun &sun, int grid, hipStream_t s) {
    return accum_impl::full<true, true>(src, v, a, vs, q, adaptive, l, grid, s, sun);
}

hipError_t accum_bounce_hdr_sun(const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive, const Sun &sun, int grid, hipStream_t s) {
    return accum_impl::bounce<true, true>(a, vs, q, adaptive, grid, s, sun);
}

}  // namespace launch
}  // namespace vrt
