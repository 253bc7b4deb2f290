// vrt_launch_accum_hdr_emit.hip -- vrt_launch_accum_emit.hip's kernels for HDR accumulations (include/vrt.h vrt_accum_keep_hdr):
// full_accum_kernel over EmitPaths<...> with HDR = true, an object of their own.
#include "vrt_launch_accum.hip.h"

namespace vrt {
namespace launch {

hipError_t accum_full_hdr_emit(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive,
                               const accum::Lens &l, const Emit &em, int grid, hipStream_t s) {
    return accum_impl::full_emit<true>(src, v, a, vs, q, adaptive, l, em, grid, s);
}

}  // namespace launch
}  // namespace vrt
