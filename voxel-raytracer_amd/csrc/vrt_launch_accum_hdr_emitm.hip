// vrt_launch_accum_hdr_emitm.hip -- vrt_launch_accum_emitm.hip's kernels for HDR accumulations (include/vrt.h vrt_accum_keep_hdr):
// full_accum_kernel over EmitMisPaths<...> with HDR = true, an object of their own.
#include "vrt_launch_accum.hip.h"

namespace vrt {
namespace launch {

hipError_t accum_full_hdr_emitm(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive,
                                const accum::Lens &l, const EmitMis &em, int grid, hipStream_t s) {
    return accum_impl::full_emit_mis<true>(src, v, a, vs, q, adaptive, l, em, grid, s);
}

}  // namespace launch
}  // namespace vrt
