// vrt_launch_accum_emitm.hip -- vrt_launch_accum_emitp.hip's kernels with vrt_set_emitter_mis (include/vrt.h): full_accum_kernel over
// EmitMisPaths<...>, which weighs the connection against the bounce ray by the balance heuristic and takes 1 / Wtot with the EmitPower
// as its last argument; an object of its own, so that the kernels of the other accumulation objects keep their device code. Two
// traversals, three ray sources, adaptive or not. The HDR forms: vrt_launch_accum_hdr_emitm.hip.
#include "vrt_launch_accum.hip.h"

namespace vrt {
namespace launch {

hipError_t accum_full_emitm(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive,
                            const accum::Lens &l, const EmitMis &em, int grid, hipStream_t s) {
    return accum_impl::full_emit_mis<false>(src, v, a, vs, q, adaptive, l, em, grid, s);
}

}  // namespace launch
}  // namespace vrt
