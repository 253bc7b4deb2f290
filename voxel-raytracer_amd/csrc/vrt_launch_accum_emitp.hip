// vrt_launch_accum_emitp.hip -- vrt_launch_accum_emit.hip's kernels with VRT_EMIT_POWER (include/vrt.h vrt_set_emitter_importance):
// full_accum_kernel over EmitPowerPaths<...>, which picks the emitter by the table of thresholds it takes with the Emit as its last
// argument, and the face among those the vertex sees; an object of its own, so that the kernels of the other accumulation objects
// keep their device code. Two traversals, three ray sources, adaptive or not. The HDR forms: vrt_launch_accum_hdr_emitp.hip.
#include "vrt_launch_accum.hip.h"

namespace vrt {
namespace launch {

hipError_t accum_full_emitp(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive,
                            const accum::Lens &l, const EmitPower &em, int grid, hipStream_t s) {
    return accum_impl::full_emit_power<false>(src, v, a, vs, q, adaptive, l, em, grid, s);
}

}  // namespace launch
}  // namespace vrt
