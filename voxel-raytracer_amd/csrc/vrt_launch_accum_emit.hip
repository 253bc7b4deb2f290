// vrt_launch_accum_emit.hip -- the progressive accumulation's kernels of VRT_MODE_FULL with emitter sampling (include/vrt.h
// vrt_set_emitter_sampling): the general full path tracer (full_accum_kernel of vrt_accum.hip.h) over EmitPaths<...>, which connects
// every shadowing vertex to the emitter list it takes, with the Sun, as its last argument, and reads KArgs::path_depth (one family
// for every depth 1..8 and any sun radius), in an object of its own so that the kernels of the other accumulation objects keep
// their device code. Two traversals, three ray sources, adaptive or not. The stack-free opaque routes have no such form: with
// sampling on they are not taken. The HDR forms: vrt_launch_accum_hdr_emit.hip.
#include "vrt_launch_accum.hip.h"

namespace vrt {
namespace launch {

hipError_t accum_full_emit(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive,
                           const accum::Lens &l, const Emit &em, int grid, hipStream_t s) {
    return accum_impl::full_emit<false>(src, v, a, vs, q, adaptive, l, em, grid, s);
}

}  // namespace launch
}  // namespace vrt
