// vrt_launch_temporal.hip -- the kernel of the temporal pass (vrt_temporal.hip.h, include/vrt.h vrt_temporal_hdr) in a launch file of
// its own: no other object's device code changes (profiles/temporal_codegen.txt). The resources are in
// profiles/temporal_resource_usage.txt.
#include <hip/hip_runtime.h>

#include "vrt_launch.h"
#include "vrt_temporal.hip.h"

namespace vrt {
namespace launch {

namespace {

template <class A>
hipError_t launch(const A &q, hipStream_t s) {
    const unsigned tiles_x = (unsigned)((q.width + temporal::kTile - 1) / temporal::kTile);
    const unsigned tiles_y = (unsigned)((q.height + temporal::kTile - 1) / temporal::kTile);
    const dim3 grid((tiles_x + temporal::kWaves - 1) / temporal::kWaves, tiles_y), block(64, temporal::kWaves);
    hipLaunchKernelGGL(temporal::temporal_kernel<A>, grid, block, 0, s, q);
    return hipGetLastError();
}

}  // namespace

hipError_t temporal_pass(const temporal::Args &q, hipStream_t s) { return launch(q, s); }
hipError_t temporal_pass_mom(const temporal::ArgsMom &q, hipStream_t s) { return launch(q, s); }

}  // namespace launch
}  // namespace vrt
