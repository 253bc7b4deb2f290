// vrt_launch_upsample.hip -- the kernel of the guided upsampling pass (vrt_upsample.hip.h, include/vrt.h vrt_upsample_hdr) in a launch
// file of its own: no other object's device code changes (profiles/upsample_codegen.txt). The resources are in
// profiles/upsample_resource_usage.txt.
#include <hip/hip_runtime.h>

#include "vrt_launch.h"
#include "vrt_upsample.hip.h"

namespace vrt {
namespace launch {

hipError_t upsample_pass(const upsample::Args &q, hipStream_t s) {
    const unsigned tiles_x = (unsigned)((q.width * q.factor + upsample::kTile - 1) / upsample::kTile);
    const unsigned tiles_y = (unsigned)((q.height * q.factor + upsample::kTile - 1) / upsample::kTile);
    const dim3 grid((tiles_x + upsample::kWaves - 1) / upsample::kWaves, tiles_y), block(64, upsample::kWaves);
    hipLaunchKernelGGL(upsample::upsample_kernel, grid, block, 0, s, q);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace vrt
