// vrt_launch_bloom.hip -- the kernels of bloom (vrt_bloom.hip.h, include/vrt.h vrt_bloom_hdr) in a launch file of their own: no other
// object's device code changes (profiles/bloom_codegen.txt). The resources are in profiles/bloom_resource_usage.txt.
#include <hip/hip_runtime.h>

#include "vrt_launch.h"
#include "vrt_bloom.hip.h"

namespace vrt {
namespace launch {

namespace {
// a 1-D grid of kTX x kTY tiles over w x h destination pixels: at most (2^30 / 32 + 1) * (2^30 / 8 + 1) / 2^30 < 2^31 of them
dim3 bloom_grid(int w, int h) {
    const uint32_t tx = ((uint32_t)w + bloom::kTX - 1u) / bloom::kTX, ty = ((uint32_t)h + bloom::kTY - 1u) / bloom::kTY;
    return dim3(tx * ty);
}
}  // namespace

hipError_t bloom_down(const bloom::DownArgs &q, bool first, bool karis, hipStream_t s) {
    const dim3 grid = bloom_grid(q.dw, q.dh), block(bloom::kBlock);
    if (!first) hipLaunchKernelGGL((bloom::bloom_down_kernel<false, false, bloom::kGather>), grid, block, 0, s, q);
    else if (karis) hipLaunchKernelGGL((bloom::bloom_down_kernel<true, true, bloom::kGather>), grid, block, 0, s, q);
    else hipLaunchKernelGGL((bloom::bloom_down_kernel<true, false, bloom::kGather>), grid, block, 0, s, q);
    return hipGetLastError();
}

hipError_t bloom_up(const bloom::UpArgs &q, bool last, hipStream_t s) {
    const dim3 grid = bloom_grid(q.dw, q.dh), block(bloom::kBlock);
    if (last) hipLaunchKernelGGL(bloom::bloom_up_kernel<true>, grid, block, 0, s, q);
    else hipLaunchKernelGGL(bloom::bloom_up_kernel<false>, grid, block, 0, s, q);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace vrt
