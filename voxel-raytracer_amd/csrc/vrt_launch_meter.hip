// vrt_launch_meter.hip -- the kernels of light metering (vrt_meter.hip.h, include/vrt.h vrt_meter_hdr and vrt_tonemap_hdr) in a
// launch file of their own: no other object's device code changes (profiles/meter_codegen.txt). The resources are in
// profiles/meter_resource_usage.txt.
#include <hip/hip_runtime.h>

#include "vrt_launch.h"
#include "vrt_meter.hip.h"

namespace vrt {
namespace launch {

hipError_t meter_histogram(const meter::HistArgs &q, hipStream_t s) {
    // a row's quads (one more than len / 4 where it starts inside one) over x, the rows over y, capped together; the loops stride
    const uint32_t quads = (q.len + 3u) / 4u + 1u;
    uint32_t bx = (quads + meter::kBlock - 1u) / meter::kBlock;
    bx = bx < meter::kMaxBlocks ? bx : meter::kMaxBlocks;
    const uint32_t room = meter::kMaxBlocks / bx, by = q.rows < room ? q.rows : room;
    hipLaunchKernelGGL(meter::histogram_kernel<meter::kMergeLanes>, dim3(bx, by), dim3(meter::kBlock), 0, s, q);
    return hipGetLastError();
}

hipError_t meter_finish(const meter::FinishArgs &q, hipStream_t s) {
    hipLaunchKernelGGL(meter::finish_kernel, dim3(1), dim3(meter::kBlock), 0, s, q);
    return hipGetLastError();
}

hipError_t meter_tonemap(const meter::ToneArgs &q, bool vec, hipStream_t s) {
    const size_t items = vec ? (q.n >> 2) + 1u : q.n, want = (items + meter::kBlock - 1u) / meter::kBlock;
    const dim3 grid((unsigned)(want < meter::kMaxBlocks * 4u ? want : meter::kMaxBlocks * 4u)), block(meter::kBlock);
    if (vec) hipLaunchKernelGGL(meter::tonemap_kernel<true>, grid, block, 0, s, q);
    else hipLaunchKernelGGL(meter::tonemap_kernel<false>, grid, block, 0, s, q);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace vrt
