// vrt_launch_filter.hip -- the kernels of the guided filter and of its variance-guided form (vrt_filter.hip.h, include/vrt.h
// vrt_filter_hdr and vrt_filter_hdr_var) in a launch file of their own: no other object's device code changes. The resources are in
// profiles/filter_resource_usage.txt and profiles/filter_var_resource_usage.txt.
#include <hip/hip_runtime.h>

#include "vrt_launch.h"
#include "vrt_filter.hip.h"

namespace vrt {
namespace launch {

namespace {
dim3 frame_grid(int width, int height) {
    return dim3((unsigned)((width + filter::kBlockX - 1) / filter::kBlockX), (unsigned)((height + filter::kBlockY - 1) / filter::kBlockY));
}
const dim3 kFrameBlock(filter::kBlockX, filter::kBlockY);

// The lattice form up to this step, the gather form above it, for both argument types. Guide-only, per level at 1080p: the lattice
// form takes 0.11 / 0.09 / 0.13 ms at steps 1 / 2 / 4 against 0.17-0.27 / 0.17 / 0.19 ms, and 0.22 / 0.24 / 0.23 ms at steps
// 8 / 16 / 32 against 0.16 / 0.15 / 0.17 ms (profiles/filter_levels_ab.txt). The variance-guided levels cross over at the same step
// (profiles/filter_var_levels_ab.txt). The constant stands beside the tile's in vrt_filter.hip.h, where the test library reads it.
using filter::kLatticeMaxStep;

template <class Q>
hipError_t level(const Q &q, bool first, bool last, hipStream_t s) {
    const filter::Level &l = filter::level_of(q);
    if (l.step <= kLatticeMaxStep) {
        const unsigned tx = (unsigned)(((l.width + l.step - 1) / l.step + filter::kLatX - 1) / filter::kLatX);
        const unsigned ty = (unsigned)(((l.height + l.step - 1) / l.step + filter::kLatY - 1) / filter::kLatY);
        const dim3 grid(tx * (unsigned)l.step, ty * (unsigned)l.step), block(filter::kLatX, filter::kLatY);
        if (first && last) hipLaunchKernelGGL((filter::filter_level_lattice_kernel<Q, true, true>), grid, block, 0, s, q);
        else if (first) hipLaunchKernelGGL((filter::filter_level_lattice_kernel<Q, true, false>), grid, block, 0, s, q);
        else if (last) hipLaunchKernelGGL((filter::filter_level_lattice_kernel<Q, false, true>), grid, block, 0, s, q);
        else hipLaunchKernelGGL((filter::filter_level_lattice_kernel<Q, false, false>), grid, block, 0, s, q);
        return hipGetLastError();
    }
    if (first) return hipErrorInvalidValue;   // step 1 is a lattice level
    const dim3 grid = frame_grid(l.width, l.height);
    if (last) hipLaunchKernelGGL((filter::filter_level_kernel<Q, true>), grid, kFrameBlock, 0, s, q);
    else hipLaunchKernelGGL((filter::filter_level_kernel<Q, false>), grid, kFrameBlock, 0, s, q);
    return hipGetLastError();
}
}  // namespace

hipError_t filter_prepass(const filter::Prepass &q, hipStream_t s) {
    hipLaunchKernelGGL(filter::filter_prepass_kernel, frame_grid(q.width, q.height), kFrameBlock, 0, s, q);
    return hipGetLastError();
}

hipError_t filter_variance(const filter::Variance &q, hipStream_t s) {
    const dim3 grid((unsigned)((q.l.width + filter::kVarX - 1) / filter::kVarX), (unsigned)((q.l.height + filter::kVarY - 1) / filter::kVarY));
    const dim3 block(filter::kVarX, filter::kVarY);
    if (q.variance) hipLaunchKernelGGL((filter::filter_variance_kernel<false>), grid, block, 0, s, q);
    else hipLaunchKernelGGL((filter::filter_variance_kernel<true>), grid, block, 0, s, q);
    return hipGetLastError();
}

hipError_t filter_level(const filter::Level &q, bool first, bool last, hipStream_t s) { return level(q, first, last, s); }
hipError_t filter_level(const filter::LevelVar &q, bool first, bool last, hipStream_t s) { return level(q, first, last, s); }

hipError_t filter_through(const filter::Through &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(filter::filter_through_kernel, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace vrt
