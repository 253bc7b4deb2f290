// vrt_launch_filter_var.hip -- the variance-guided filter's kernels (vrt_filter_var.hip.h, include/vrt.h vrt_filter_hdr_var) in a
// launch file of their own: no other object's device code changes. The resources are in profiles/filter_var_resource_usage.txt.
#include <hip/hip_runtime.h>

#include "vrt_launch.h"
#define VRT_FILTER_NO_PLAIN_KERNELS   // the prepass and levels == 0 are vrt_launch_filter.o's
#include "vrt_filter_var.hip.h"

namespace vrt {
namespace launch {

// The lattice form up to this step, the gather form above it (profiles/filter_var_levels_ab.txt)
#ifndef VRT_FILTER_VAR_LATTICE_MAX_STEP
#define VRT_FILTER_VAR_LATTICE_MAX_STEP 4
#endif
constexpr int kVarLatticeMaxStep = VRT_FILTER_VAR_LATTICE_MAX_STEP;

hipError_t filter_variance(const filter::Variance &q, hipStream_t s) {
    const dim3 grid((unsigned)((q.l.width + filter::kVarX - 1) / filter::kVarX), (unsigned)((q.l.height + filter::kVarY - 1) / filter::kVarY));
    const dim3 block(filter::kVarX, filter::kVarY);
    if (q.variance) hipLaunchKernelGGL((filter::filter_variance_kernel<false>), grid, block, 0, s, q);
    else hipLaunchKernelGGL((filter::filter_variance_kernel<true>), grid, block, 0, s, q);
    return hipGetLastError();
}

hipError_t filter_var_level(const filter::LevelVar &q, bool first, bool last, hipStream_t s) {
    const filter::Level &l = q.l;
    if (l.step <= kVarLatticeMaxStep) {
        const unsigned tx = (unsigned)(((l.width + l.step - 1) / l.step + filter::kLatX - 1) / filter::kLatX);
        const unsigned ty = (unsigned)(((l.height + l.step - 1) / l.step + filter::kLatY - 1) / filter::kLatY);
        const dim3 grid(tx * (unsigned)l.step, ty * (unsigned)l.step), block(filter::kLatX, filter::kLatY);
        if (first && last) hipLaunchKernelGGL((filter::filter_var_level_lattice_kernel<true, true>), grid, block, 0, s, q);
        else if (first) hipLaunchKernelGGL((filter::filter_var_level_lattice_kernel<true, false>), grid, block, 0, s, q);
        else if (last) hipLaunchKernelGGL((filter::filter_var_level_lattice_kernel<false, true>), grid, block, 0, s, q);
        else hipLaunchKernelGGL((filter::filter_var_level_lattice_kernel<false, false>), grid, block, 0, s, q);
        return hipGetLastError();
    }
    if (first) return hipErrorInvalidValue;   // step 1 is a lattice level
    const dim3 grid((unsigned)((l.width + filter::kBlockX - 1) / filter::kBlockX), (unsigned)((l.height + filter::kBlockY - 1) / filter::kBlockY));
    const dim3 block(filter::kBlockX, filter::kBlockY);
    if (last) hipLaunchKernelGGL((filter::filter_var_level_kernel<true>), grid, block, 0, s, q);
    else hipLaunchKernelGGL((filter::filter_var_level_kernel<false>), grid, block, 0, s, q);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace vrt
