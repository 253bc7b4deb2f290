// vrt_launch_impl.hip.h -- the instantiated (traversal, workgroup size, waves-per-SIMD) combinations of trace_kernel, shared by the
// per-mode launch files (vrt_launch_primary / _shadow / _full .hip: one mode each, so the three compile side by side).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "vrt_internal.h"
#include "vrt_launch.h"
#include "vrt_kernels.hip.h"
#include "vrt_kernels_v1.hip.h"
#include "vrt_kernels_wide.hip.h"
#include "vrt_kernels_v4.hip.h"
#include "vrt_full.hip.h"

namespace vrt {
namespace launch {

template <int MODE, class TRAV, int BLOCK, int WPE, int SCHED = 0>
// ev0/ev1 (both or neither): events attached to THIS dispatch packet (hipExtLaunchKernel), so their elapsed time is
// the kernel's own begin-to-end time, as a profiler reports it, without the latency of separate event markers
hipError_t launch_one(const vrt::KArgs &a, const vrt::ViewSet &vs, int grid, hipStream_t s, hipEvent_t ev0 = nullptr,
                      hipEvent_t ev1 = nullptr) {  // grid.y = a.n_views
    void (*kernel)(const vrt::KArgs, const vrt::ViewSet) = &vrt::trace_kernel<MODE, TRAV, BLOCK, WPE, SCHED>;
    if (ev0 || ev1)   // either may be null: the two-pass full path tracer times from the first kernel's start to the second one's end
        hipExtLaunchKernelGGL(kernel, dim3(grid, a.n_views), dim3(BLOCK), 0, s, ev0, ev1, 0, a, vs);
    else
        hipLaunchKernelGGL(kernel, dim3(grid, a.n_views), dim3(BLOCK), 0, s, a, vs);
    return hipGetLastError();
}

// The combinations that exist in the feedback-scheduled flavours too (KArgs::group_order / tile_cost choose one).
template <int MODE, class TRAV, int BLOCK, int WPE>
hipError_t launch_sched(const vrt::KArgs &a, const vrt::ViewSet &vs, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    switch ((a.group_order ? 1 : 0) | (a.tile_cost ? 2 : 0)) {
        case 1: return launch_one<MODE, TRAV, BLOCK, WPE, 1>(a, vs, grid, s, ev0, ev1);
        case 2: return launch_one<MODE, TRAV, BLOCK, WPE, 2>(a, vs, grid, s, ev0, ev1);
        case 3: return launch_one<MODE, TRAV, BLOCK, WPE, 3>(a, vs, grid, s, ev0, ev1);
        default: return launch_one<MODE, TRAV, BLOCK, WPE>(a, vs, grid, s, ev0, ev1);
    }
}

// Primary and primary + shadow rays: the default (v4), the v3 kernels the dispatcher takes for an eye inside a medium (six waves
// per SIMD; seven for variant 20's shadow march) and the record-array fallbacks.
template <int MODE>
hipError_t launch_mode(const Variant &v, const vrt::KArgs &a, const vrt::ViewSet &vs, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (v.trav == 4 && v.wpe == 7) return launch_sched<MODE, v4::Trav, 64, 7>(a, vs, grid, s, ev0, ev1);
    if (v.trav == 3 && v.wpe == 6) return launch_sched<MODE, v3::Trav, 64, 6>(a, vs, grid, s, ev0, ev1);
    if (v.trav == 3 && v.wpe == 7) return launch_sched<MODE, v3::Trav, 64, 7>(a, vs, grid, s, ev0, ev1);
    if (v.trav == 2) return launch_one<MODE, v2::Trav, 256, 1>(a, vs, grid, s, ev0, ev1);
    if (v.trav == 1) return launch_one<MODE, v1::Trav, 256, 1>(a, vs, grid, s, ev0, ev1);
    return hipErrorInvalidValue;
}

}  // namespace launch
}  // namespace vrt
