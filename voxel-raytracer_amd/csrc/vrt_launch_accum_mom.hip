// vrt_launch_accum_mom.hip -- the kernels of HDR accumulations that keep moments (include/vrt.h vrt_accum_keep_moments; vrt_accum.hip.h
// with HDR = MOM = true): the sample kernels' moments forms in the shapes of vrt_launch_accum.hip.h, the repeat of a frame's float
// colour with its moments, and M3's variance plane. The corner frame and pass 1 are the HDR object's: they keep no sums.
#include "vrt_launch_accum.hip.h"
#include "vrt_accum_mom.hip.h"

namespace vrt {
namespace launch {

hipError_t accum_primary_mom(int mode, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::MomArgs &q,
                             bool adaptive, const accum::Lens &l, int grid, hipStream_t s) {
    return accum_impl::primary<true, true>(mode, src, v, a, vs, q, adaptive, l, grid, s);
}

// the sample launches of VRT_MODE_FULL, the plain family's (the other families: objects of their own)
template struct AccumPaths<true, PathFamily::kPlain, true>;

hipError_t accum_repeat_mom(const accum::RepeatMomOf<accum::Repeat> &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::repeat_mom_kernel<false>, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t accum_repeat_mom(const accum::RepeatMomOf<accum::RepeatAdapt> &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::repeat_mom_kernel<true>, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t accum_variance(const accum::MomVariance &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::mom_variance_kernel, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace vrt
