// vrt_launch_accum_hdr.hip -- the kernels of HDR accumulations (include/vrt.h vrt_accum_keep_hdr; vrt_accum.hip.h with HDR = true):
// the sample kernels' HDR forms in the shapes of vrt_launch_accum.hip.h, the repeat of a frame's float colour, the corner frame
// that leaves it (the mode's frame, or pass 1 of the opaque path) and the HDR resolve.
#include "vrt_launch_accum.hip.h"
#include "vrt_accum_hdr.hip.h"

namespace vrt {
namespace launch {

hipError_t accum_primary_hdr(int mode, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q,
                             bool adaptive, const accum::Lens &l, int grid, hipStream_t s) {
    return accum_impl::primary<true>(mode, src, v, a, vs, q, adaptive, l, grid, s);
}

// the sample launches of VRT_MODE_FULL, the plain family's (the other families: objects of their own)
template struct AccumPaths<true, PathFamily::kPlain>;

hipError_t accum_repeat_hdr(const accum::RepeatHdrOf<accum::Repeat> &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::repeat_kernel<true>, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t accum_repeat_hdr(const accum::RepeatHdrOf<accum::RepeatAdapt> &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::repeat_adaptive_kernel<true>, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t accum_frame_hdr(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrFrame &q, int grid, hipStream_t s) {
    if (mode != VRT_MODE_PRIMARY && mode != VRT_MODE_PRIMARY_SHADOW) return hipErrorInvalidValue;
    const bool shadow = mode == VRT_MODE_PRIMARY_SHADOW;
    return accum_impl::primary_shapes(v, false, [&](auto sh) {
        using S = decltype(sh);
        return shadow ? accum_impl::go(accum::hdr_frame_kernel<1, typename S::Trav, S::kBlock, S::kWpe, false>, grid, S::kBlock, s, a, vs, q)
                      : accum_impl::go(accum::hdr_frame_kernel<0, typename S::Trav, S::kBlock, S::kWpe, false>, grid, S::kBlock, s, a, vs, q);
    });
}

hipError_t accum_pass1_hdr(const KArgs &a, const ViewSet &vs, const accum::HdrFrame &q, int grid, hipStream_t s) {
    return accum_impl::go(accum::hdr_frame_kernel<1, v4::Trav, 64, 7, true>, grid, 64, s, a, vs, q);
}

hipError_t accum_resolve_hdr(const accum::HdrResolve &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::hdr_resolve_kernel, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace vrt
