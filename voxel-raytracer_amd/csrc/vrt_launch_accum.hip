// vrt_launch_accum.hip -- the progressive accumulation's kernels (vrt_accum.hip.h): one launch function per shape -- the primary
// modes and the opaque chain looped in the lanes, one sample of the general full path tracer, the bounce over pass 1's seeds --
// each for the ray source and the adaptive form asked for (vrt_launch_accum.hip.h); then the repeat of a frame, the resolves, the
// round's tile list and vrt_accum_counts' kernel. The forms of HDR accumulations: vrt_launch_accum_hdr.hip.
#include "vrt_launch_accum.hip.h"
#include "vrt_accum_state.hip.h"

namespace vrt {
namespace launch {

hipError_t accum_primary(int mode, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q,
                         bool adaptive, const accum::Lens &l, int grid, hipStream_t s) {
    return accum_impl::primary<false>(mode, src, v, a, vs, q, adaptive, l, grid, s);
}

// the sample launches of VRT_MODE_FULL, the plain family's (the other families: objects of their own)
template struct AccumPaths<false, PathFamily::kPlain>;

hipError_t accum_repeat(const accum::Repeat &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::repeat_kernel<false>, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t accum_repeat(const accum::RepeatAdapt &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::repeat_adaptive_kernel<false>, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t accum_resolve(const accum::Resolve &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::accum_resolve_kernel, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t adaptive_resolve(const accum::Resolve &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(accum::adaptive_resolve_kernel, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t adaptive_tiles(const accum::Tiles &t, hipStream_t s) {
    const uint32_t n = (uint32_t)((t.width + 7) / 8) * (uint32_t)((t.height + 7) / 8);
    hipError_t e = hipMemsetAsync(t.n_tiles, 0, sizeof(uint32_t), s);
    if (e != hipSuccess || n == 0u) return e;
    hipLaunchKernelGGL(accum::compact_tiles_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, t);
    return hipGetLastError();
}

hipError_t adaptive_counts(const accum::Counts &c, hipStream_t s) {
    hipError_t e = hipMemsetAsync(c.n_active, 0, sizeof(uint32_t), s);
    if (e != hipSuccess || c.pixels == 0u) return e;
    const uint32_t blocks = (c.pixels + 255u) / 256u;
    hipLaunchKernelGGL(accum::adaptive_counts_kernel, dim3(blocks < 1024u ? blocks : 1024u), dim3(256), 0, s, c);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace vrt
