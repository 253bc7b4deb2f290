// vrt_launch_guides.hip -- the guide planes' kernels (vrt_guides.hip.h): guide_kernel over a frame for the accumulation's three ray
// sources and over a caller's ray batch, and the resolve of the state. Two routes, as every path tracer family but the plain one
// has: the default wide traversal -- v4's one-loop form where the dispatcher proved every origin in empty space (variant trav 4, as
// the accumulation's primary kernels take it), its general loop otherwise and for ray batches -- and the record-array traversal v1,
// right for any tree (vrt_set_variant(1)). Every traversal gives the same hit, so the variants between are normalised to these.
#include "vrt_launch_accum.hip.h"
#include "vrt_guides.hip.h"

namespace vrt {
namespace launch {

namespace {
using accum_impl::go;

// Waves per SIMD (profiles/guides_resource_usage.txt): the march's own budget, as the accumulation's primary kernels have it -- 72
// registers hold the march and the ten state words. The lens forms take one wave fewer: lens_sample() inside the loop needs the
// registers, and at the budgets above them they keep 12-20 bytes per lane in scratch; one down, none.
constexpr int kWpeEye85 = 7, kWpeAny = 6;
// GLASS: the past-glass forms (vrt_set_guide_glass). They hold the general march alone and, beside it, the chain's state -- origin,
// direction, medium, path length, first alpha -- across the march and the refraction's arithmetic after it. At the general march's
// six waves (five for the lens) that leaves 12-60 bytes per lane in scratch; one wave per SIMD lower, none
// (profiles/guides_glass_resource_usage.txt). The record-array forms are unconstrained as their plain twins are.
constexpr int kWpeGlass = kWpeAny - 1;

template <class TRAV, int BLOCK, int WPE, bool GLASS>
hipError_t frame(accum::Source src, const KArgs &a, const ViewSet &vs, const guides::Args &q, const accum::Lens &l, int grid, hipStream_t s) {
    if (src == accum::Source::kCorner) return go(guides::guide_kernel<accum::CornerSource, TRAV, BLOCK, WPE, GLASS>, grid, BLOCK, s, a, vs, q);
    // (the past-glass jitter form keeps the loop's arguments beside the chain: at kWpeGlass it spills two registers, one lower none)
    constexpr int kJitterWpe = (GLASS && WPE > 1) ? WPE - 1 : WPE;
    if (src == accum::Source::kJitter) return go(guides::guide_kernel<accum::JitterSource, TRAV, BLOCK, kJitterWpe, GLASS>, grid, BLOCK, s, a, vs, q);
    return go(guides::guide_kernel<accum::LensSource, TRAV, BLOCK, (WPE > 1 ? WPE - 1 : 1), GLASS, accum::Lens>, grid, BLOCK, s, a, vs, q, l);
}
template <class TRAV, int BLOCK, int WPE>
hipError_t frame(bool glass, accum::Source src, const KArgs &a, const ViewSet &vs, const guides::Args &q, const accum::Lens &l, int grid, hipStream_t s) {
    return glass ? frame<TRAV, BLOCK, WPE, true>(src, a, vs, q, l, grid, s) : frame<TRAV, BLOCK, WPE, false>(src, a, vs, q, l, grid, s);
}
}  // namespace

hipError_t accum_guides(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const guides::Args &q, const accum::Lens &l,
                        bool glass, int grid, hipStream_t s) {
    if (q.n == 0u) return hipSuccess;
    // past glass every segment takes the general march, so the two wide routes share one set of kernels
    if (v.trav >= 3 && glass) return frame<v4::TravAny, 64, kWpeGlass, true>(src, a, vs, q, l, grid, s);
    if (v.trav == 4) return frame<v4::Trav, 64, kWpeEye85, false>(src, a, vs, q, l, grid, s);
    if (v.trav == 3) return frame<v4::TravAny, 64, kWpeAny, false>(src, a, vs, q, l, grid, s);
    if (v.trav >= 1) return frame<v1::Trav, 256, 1>(glass, src, a, vs, q, l, grid, s);
    return hipErrorInvalidValue;
}

hipError_t guides_resolve(const guides::Resolve &q, hipStream_t s) {
    if (q.pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(guides::guide_resolve_kernel, dim3((q.pixels + 255u) / 256u), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t guide_rays(const Variant &v, const KArgs &a, const ViewSet &vs, const guides::RayArgs &q, bool glass, uint32_t grid, hipStream_t s) {
    if (q.n == 0u) return hipSuccess;
    if (v.trav >= 3 && glass) return go(guides::guide_kernel<guides::RaySource, v4::TravAny, 64, kWpeGlass, true>, (int)grid, 64, s, a, vs, q);
    if (v.trav >= 3) return go(guides::guide_kernel<guides::RaySource, v4::TravAny, 64, kWpeAny, false>, (int)grid, 64, s, a, vs, q);
    if (v.trav >= 1 && glass) return go(guides::guide_kernel<guides::RaySource, v1::Trav, 64, 1, true>, (int)grid, 64, s, a, vs, q);
    if (v.trav >= 1) return go(guides::guide_kernel<guides::RaySource, v1::Trav, 64, 1, false>, (int)grid, 64, s, a, vs, q);
    return hipErrorInvalidValue;
}

}  // namespace launch
}  // namespace vrt
