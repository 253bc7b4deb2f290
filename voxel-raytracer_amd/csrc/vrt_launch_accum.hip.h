// vrt_launch_accum.hip.h -- the launch functions of the progressive accumulation's sample kernels (vrt_accum.hip.h), templated on
// HDR and, for VRT_MODE_FULL, on the family of path tracer kernels (vrt_launch.h PathFamily): vrt_launch_accum.hip instantiates the
// plain forms, vrt_launch_accum_hdr.hip those of HDR accumulations, vrt_launch_accum_mom.hip those of HDR accumulations that keep
// moments (MOM), vrt_launch_accum{,_hdr,_mom}_{deep,sun,emit,emitp,emitm}.hip one family's each (objects of their own, so that
// `make -j` compiles them side by side). One function per shape -- the primary modes
// and the opaque chain looped in the lanes, one sample of the general full path tracer, the bounce over pass 1's seeds, the repeat
// of a frame -- each for the ray source and the adaptive form asked for.
#pragma once
#include <hip/hip_runtime.h>

#include "vrt_launch.h"
#include "vrt_kernels.hip.h"
#include "vrt_kernels_v1.hip.h"
#include "vrt_kernels_wide.hip.h"
#include "vrt_kernels_v4.hip.h"
#include "vrt_accum.hip.h"

namespace vrt {
namespace launch {
// A family's wrapper of the traversal T (vrt_common.hip.h): the plain family launches the kernels over T itself
template <PathFamily F, class T> struct PathsOf { using type = T; };
template <class T> struct PathsOf<PathFamily::kDeep, T> { using type = DeepPaths<T>; };
template <class T> struct PathsOf<PathFamily::kSun, T> { using type = SunPaths<T>; };
template <class T> struct PathsOf<PathFamily::kEmit, T> { using type = EmitPaths<T>; };
template <class T> struct PathsOf<PathFamily::kEmitPower, T> { using type = EmitPowerPaths<T>; };
template <class T> struct PathsOf<PathFamily::kEmitMis, T> { using type = EmitMisPaths<T>; };
template <PathFamily F, class T> using Paths = typename PathsOf<F, T>::type;
// ... and its slice of the PathArgs, the kernels' last argument (Paths<F, T>::Arg): f(slice), or f() for the families that take none
template <PathFamily F, class FN>
hipError_t with_arg(const PathArgs &pa, FN &&f) {
    if constexpr (F == PathFamily::kEmitMis) return f(pa);
    else if constexpr (F == PathFamily::kEmitPower) return f(pa.power);
    else if constexpr (F == PathFamily::kEmit) return f(pa.power.emit);
    else if constexpr (F == PathFamily::kSun) return f(pa.power.emit.sun);
    else return f();
}

namespace accum_impl {

template <class K, class... P>
hipError_t go(K kernel, int grid, int block, hipStream_t s, const P &...p) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, p...);
    return hipGetLastError();
}

// A kernel's traversal, workgroup, waves per SIMD and form: f(Shape<...>{}) for the variant's traversal and `adaptive`
template <class TRAV, int BLOCK, int WPE, bool ADAPT>
struct Shape {
    using Trav = TRAV;
    static constexpr int kBlock = BLOCK, kWpe = WPE;
    static constexpr bool kAdapt = ADAPT;
};
template <class TRAV, int BLOCK, int WPE, class F>
hipError_t shape(bool adaptive, F &&f) {
    return adaptive ? f(Shape<TRAV, BLOCK, WPE, true>{}) : f(Shape<TRAV, BLOCK, WPE, false>{});
}
// ... and a kernel's ray source: the plain one, or with an argument A the one that carries it too
template <class PLAIN, template <class> class WITH, class... A> struct SrcOf { using type = PLAIN; };
template <class PLAIN, template <class> class WITH, class A> struct SrcOf<PLAIN, WITH, A> { using type = WITH<A>; };
template <class... A> using CornerSrc = typename SrcOf<accum::CornerSource, accum::ArgCornerSource, A...>::type;
template <class... A> using JitterSrc = typename SrcOf<accum::JitterSource, accum::ArgJitterSource, A...>::type;
template <class... A> using LensSrc = typename SrcOf<accum::LensSource, accum::ArgLensSource, A...>::type;
// the general full path tracer: the shapes trace_full() launches trace_kernel<2> in. Every family but the plain one gives the same
// bytes in every variant, so a launch is normalised to one of two instantiated traversals of its workgroup shape -- v4 for the wide
// ones, v1 (right for any tree) for the record-array ones
template <PathFamily F, class FN>
hipError_t full_shapes(const Variant &v, bool adaptive, FN &&f) {
    if constexpr (F != PathFamily::kPlain) {
        if (v.trav >= 3) return shape<Paths<F, v4::TravAny>, 64, 5>(adaptive, f);
        if (v.trav >= 1) return shape<Paths<F, v1::Trav>, 256, 1>(adaptive, f);
        return hipErrorInvalidValue;
    } else {
        if (v.trav == 4) return shape<v4::TravAny, 64, 5>(adaptive, f);
        if (v.trav == 3) return shape<v3::Trav, 64, 5>(adaptive, f);
        if (v.trav == 2) return shape<v2::Trav, 256, 1>(adaptive, f);
        if (v.trav == 1) return shape<v1::Trav, 256, 1>(adaptive, f);
        return hipErrorInvalidValue;
    }
}
// the primary modes: the variants the dispatcher normalises an accumulation to
template <class F>
hipError_t primary_shapes(const Variant &v, bool adaptive, F &&f) {
    if (v.trav == 4) return shape<v4::Trav, 64, 7>(adaptive, f);
    if (v.trav == 3) return shape<v3::Trav, 64, 6>(adaptive, f);
    if (v.trav == 2) return shape<v2::Trav, 256, 1>(adaptive, f);
    if (v.trav == 1) return shape<v1::Trav, 256, 1>(adaptive, f);
    return hipErrorInvalidValue;
}

// what the dispatcher fills (every field a form may need), and the kernel's own slice of it
template <bool HDR, bool MOM = false>
using Filled = typename std::conditional<MOM, accum::MomArgs, typename std::conditional<HDR, accum::HdrArgs, accum::AdaptArgs>::type>::type;
template <bool ADAPT, bool HDR, bool MOM = false>
accum::ArgsOf<ADAPT, HDR, MOM> slice(const Filled<HDR, MOM> &q) {
    if constexpr (HDR && !ADAPT) {
        accum::ArgsOf<false, true, MOM> r{};
        static_cast<accum::Args &>(r) = q;
        r.hsum = q.hsum;
        r.hframe = q.hframe;
        if constexpr (MOM) r.msum = q.msum;
        return r;
    } else {
        return q;
    }
}

template <bool HDR, bool MOM = false>
hipError_t primary(int mode, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const Filled<HDR, MOM> &q, bool adaptive,
                   const accum::Lens &l, int grid, hipStream_t s) {
    if (mode != VRT_MODE_PRIMARY && mode != VRT_MODE_PRIMARY_SHADOW) return hipErrorInvalidValue;
    const bool shadow = mode == VRT_MODE_PRIMARY_SHADOW;
    return primary_shapes(v, adaptive, [&](auto sh) {
        using S = decltype(sh);
        const accum::ArgsOf<S::kAdapt, HDR, MOM> qs = slice<S::kAdapt, HDR, MOM>(q);
        if (src == accum::Source::kJitter)
            return shadow ? go(accum::primary_accum_kernel<accum::JitterSource, 1, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, MOM>, grid, S::kBlock, s, a, vs, qs)
                          : go(accum::primary_accum_kernel<accum::JitterSource, 0, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, MOM>, grid, S::kBlock, s, a, vs, qs);
        if (src == accum::Source::kLens)
            return shadow ? go(accum::primary_accum_kernel<accum::LensSource, 1, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, MOM, accum::Lens>, grid, S::kBlock, s, a, vs, qs, l)
                          : go(accum::primary_accum_kernel<accum::LensSource, 0, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, MOM, accum::Lens>, grid, S::kBlock, s, a, vs, qs, l);
        return hipErrorInvalidValue;   // the corner's samples of these modes are the frame: accum_repeat
    });
}

// The three sample launches of VRT_MODE_FULL over the family F, `arg` its argument (one, or none). The emitter families exist for
// the general path tracer only: the opaque routes have no such kernels.
template <bool HDR, PathFamily F, bool MOM, class... ARG>
hipError_t opaque(accum::Source src, const KArgs &a, const ViewSet &vs, const Filled<HDR, MOM> &q, bool adaptive, const accum::Lens &l, int grid,
                  hipStream_t s, const ARG &...arg) {
    if constexpr (F >= PathFamily::kEmit) return hipErrorInvalidValue;
    else return shape<Paths<F, v4::Trav>, 64, F == PathFamily::kPlain ? 6 : accum::kDeepOpaqueWpe>(adaptive, [&](auto sh) {
        using S = decltype(sh);
        const accum::ArgsOf<S::kAdapt, HDR, MOM> qs = slice<S::kAdapt, HDR, MOM>(q);
        if (src == accum::Source::kJitter) return go(accum::opaque_accum_kernel<JitterSrc<ARG...>, typename S::Trav, S::kWpe, S::kAdapt, HDR, MOM, ARG...>, grid, 64, s, a, vs, qs, arg...);
        if (src == accum::Source::kLens) return go(accum::opaque_accum_kernel<LensSrc<ARG...>, typename S::Trav, S::kWpe, S::kAdapt, HDR, MOM, accum::Lens, ARG...>, grid, 64, s, a, vs, qs, l, arg...);
        return hipErrorInvalidValue;   // the corner's: pass 1 once, then accum_bounce
    });
}

template <bool HDR, PathFamily F, bool MOM, class... ARG>
hipError_t full(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const Filled<HDR, MOM> &q, bool adaptive,
                const accum::Lens &l, int grid, hipStream_t s, const ARG &...arg) {
    return full_shapes<F>(v, adaptive, [&](auto sh) {
        using S = decltype(sh);
        const accum::ArgsOf<S::kAdapt, HDR, MOM> qs = slice<S::kAdapt, HDR, MOM>(q);
        if (src == accum::Source::kCorner)
            return go(accum::full_accum_kernel<CornerSrc<ARG...>, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, MOM, ARG...>, grid, S::kBlock, s, a, vs, qs, arg...);
        if (src == accum::Source::kJitter)
            return go(accum::full_accum_kernel<JitterSrc<ARG...>, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, MOM, ARG...>, grid, S::kBlock, s, a, vs, qs, arg...);
        return go(accum::full_accum_kernel<LensSrc<ARG...>, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, MOM, accum::Lens, ARG...>, grid, S::kBlock, s, a, vs, qs, l, arg...);
    });
}

template <bool HDR, PathFamily F, bool MOM, class... ARG>
hipError_t bounce(const KArgs &a, const ViewSet &vs, const Filled<HDR, MOM> &q, bool adaptive, int grid, hipStream_t s, const ARG &...arg) {
    if constexpr (F >= PathFamily::kEmit) return hipErrorInvalidValue;
    else if (adaptive) return go(accum::bounce_accum_kernel<Paths<F, v4::TravAny>, true, HDR, MOM, ARG...>, grid, 64, s, a, vs, slice<true, HDR, MOM>(q), arg...);
    else return go(accum::bounce_accum_kernel<Paths<F, v4::TravAny>, false, HDR, MOM, ARG...>, grid, 64, s, a, vs, slice<false, HDR, MOM>(q), arg...);
}

}  // namespace accum_impl

// vrt_launch.h AccumPaths: each object instantiates its own (`template struct AccumPaths<HDR, F>;`, `<true, F, true>` with moments) and so
// holds that family's kernels
template <bool HDR, PathFamily F, bool MOM>
hipError_t AccumPaths<HDR, F, MOM>::opaque(accum::Source src, const KArgs &a, const ViewSet &vs, const accum::MomArgs &q, bool adaptive,
                                      const accum::Lens &l, const PathArgs &pa, int grid, hipStream_t s) {
    return with_arg<F>(pa, [&](const auto &...arg) { return accum_impl::opaque<HDR, F, MOM>(src, a, vs, q, adaptive, l, grid, s, arg...); });
}
template <bool HDR, PathFamily F, bool MOM>
hipError_t AccumPaths<HDR, F, MOM>::full(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::MomArgs &q, bool adaptive,
                                    const accum::Lens &l, const PathArgs &pa, int grid, hipStream_t s) {
    return with_arg<F>(pa, [&](const auto &...arg) { return accum_impl::full<HDR, F, MOM>(src, v, a, vs, q, adaptive, l, grid, s, arg...); });
}
template <bool HDR, PathFamily F, bool MOM>
hipError_t AccumPaths<HDR, F, MOM>::bounce(const KArgs &a, const ViewSet &vs, const accum::MomArgs &q, bool adaptive, const PathArgs &pa, int grid,
                                      hipStream_t s) {
    return with_arg<F>(pa, [&](const auto &...arg) { return accum_impl::bounce<HDR, F, MOM>(a, vs, q, adaptive, grid, s, arg...); });
}
}  // namespace launch
}  // namespace vrt
