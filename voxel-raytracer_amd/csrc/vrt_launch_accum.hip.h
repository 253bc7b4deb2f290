// vrt_launch_accum.hip.h -- the launch functions of the progressive accumulation's sample kernels (vrt_accum.hip.h), templated on
// HDR: vrt_launch_accum.hip instantiates the plain forms, vrt_launch_accum_hdr.hip those of HDR accumulations (two objects, so
// that `make -j` compiles them side by side). One function per shape -- the primary modes and the opaque chain looped in the
// lanes, one sample of the general full path tracer, the bounce over pass 1's seeds, the repeat of a frame -- each for the ray
// source and the adaptive form asked for.
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
// DEEP (the objects vrt_launch_accum_deep.hip, vrt_launch_accum_hdr_deep.hip): the kernels that honour KArgs::path_depth
// SUN (vrt_launch_accum_sun.hip, vrt_launch_accum_hdr_sun.hip): those that also honour the sun disc, at every depth; their last
// argument is the Sun (`sun...`, one or none)
template <bool DEEP, class T, bool SUN = false>
using Path = typename std::conditional<SUN, SunPaths<T>, typename std::conditional<DEEP, DeepPaths<T>, T>::type>::type;
template <bool SUN, class PLAIN, class WITH_SUN>
using Src = typename std::conditional<SUN, WITH_SUN, PLAIN>::type;
// the general full path tracer: the shapes trace_full() launches trace_kernel<2> in. DEEP: every variant gives the same bytes, so a
// launch is normalised to one of two instantiated traversals of its workgroup shape -- v4 for the wide ones, v1 (right for any
// tree) for the record-array ones
template <bool DEEP = false, bool SUN = false, class F>
hipError_t full_shapes(const Variant &v, bool adaptive, F &&f) {
    if constexpr (DEEP) {
        if (v.trav >= 3) return shape<Path<true, v4::TravAny, SUN>, 64, 5>(adaptive, f);
        if (v.trav >= 1) return shape<Path<true, v1::Trav, SUN>, 256, 1>(adaptive, f);
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
template <bool HDR>
using Filled = typename std::conditional<HDR, accum::HdrArgs, accum::AdaptArgs>::type;
template <bool ADAPT, bool HDR>
accum::ArgsOf<ADAPT, HDR> slice(const Filled<HDR> &q) {
    if constexpr (HDR && !ADAPT) {
        accum::ArgsOf<false, true> r{};
        static_cast<accum::Args &>(r) = q;
        r.hsum = q.hsum;
        r.hframe = q.hframe;
        return r;
    } else {
        return q;
    }
}

template <bool HDR>
hipError_t primary(int mode, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const Filled<HDR> &q, bool adaptive,
                   const accum::Lens &l, int grid, hipStream_t s) {
    if (mode != VRT_MODE_PRIMARY && mode != VRT_MODE_PRIMARY_SHADOW) return hipErrorInvalidValue;
    const bool shadow = mode == VRT_MODE_PRIMARY_SHADOW;
    return primary_shapes(v, adaptive, [&](auto sh) {
        using S = decltype(sh);
        const accum::ArgsOf<S::kAdapt, HDR> qs = slice<S::kAdapt, HDR>(q);
        if (src == accum::Source::kJitter)
            return shadow ? go(accum::primary_accum_kernel<accum::JitterSource, 1, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR>, grid, S::kBlock, s, a, vs, qs)
                          : go(accum::primary_accum_kernel<accum::JitterSource, 0, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR>, grid, S::kBlock, s, a, vs, qs);
        if (src == accum::Source::kLens)
            return shadow ? go(accum::primary_accum_kernel<accum::LensSource, 1, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, accum::Lens>, grid, S::kBlock, s, a, vs, qs, l)
                          : go(accum::primary_accum_kernel<accum::LensSource, 0, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, accum::Lens>, grid, S::kBlock, s, a, vs, qs, l);
        return hipErrorInvalidValue;   // the corner's samples of these modes are the frame: accum_repeat
    });
}

template <bool HDR, bool DEEP = false, class... SUN>
hipError_t opaque(accum::Source src, const KArgs &a, const ViewSet &vs, const Filled<HDR> &q, bool adaptive, const accum::Lens &l, int grid,
                  hipStream_t s, const SUN &...sun) {
    constexpr bool kSun = sizeof...(SUN) != 0;
    return shape<Path<DEEP, v4::Trav, kSun>, 64, DEEP ? accum::kDeepOpaqueWpe : 6>(adaptive, [&](auto sh) {
        using S = decltype(sh);
        const accum::ArgsOf<S::kAdapt, HDR> qs = slice<S::kAdapt, HDR>(q);
        if (src == accum::Source::kJitter) return go(accum::opaque_accum_kernel<Src<kSun, accum::JitterSource, accum::SunJitterSource>, typename S::Trav, S::kWpe, S::kAdapt, HDR, SUN...>, grid, 64, s, a, vs, qs, sun...);
        if (src == accum::Source::kLens) return go(accum::opaque_accum_kernel<Src<kSun, accum::LensSource, accum::SunLensSource>, typename S::Trav, S::kWpe, S::kAdapt, HDR, accum::Lens, SUN...>, grid, 64, s, a, vs, qs, l, sun...);
        return hipErrorInvalidValue;   // the corner's: pass 1 once, then accum_bounce
    });
}

template <bool HDR, bool DEEP = false, class... SUN>
hipError_t full(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const Filled<HDR> &q, bool adaptive,
                const accum::Lens &l, int grid, hipStream_t s, const SUN &...sun) {
    constexpr bool kSun = sizeof...(SUN) != 0;
    return full_shapes<DEEP, kSun>(v, adaptive, [&](auto sh) {
        using S = decltype(sh);
        const accum::ArgsOf<S::kAdapt, HDR> qs = slice<S::kAdapt, HDR>(q);
        if (src == accum::Source::kCorner)
            return go(accum::full_accum_kernel<Src<kSun, accum::CornerSource, accum::SunCornerSource>, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, SUN...>, grid, S::kBlock, s, a, vs, qs, sun...);
        if (src == accum::Source::kJitter)
            return go(accum::full_accum_kernel<Src<kSun, accum::JitterSource, accum::SunJitterSource>, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, SUN...>, grid, S::kBlock, s, a, vs, qs, sun...);
        return go(accum::full_accum_kernel<Src<kSun, accum::LensSource, accum::SunLensSource>, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, accum::Lens, SUN...>, grid, S::kBlock, s, a, vs, qs, l, sun...);
    });
}

// EMIT (vrt_launch_accum_emit.hip, vrt_launch_accum_hdr_emit.hip): the general full path tracer over EmitPaths<...>, in the two
// normalised traversals of the DEEP forms; the kernels' last argument is the Emit
template <bool HDR>
hipError_t full_emit(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const Filled<HDR> &q, bool adaptive,
                     const accum::Lens &l, const Emit &em, int grid, hipStream_t s) {
    const auto f = [&](auto sh) {
        using S = decltype(sh);
        const accum::ArgsOf<S::kAdapt, HDR> qs = slice<S::kAdapt, HDR>(q);
        if (src == accum::Source::kCorner)
            return go(accum::full_accum_kernel<accum::EmitCornerSource, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, Emit>, grid, S::kBlock, s, a, vs, qs, em);
        if (src == accum::Source::kJitter)
            return go(accum::full_accum_kernel<accum::EmitJitterSource, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, Emit>, grid, S::kBlock, s, a, vs, qs, em);
        return go(accum::full_accum_kernel<accum::EmitLensSource, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, accum::Lens, Emit>, grid, S::kBlock, s, a, vs, qs, l, em);
    };
    if (v.trav >= 3) return shape<EmitPaths<v4::TravAny>, 64, 5>(adaptive, f);
    if (v.trav >= 1) return shape<EmitPaths<v1::Trav>, 256, 1>(adaptive, f);
    return hipErrorInvalidValue;
}

// EMIT POWER (vrt_launch_accum_emitp.hip, vrt_launch_accum_hdr_emitp.hip): the same over EmitPowerPaths<...> (include/vrt.h
// vrt_set_emitter_importance, VRT_EMIT_POWER); the kernels' last argument is the EmitPower
template <bool HDR>
hipError_t full_emit_power(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const Filled<HDR> &q, bool adaptive,
                           const accum::Lens &l, const EmitPower &em, int grid, hipStream_t s) {
    const auto f = [&](auto sh) {
        using S = decltype(sh);
        const accum::ArgsOf<S::kAdapt, HDR> qs = slice<S::kAdapt, HDR>(q);
        if (src == accum::Source::kCorner)
            return go(accum::full_accum_kernel<accum::EmitPowerCornerSource, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, EmitPower>, grid, S::kBlock, s, a, vs, qs, em);
        if (src == accum::Source::kJitter)
            return go(accum::full_accum_kernel<accum::EmitPowerJitterSource, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, EmitPower>, grid, S::kBlock, s, a, vs, qs, em);
        return go(accum::full_accum_kernel<accum::EmitPowerLensSource, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, accum::Lens, EmitPower>, grid, S::kBlock, s, a, vs, qs, l, em);
    };
    if (v.trav >= 3) return shape<EmitPowerPaths<v4::TravAny>, 64, 5>(adaptive, f);
    if (v.trav >= 1) return shape<EmitPowerPaths<v1::Trav>, 256, 1>(adaptive, f);
    return hipErrorInvalidValue;
}

// EMIT MIS (vrt_launch_accum_emitm.hip, vrt_launch_accum_hdr_emitm.hip): the same over EmitMisPaths<...> (include/vrt.h
// vrt_set_emitter_mis); the kernels' last argument is the EmitMis
template <bool HDR>
hipError_t full_emit_mis(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const Filled<HDR> &q, bool adaptive,
                         const accum::Lens &l, const EmitMis &em, int grid, hipStream_t s) {
    const auto f = [&](auto sh) {
        using S = decltype(sh);
        const accum::ArgsOf<S::kAdapt, HDR> qs = slice<S::kAdapt, HDR>(q);
        if (src == accum::Source::kCorner)
            return go(accum::full_accum_kernel<accum::EmitMisCornerSource, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, EmitMis>, grid, S::kBlock, s, a, vs, qs, em);
        if (src == accum::Source::kJitter)
            return go(accum::full_accum_kernel<accum::EmitMisJitterSource, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, EmitMis>, grid, S::kBlock, s, a, vs, qs, em);
        return go(accum::full_accum_kernel<accum::EmitMisLensSource, typename S::Trav, S::kBlock, S::kWpe, S::kAdapt, HDR, accum::Lens, EmitMis>, grid, S::kBlock, s, a, vs, qs, l, em);
    };
    if (v.trav >= 3) return shape<EmitMisPaths<v4::TravAny>, 64, 5>(adaptive, f);
    if (v.trav >= 1) return shape<EmitMisPaths<v1::Trav>, 256, 1>(adaptive, f);
    return hipErrorInvalidValue;
}

template <bool HDR, bool DEEP = false, class... SUN>
hipError_t bounce(const KArgs &a, const ViewSet &vs, const Filled<HDR> &q, bool adaptive, int grid, hipStream_t s, const SUN &...sun) {
    if constexpr (sizeof...(SUN) != 0) {
        if (adaptive) return go(accum::bounce_accum_sun_kernel<SunPaths<v4::TravAny>, true, HDR>, grid, 64, s, a, vs, slice<true, HDR>(q), sun...);
        return go(accum::bounce_accum_sun_kernel<SunPaths<v4::TravAny>, false, HDR>, grid, 64, s, a, vs, slice<false, HDR>(q), sun...);
    } else {
        if (adaptive) return go(accum::bounce_accum_kernel<Path<DEEP, v4::TravAny>, true, HDR>, grid, 64, s, a, vs, slice<true, HDR>(q));
        return go(accum::bounce_accum_kernel<Path<DEEP, v4::TravAny>, false, HDR>, grid, 64, s, a, vs, slice<false, HDR>(q));
    }
}

}  // namespace accum_impl
}  // namespace launch
}  // namespace vrt
