// vrt_accum.hip.h -- the progressive accumulation's kernels (include/vrt.h vrt_accum_*). Sample k of a pixel is the frame of the
// accumulation's mode rendered with initRNG(pixel, k) (comp:380-387; comp:629 itself passes 0) from the sample's ray: the same
// camera, uniforms and tree, only the random numbers and the ray differ. An accumulation keeps, per pixel and channel, the integer
// sum of the unorm8 bytes each sample would store -- exact and independent of the order of the adds -- and resolves it to
// (sum + n / 2) / n. Every kernel adds a launch's samples to the sums with one read-add-write of a pixel's sums, one lane per
// pixel: no atomics.
//
// A sample's ray comes from one of three sources (the template parameter SRC of the kernels below):
//   CornerSource  the pixel's corner, the frame's own ray: only the full path tracer's random numbers differ between samples
//   JitterSource  the ray moved from the corner by (jitter_x(k), jitter_y(k)) (VRT_ACCUM_JITTER, vrt_common.hip.h jittered_ray_dir())
//   LensSource    a thin lens (vrt_set_lens): the ray of lens_sample() (vrt_lens.hip.h), jittered or not per the accumulation's flags
// Sample 0 of every source is the frame itself. The jittered and lens accumulations, and those of VRT_MODE_PRIMARY / _SHADOW,
// take the frame's (voxel ID, dist) image from an ordinary frame rendered once per accumulation (vrt_accum.cpp); the corner
// source's one-sample kernel writes it.
//
// The kernels by shape and source (vrt_dispatch.cpp enqueue() picks one as it picks the form of a frame):
//   shape                                           corner                 jitter / lens
//   samples looped in the lanes, modes 0 / 1        repeat_kernel          primary_accum_kernel<JitterSource / LensSource, ...>
//   MODE 6's chain looped in the lanes (opaque)     bounce_accum_kernel    opaque_accum_kernel<JitterSource / LensSource, ...>
//   one sample per launch, the general full tracer  full_accum_kernel<CornerSource / JitterSource / LensSource, ...>
// The corner source has kernels of its own where a sample does not depend on its ray: a primary mode's every sample is the frame
// (repeat_kernel), and an opaque scene's pass 1 runs once per accumulation (bounce_accum_kernel). Then the resolve:
// accum_resolve_kernel (vrt_accum_state.hip.h, with the other kernels that only read or list the state).
//
// Adaptive accumulations (include/vrt.h vrt_accum_begin_adaptive) take the same kernels with the template parameter ADAPT = true:
// each lane reads its pixel's state (sums, its count n in the fourth word, Q) once, takes a round's sample only while
// adaptive_active() holds, and writes the state back once. The sample-looped kernels leave the loop at the pixel's stop;
// the one-sample kernels trace the tiles compact_tiles_kernel listed for the round and leave inactive lanes idle.
//
// HDR accumulations (include/vrt.h vrt_accum_keep_hdr) take the same kernels with the template parameter HDR = true: beside the
// bytes, the float colour each sample's unorm8() receives goes, clamped by hdr_value(), into three float64 sums per pixel, one
// add per sample in sample order -- so a lane reads its pixel's sums before its first sample and writes them after its last.
// Where every sample of a pixel is the same float c (repeat_kernel, the bounce kernel's sky and emissive pixels), k samples add
// (double)c * k: m * c is exact in a double for m <= 2^24, so the product equals the k adds. Those routes read the float from
// hdr_frame_kernel's image, which replaces the frame (or pass 1) they otherwise take the bytes from. Both, and hdr_resolve_kernel: vrt_accum_hdr.hip.h.
//
// Accumulations that keep moments (include/vrt.h vrt_accum_keep_moments, points M1-M3) take the HDR kernels with the template
// parameter MOM = true as well: each sample's luminance y = Y(h(c)) and its float32 square go into two more float64 sums per pixel,
// one add each where the colour sums take theirs, and k equal samples add (double)y * k and (double)q * k -- exact as above, y and
// q being floats. The repeat kernels' forms and the M3 resolve: vrt_accum_mom.hip.h.
#pragma once
#include "vrt_accum.h"
#include "vrt_hdr.hip.h"
#include "vrt_full.hip.h"
#include "vrt_lens.hip.h"

namespace vrt {
namespace accum {

VRT_DEV void add_bytes(uint32_t rgba, uint32_t &r, uint32_t &g, uint32_t &b) {
    r += rgba & 0xffu;
    g += (rgba >> 8) & 0xffu;
    b += (rgba >> 16) & 0xffu;
}

VRT_DEV void store_sums(uint32_t *sums, size_t o, uint32_t r, uint32_t g, uint32_t b) {
    uint4 *p = reinterpret_cast<uint4 *>(sums) + o;
    uint4 s = *p;
    s.x += r; s.y += g; s.z += b;
    *p = s;
}

// ---- adaptive state (ADAPT = true) ----
struct PixelState { uint32_t r, g, b, n; uint64_t q; };

VRT_DEV PixelState load_state(const AdaptArgs &q, size_t o) {
    const uint4 s = reinterpret_cast<const uint4 *>(q.sums)[o];
    return PixelState{s.x, s.y, s.z, s.w, q.sq[o]};
}

VRT_DEV void store_state(const AdaptArgs &q, size_t o, const PixelState &p) {
    reinterpret_cast<uint4 *>(q.sums)[o] = make_uint4(p.r, p.g, p.b, p.n);
    q.sq[o] = p.q;
}

VRT_DEV bool state_active(uint32_t min, uint32_t max, uint32_t tol, const PixelState &p) {
    return adaptive_active(p.n, (uint64_t)p.r + p.g + p.b, p.q, min, max, tol);
}

VRT_DEV void add_sample(uint32_t rgba, PixelState &p) {
    const uint32_t r = rgba & 0xffu, g = (rgba >> 8) & 0xffu, b = (rgba >> 16) & 0xffu, l = r + g + b;
    p.r += r; p.g += g; p.b += b;
    p.n += 1u;
    p.q += (uint64_t)(l * l);
}

// adds `k` more samples equal to rgba (l * l * k < 2^44)
VRT_DEV void add_repeat(uint32_t rgba, uint32_t k, PixelState &p) {
    const uint32_t r = rgba & 0xffu, g = (rgba >> 8) & 0xffu, b = (rgba >> 16) & 0xffu, l = r + g + b;
    p.r += r * k; p.g += g * k; p.b += b * k;
    p.n += k;
    p.q += (uint64_t)(l * l) * k;
}

// ---- HDR sums (HDR = true) ----
struct HdrSum { double r, g, b; };

// hdr_value(): h(c) of include/vrt.h, and tone_map(): vrt_hdr.hip.h

VRT_DEV HdrSum load_hdr(const double *hsum, size_t o) {
    const double *p = hsum + o * 3;
    return HdrSum{p[0], p[1], p[2]};
}
VRT_DEV void store_hdr(double *hsum, size_t o, const HdrSum &h) {
    double *p = hsum + o * 3;
    p[0] = h.r; p[1] = h.g; p[2] = h.b;
}
VRT_DEV void add_hdr(const float *fc, HdrSum &h) {
    h.r = h.r + (double)hdr_value(fc[0]);
    h.g = h.g + (double)hdr_value(fc[1]);
    h.b = h.b + (double)hdr_value(fc[2]);
}
// k more samples equal to fc, for a pixel whose every sample is fc (see above)
VRT_DEV void add_hdr_repeat(const float *fc, uint32_t k, HdrSum &h) {
    h.r = h.r + (double)hdr_value(fc[0]) * (double)k;
    h.g = h.g + (double)hdr_value(fc[1]) * (double)k;
    h.b = h.b + (double)hdr_value(fc[2]) * (double)k;
}

// The sample-looped kernels keep a lane's three float64 sums in LDS across the loop (24 bytes per lane), as the bounce kernel keeps
// its state, rather than six more live registers at budgets of 72 and 80 (what the HDR forms still spill: profiles/accum_resource_usage.txt)
VRT_DEV void lds_put_hdr(volatile double *p, int n, const HdrSum &h) { p[0] = h.r; p[n] = h.g; p[2 * n] = h.b; }
VRT_DEV HdrSum lds_get_hdr(volatile double *p, int n) { return HdrSum{p[0], p[n], p[2 * n]}; }
VRT_DEV void lds_add_hdr(volatile double *p, int n, const float *fc) {
    p[0] = p[0] + (double)hdr_value(fc[0]);
    p[n] = p[n] + (double)hdr_value(fc[1]);
    p[2 * n] = p[2 * n] + (double)hdr_value(fc[2]);
}

// ---- luminance moments (MOM = true): M1 and M2 of include/vrt.h vrt_accum_keep_moments ----
struct MomSum { double s1, s2; };

// y = Y(h(c)) with V1's Y and its association
VRT_DEV float mom_luminance(const float *fc) { return (0.2126f * hdr_value(fc[0]) + 0.7152f * hdr_value(fc[1])) + 0.0722f * hdr_value(fc[2]); }

VRT_DEV MomSum load_mom(const double *msum, size_t o) {
    const double *p = msum + o * 2;
    return MomSum{p[0], p[1]};
}
VRT_DEV void store_mom(double *msum, size_t o, const MomSum &m) {
    double *p = msum + o * 2;
    p[0] = m.s1; p[1] = m.s2;
}
VRT_DEV void add_mom(const float *fc, MomSum &m) {
    const float y = mom_luminance(fc), q = y * y;
    m.s1 = m.s1 + (double)y;
    m.s2 = m.s2 + (double)q;
}
VRT_DEV void add_mom_repeat(const float *fc, uint32_t k, MomSum &m) {
    const float y = mom_luminance(fc), q = y * y;
    m.s1 = m.s1 + (double)y * (double)k;
    m.s2 = m.s2 + (double)q * (double)k;
}
// ... in the LDS slots of the sample-looped kernels, planes 3 and 4 behind the three colour sums' (16 bytes more per lane)
VRT_DEV void lds_put_mom(volatile double *p, int n, const MomSum &m) { p[3 * n] = m.s1; p[4 * n] = m.s2; }
VRT_DEV MomSum lds_get_mom(volatile double *p, int n) { return MomSum{p[3 * n], p[4 * n]}; }
VRT_DEV void lds_add_mom(volatile double *p, int n, const float *fc) {
    const float y = mom_luminance(fc), q = y * y;
    p[3 * n] = p[3 * n] + (double)y;
    p[4 * n] = p[4 * n] + (double)q;
}

VRT_DEV size_t pixel_offset(const KArgs &a, int px, int py) { return (size_t)py * (size_t)a.width + (size_t)px; }

// This lane's pixel of 8 x 8 tile `tile` of a whole frame (KArgs: row0 = 0, n_rows = height, compact = 0)
VRT_DEV void tile_pixel(const KArgs &a, int tile, int &px, int &py) {
    const int lane = threadIdx.x & 63;
    const int tiles_x = (a.width + 7) / 8;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    px = tx * 8 + (lane & 7);
    py = ty * 8 + (lane >> 3);
}

// One 8 x 8 tile per wave, trace_kernel's tiles in order; false past the frame's edge. Written out rather than through
// tile_pixel(): with the tile computed ahead of the lane, the kernels' tile arithmetic compiles differently.
template <int BLOCK>
VRT_DEV bool frame_pixel(const KArgs &a, int &px, int &py) {
    const int lane = threadIdx.x & 63;
    const int tiles_x = (a.width + 7) / 8;
    const int tile = (int)blockIdx.x * (BLOCK / 64) + (int)(threadIdx.x >> 6);
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    px = tx * 8 + (lane & 7);
    py = ty * 8 + (lane >> 3);
    return px < a.width && py < a.height;
}

// An adaptive one-sample launch: wave w of the grid (sized for every tile) takes tile q.tiles[w] while w < *q.n_tiles
template <int BLOCK>
VRT_DEV bool listed_pixel(const KArgs &a, const AdaptArgs &q, int &px, int &py) {
    const uint32_t slot = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (slot >= *q.n_tiles) return false;
    tile_pixel(a, (int)q.tiles[slot], px, py);
    return px < a.width && py < a.height;
}

// The arguments of a sample loop, re-read from the kernarg segment for every sample (late_args(), late_view()): held in scalar
// registers across the loop's back edge they spill, into vector lanes and from there to scratch (20 SGPRs, then 18 VGPRs in the
// bounce kernel)
VRT_DEV KArgs loop_args(const KArgs &a) {
#ifdef __HIP_DEVICE_COMPILE__
    return *late_args();
#else
    return a;
#endif
}
VRT_DEV View loop_view(const ViewSet &vs) {
#ifdef __HIP_DEVICE_COMPILE__
    return *late_view();
#else
    return vs.v[0];
#endif
}

// ---- ray sources (JIT and LENS of trace_pixel and trace_pixel_full) ----
struct CornerSource { static constexpr bool kJitter = false, kLens = false; };
struct JitterSource { static constexpr bool kJitter = true, kLens = false; };
struct LensSource {
    static constexpr bool kJitter = false, kLens = true;
    const Lens &L;   // the kernel's Lens argument, read where it is used
};
// ... and the same three for the kernels over a family that takes an argument (vrt_common.hip.h: SunPaths<...> and the emitter
// families; A = TRAV::Arg): the kernel's last argument, handed to the traversal's context by TRAV::take()
template <class A> struct ArgCornerSource { static constexpr bool kJitter = false, kLens = false; const A &S; };
template <class A> struct ArgJitterSource { static constexpr bool kJitter = true, kLens = false; const A &S; };
template <class A> struct ArgLensSource {
    static constexpr bool kJitter = false, kLens = true;
    const Lens &L;
    const A &S;
};

// ---- the kernels of the three shapes ----
// L...: the lens kernels' fourth argument, the Lens. Each body is its kernel's own and writes out its trace call per source and its
// ADAPT pairs: a shared __device__ body under thin wrappers, the call as a member of the source, or an accumulator type over ADAPT
// each compile to different code (profiles/accum_kernel_fold_codegen.txt).

// q.n samples q.first, q.first + 1, ... of MODE 0 or 1, looped in the lanes: the traversal the frame kernel would take
// (trace_kernel's 8 x 8 tiles, its eye lookup and empty-octant proofs: the eye does not move), the shadow ray in MODE 1
template <class SRC, int MODE, class TRAV, int BLOCK, int WPE, bool ADAPT, bool HDR, bool MOM, class... L>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(WPE))) void primary_accum_kernel(const KArgs a, const ViewSet vs, const ArgsOf<ADAPT, HDR, MOM> q, const L... lens) {
    static_assert(HDR || !MOM, "the moments ride with the HDR sums");
    const SRC src{lens...};
    typename TRAV::Ctx tc_;
    TRAV::block_init(a, tc_);
    int px, py;
    if (!frame_pixel<BLOCK>(a, px, py)) return;
    uint32_t r = 0u, g = 0u, b = 0u;
    PixelState st{};
    __shared__ double s_hsum[HDR ? (MOM ? 5 : 3) : 1][HDR ? BLOCK : 1];   // (HDR = false: never touched, and dropped)
    volatile double *vs_hsum = &s_hsum[0][HDR ? threadIdx.x : 0];
    if constexpr (ADAPT) st = load_state(q, pixel_offset(a, px, py));
    if constexpr (HDR) lds_put_hdr(vs_hsum, BLOCK, load_hdr(q.hsum, pixel_offset(a, px, py)));
    if constexpr (MOM) lds_put_mom(vs_hsum, BLOCK, load_mom(q.msum, pixel_offset(a, px, py)));
    for (uint32_t k = 0; k < q.n; ++k) {
        if constexpr (ADAPT)
            if (!state_active(q.min, q.max, q.tol, st)) break;
        uint32_t rgba;
        int2 idd;
        LateOut lo;
        float fc[3];
        const KArgs ak = loop_args(a);
        const View vk = loop_view(vs);
        if constexpr (SRC::kLens) {
            const LensRay lr = lens_sample(ak, vk, src.L, px, py, q.first + k);
            if constexpr (HDR) trace_pixel<MODE, TRAV, false, true, false, true>(ak, vk, tc_, px, py, rgba, idd, lo, nullptr, nullptr, q.first + k, &lr, 0u, fc);
            else trace_pixel<MODE, TRAV, false, true>(ak, vk, tc_, px, py, rgba, idd, lo, nullptr, nullptr, q.first + k, &lr);
        } else if constexpr (HDR) trace_pixel<MODE, TRAV, SRC::kJitter, false, false, true>(ak, vk, tc_, px, py, rgba, idd, lo, nullptr, nullptr, q.first + k, nullptr, 0u, fc);
        else trace_pixel<MODE, TRAV, SRC::kJitter>(ak, vk, tc_, px, py, rgba, idd, lo, nullptr, nullptr, q.first + k);
        if constexpr (ADAPT) add_sample(rgba, st);
        else add_bytes(rgba, r, g, b);
        if constexpr (HDR) lds_add_hdr(vs_hsum, BLOCK, fc);
        if constexpr (MOM) lds_add_mom(vs_hsum, BLOCK, fc);
    }
    if constexpr (ADAPT) store_state(q, pixel_offset(a, px, py), st);
    else store_sums(q.sums, pixel_offset(a, px, py), r, g, b);
    if constexpr (HDR) store_hdr(q.hsum, pixel_offset(a, px, py), lds_get_hdr(vs_hsum, BLOCK));
    if constexpr (MOM) store_mom(q.msum, pixel_offset(a, px, py), lds_get_mom(vs_hsum, BLOCK));
}

// q.n samples of MODE 6's two stages, looped in the lanes: pass 1 from the sample's ray, its seed in registers, then bounce_pixel
// with initRNG's sample index; 64 lanes, one 8 x 8 tile per wave. Pass 1 depends on the sample, so it cannot be shared as
// bounce_accum_kernel shares it.
template <class SRC, class TRAV, int WPE, bool ADAPT, bool HDR, bool MOM, class... L>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE))) void opaque_accum_kernel(const KArgs a, const ViewSet vs, const ArgsOf<ADAPT, HDR, MOM> q, const L... lens) {
    static_assert(HDR || !MOM, "the moments ride with the HDR sums");
    const SRC src{lens...};
    typename TRAV::Ctx tc_;
    TRAV::block_init(a, tc_);
    if constexpr (sun_paths<TRAV>::value) TRAV::take(tc_, src.S);
    int px, py;
    if (!frame_pixel<64>(a, px, py)) return;
    uint32_t r = 0u, g = 0u, b = 0u;
    PixelState st{};
    __shared__ double s_hsum[HDR ? (MOM ? 5 : 3) : 1][HDR ? 64 : 1];
    volatile double *vs_hsum = &s_hsum[0][HDR ? threadIdx.x : 0];
    if constexpr (ADAPT) st = load_state(q, pixel_offset(a, px, py));
    if constexpr (HDR) lds_put_hdr(vs_hsum, 64, load_hdr(q.hsum, pixel_offset(a, px, py)));
    if constexpr (MOM) lds_put_mom(vs_hsum, 64, load_mom(q.msum, pixel_offset(a, px, py)));
    for (uint32_t k = 0; k < q.n; ++k) {
        if constexpr (ADAPT)
            if (!state_active(q.min, q.max, q.tol, st)) break;
        const uint32_t sample = q.first + k;
        uint32_t rgba, both;
        int2 idd;
        LateOut lo;
        Seed seed;
        seed.word = 0u;
        float fc[3];   // HDR: pass 1's colour, then the bounce's where the pixel has one -- as the bytes go
        const KArgs ak = loop_args(a);
        const View vk = loop_view(vs);
        if constexpr (SRC::kLens) {
            const LensRay lr = lens_sample(ak, vk, src.L, px, py, sample);
            if constexpr (HDR) trace_pixel<1, TRAV, false, true, false, true>(ak, vk, tc_, px, py, rgba, idd, lo, nullptr, &seed, sample, &lr, 0u, fc);
            else trace_pixel<1, TRAV, false, true>(ak, vk, tc_, px, py, rgba, idd, lo, nullptr, &seed, sample, &lr);
        } else if constexpr (HDR) trace_pixel<1, TRAV, SRC::kJitter, false, false, true>(ak, vk, tc_, px, py, rgba, idd, lo, nullptr, &seed, sample, nullptr, 0u, fc);
        else trace_pixel<1, TRAV, SRC::kJitter>(ak, vk, tc_, px, py, rgba, idd, lo, nullptr, &seed, sample);
        if constexpr (HDR) {
            if (full::bounce_pixel<TRAV, true>(ak, tc_, px, py, seed, both, sample, fc)) rgba = both;
        } else {
            if (full::bounce_pixel<TRAV>(ak, tc_, px, py, seed, both, sample)) rgba = both;
        }
        if constexpr (ADAPT) add_sample(rgba, st);
        else add_bytes(rgba, r, g, b);
        if constexpr (HDR) lds_add_hdr(vs_hsum, 64, fc);
        if constexpr (MOM) lds_add_mom(vs_hsum, 64, fc);
    }
    if constexpr (ADAPT) store_state(q, pixel_offset(a, px, py), st);
    else store_sums(q.sums, pixel_offset(a, px, py), r, g, b);
    if constexpr (HDR) store_hdr(q.hsum, pixel_offset(a, px, py), lds_get_hdr(vs_hsum, 64));
    if constexpr (MOM) store_mom(q.msum, pixel_offset(a, px, py), lds_get_mom(vs_hsum, 64));
}

// Sample q.first (q.n == 1) of the general full path tracer: trace_kernel<2>'s tiles, one pixel per lane.
// ADAPT: the waves take the round's listed tiles (listed_pixel()), and only active lanes trace.
template <class SRC, class TRAV, int BLOCK, int WPE, bool ADAPT, bool HDR, bool MOM, class... L>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(WPE))) void full_accum_kernel(const KArgs a, const ViewSet vs, const ArgsOf<ADAPT, HDR, MOM> q, const L... lens) {
    static_assert(HDR || !MOM, "the moments ride with the HDR sums");
    const SRC src{lens...};
    typename TRAV::Ctx tc_;
    TRAV::block_init(a, tc_);
    // (SunPaths<...>: the Sun assigned here, not through its take() -- with the call seven of this kernel's forms compile to the same
    // instructions in another order and other registers, profiles/path_family_fold_codegen.txt)
    if constexpr (emit_paths<TRAV>::value) TRAV::take(tc_, src.S);
    else if constexpr (sun_paths<TRAV>::value) tc_.sun = src.S;
    int px, py;
    if constexpr (ADAPT) {
        if (!listed_pixel<BLOCK>(a, q, px, py)) return;
    } else {
        if (!frame_pixel<BLOCK>(a, px, py)) return;
    }
    PixelState st{};
    if constexpr (ADAPT) {
        st = load_state(q, pixel_offset(a, px, py));
        if (!state_active(q.min, q.max, q.tol, st)) return;
    }
    uint32_t rgba;
    int2 idd;
    LateOut lo;
    float fc[3];
    if constexpr (SRC::kLens) {
        const LensRay lr = lens_sample(a, vs.v[0], src.L, px, py, q.first);
        if constexpr (HDR) full::trace_pixel_full<TRAV, false, true, true>(a, vs.v[0], tc_, px, py, rgba, idd, lo, q.first, &lr, fc);
        else full::trace_pixel_full<TRAV, false, true>(a, vs.v[0], tc_, px, py, rgba, idd, lo, q.first, &lr);
    } else if constexpr (HDR) full::trace_pixel_full<TRAV, SRC::kJitter, false, true>(a, vs.v[0], tc_, px, py, rgba, idd, lo, q.first, nullptr, fc);
    else full::trace_pixel_full<TRAV, SRC::kJitter>(a, vs.v[0], tc_, px, py, rgba, idd, lo, q.first);
    if constexpr (HDR) {   // one sample: the pixel's sums read, added to and written here
        HdrSum hs = load_hdr(q.hsum, pixel_offset(a, px, py));
        add_hdr(fc, hs);
        store_hdr(q.hsum, pixel_offset(a, px, py), hs);
    }
    if constexpr (MOM) {
        MomSum ms = load_mom(q.msum, pixel_offset(a, px, py));
        add_mom(fc, ms);
        store_mom(q.msum, pixel_offset(a, px, py), ms);
    }
    if constexpr (ADAPT) {
        add_sample(rgba, st);
        store_state(q, pixel_offset(a, px, py), st);
    } else {
        uint32_t r = 0u, g = 0u, b = 0u;
        add_bytes(rgba, r, g, b);
        store_sums(q.sums, pixel_offset(a, px, py), r, g, b);
    }
    if constexpr (!SRC::kJitter && !SRC::kLens) q.out_id[pixel_offset(a, px, py)] = idd;   // no frame of its own: the id_dist is the samples'
}

// One wave per 8 x 8 tile of a whole frame (KArgs: row0 = 0, n_rows = height, compact = 0); a.defer_rec holds pass 1's seeds in
// the tile-major planes of MODE 4 / 5 (vrt_common.hip.h kSeedPlanes). Built as MODE 5 is: 64 lanes, seven waves per SIMD, whose
// 72 registers MODE 5's bounce fills. The loop's own state -- the seed, which MODE 5 lets die at the march, and the three sums --
// waits in LDS (2 KiB per wave; 28 waves per CU hold 56 of its 160 KiB) instead of in spilled registers: the lane loads its seed
// from memory once, and each sample reads it back from LDS and adds its bytes there.
// ADAPT: the loop stops at the pixel's stop (n and Q in registers); sky and emissive pixels, whose every sample is the same,
// take adaptive_constant_count() at once.
// HDR: the three float64 sums wait in LDS too (1.5 KiB more per wave: 98 of the CU's 160 KiB at 28 waves); sky and emissive pixels
// take their float colour from q.hframe, which hdr_frame_kernel wrote as it ran pass 1.
// Over DeepPaths<...> (a path depth above 1: full::bounce_chain()) the kernels of the opaque route are built for fewer waves per SIMD
// than their depth-1 twins, at the budget where the chain's loop-carried state -- origin, direction, tint, colour, RNG, medium, live
// across every segment's march and shadow ray -- stays in registers: no scratch (profiles/path_depth_resource_usage.txt; at the
// twins' 72 and 80 registers the compiler parks 16-71 of them in scratch around the marches, inside the depth loop).
// X...: the Sun of SunPaths<...> (include/vrt.h vrt_set_sun_disc) as a fourth argument of its own, none for the other traversals:
// full::bounce_pixel() then ignores the seed's lit bit and casts the depth-0 shadow ray per sample.
template <class TRAV, bool ADAPT, bool HDR>
constexpr int bounce_wpe() { return deep_paths<TRAV>::value ? (ADAPT && HDR ? 3 : 4) : 7; }
constexpr int kDeepOpaqueWpe = 4;   // opaque_accum_kernel over DeepPaths<...> (vrt_launch_accum.hip.h)
// MOM: the two moment sums wait there as well (1 KiB more per wave: 126 KiB at 28 waves); sky and emissive pixels take y and q from the
// same float colour.
template <class TRAV, bool ADAPT = false, bool HDR = false, bool MOM = false, class... X>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(bounce_wpe<TRAV, ADAPT, HDR>()))) void bounce_accum_kernel(const KArgs a, const ViewSet vs, const ArgsOf<ADAPT, HDR, MOM> q, const X... arg) {
    static_assert(HDR || !MOM, "the moments ride with the HDR sums");
    __shared__ uint32_t s_seed[kSeedPlanes][64];
    __shared__ uint32_t s_sum[3][64];
    __shared__ double s_hsum[HDR ? (MOM ? 5 : 3) : 1][HDR ? 64 : 1];   // (HDR = false: never touched, and dropped)
    typename TRAV::Ctx tc_;
    TRAV::block_init(a, tc_);
    if constexpr (sizeof...(X) != 0) ((tc_.sun = arg), ...);   // the one Sun, assigned as full_accum_kernel assigns it and for its reason
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x;
    int px, py;
    tile_pixel(a, tile, px, py);
    if (px >= a.width || py >= a.height) return;
    const uint32_t *sp = reinterpret_cast<const uint32_t *>(a.defer_rec) + ((size_t)tile * kSeedPlanes) * 64 + lane;
    const uint32_t word = sp[3 * 64];
    uint32_t r = 0u, g = 0u, b = 0u;
    PixelState st{};
    HdrSum hs{};
    if constexpr (ADAPT) st = load_state(q, (size_t)py * (size_t)a.width + (size_t)px);
    if constexpr (HDR) hs = load_hdr(q.hsum, (size_t)py * (size_t)a.width + (size_t)px);
    MomSum ms{};
    if constexpr (MOM) ms = load_mom(q.msum, (size_t)py * (size_t)a.width + (size_t)px);
    if (word & kSeedValid) {
#pragma unroll
        for (uint32_t p = 0; p < kSeedPlanes; ++p) s_seed[p][lane] = sp[p * 64];
        if constexpr (ADAPT) {
            s_sum[0][lane] = st.r; s_sum[1][lane] = st.g; s_sum[2][lane] = st.b;
        } else {
            s_sum[0][lane] = 0u; s_sum[1][lane] = 0u; s_sum[2][lane] = 0u;
        }
        // volatile: the seed is read back for every sample, not hoisted into registers across the loop
        volatile uint32_t *vs_seed = &s_seed[0][0];
        volatile uint32_t *vs_sum = &s_sum[0][0];
        volatile double *vs_hsum = &s_hsum[0][0];
        if constexpr (HDR) { vs_hsum[0 * 64 + lane] = hs.r; vs_hsum[1 * 64 + lane] = hs.g; vs_hsum[2 * 64 + lane] = hs.b; }
        if constexpr (MOM) lds_put_mom(vs_hsum + lane, 64, ms);
        // every sample is bounce_pixel's own arithmetic on the same seed: direct term, then the bounce's term, then unorm8
        for (uint32_t k = 0; k < q.n; ++k) {
            if constexpr (ADAPT) {
                st.r = vs_sum[0 * 64 + lane]; st.g = vs_sum[1 * 64 + lane]; st.b = vs_sum[2 * 64 + lane];
                if (!state_active(q.min, q.max, q.tol, st)) break;
            }
            Seed seed;
            seed.hp = F3{__uint_as_float(vs_seed[0 * 64 + lane]), __uint_as_float(vs_seed[1 * 64 + lane]), __uint_as_float(vs_seed[2 * 64 + lane])};
            seed.word = vs_seed[3 * 64 + lane];
            seed.iof = __uint_as_float(vs_seed[4 * 64 + lane]);
            const KArgs ak = loop_args(a);
            uint32_t rgba = 0u;
            if constexpr (HDR) {
                float fc[3] = {0.0f, 0.0f, 0.0f};
                full::bounce_pixel<TRAV, true>(ak, tc_, px, py, seed, rgba, q.first + k, fc);
                vs_hsum[0 * 64 + lane] = vs_hsum[0 * 64 + lane] + (double)hdr_value(fc[0]);
                vs_hsum[1 * 64 + lane] = vs_hsum[1 * 64 + lane] + (double)hdr_value(fc[1]);
                vs_hsum[2 * 64 + lane] = vs_hsum[2 * 64 + lane] + (double)hdr_value(fc[2]);
                if constexpr (MOM) lds_add_mom(vs_hsum + lane, 64, fc);
            } else full::bounce_pixel<TRAV>(ak, tc_, px, py, seed, rgba, q.first + k);
            vs_sum[0 * 64 + lane] = vs_sum[0 * 64 + lane] + (rgba & 0xffu);
            vs_sum[1 * 64 + lane] = vs_sum[1 * 64 + lane] + ((rgba >> 8) & 0xffu);
            vs_sum[2 * 64 + lane] = vs_sum[2 * 64 + lane] + ((rgba >> 16) & 0xffu);
            if constexpr (ADAPT) {
                const uint32_t l = (rgba & 0xffu) + ((rgba >> 8) & 0xffu) + ((rgba >> 16) & 0xffu);
                st.n += 1u;
                st.q += (uint64_t)(l * l);
            }
        }
        r = vs_sum[0 * 64 + lane]; g = vs_sum[1 * 64 + lane]; b = vs_sum[2 * 64 + lane];
        if constexpr (HDR) { hs.r = vs_hsum[0 * 64 + lane]; hs.g = vs_hsum[1 * 64 + lane]; hs.b = vs_hsum[2 * 64 + lane]; }
        if constexpr (MOM) ms = lds_get_mom(vs_hsum + lane, 64);
    } else if constexpr (ADAPT) {
        const uint32_t more = adaptive_constant_count(st.n, q.n, q.min) - st.n;
        add_repeat(q.pass1_rgba[(size_t)py * (size_t)a.width + (size_t)px], more, st);
        r = st.r; g = st.g; b = st.b;
        if constexpr (HDR) add_hdr_repeat(q.hframe + ((size_t)py * (size_t)a.width + (size_t)px) * 3, more, hs);
        if constexpr (MOM) add_mom_repeat(q.hframe + ((size_t)py * (size_t)a.width + (size_t)px) * 3, more, ms);
    } else {   // sky, emissive surfaces: pass 1's bytes are every sample's
        add_bytes(q.pass1_rgba[(size_t)py * (size_t)a.width + (size_t)px], r, g, b);
        r *= q.n; g *= q.n; b *= q.n;
        if constexpr (HDR) add_hdr_repeat(q.hframe + ((size_t)py * (size_t)a.width + (size_t)px) * 3, q.n, hs);
        if constexpr (MOM) add_mom_repeat(q.hframe + ((size_t)py * (size_t)a.width + (size_t)px) * 3, q.n, ms);
    }
    if constexpr (HDR) store_hdr(q.hsum, (size_t)py * (size_t)a.width + (size_t)px, hs);
    if constexpr (MOM) store_mom(q.msum, (size_t)py * (size_t)a.width + (size_t)px, ms);
    if constexpr (ADAPT) {
        st.r = r; st.g = g; st.b = b;
        store_state(q, (size_t)py * (size_t)a.width + (size_t)px, st);
    } else {
        store_sums(q.sums, (size_t)py * (size_t)a.width + (size_t)px, r, g, b);
    }
}

// A primary mode from the corner: every sample is the frame in q.frame_rgba, so n samples add n times its bytes
// (HDR: and n times its float colour in q.hframe)
template <bool HDR>
__global__ __launch_bounds__(256) void repeat_kernel(const typename std::conditional<HDR, RepeatHdrOf<Repeat>, Repeat>::type q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= q.pixels) return;
    uint32_t r = 0u, g = 0u, b = 0u;
    add_bytes(q.frame_rgba[i], r, g, b);
    store_sums(q.sums, i, r * q.n, g * q.n, b * q.n);
    if constexpr (HDR) {
        HdrSum hs = load_hdr(q.hsum, i);
        add_hdr_repeat(q.hframe + (size_t)i * 3, q.n, hs);
        store_hdr(q.hsum, i, hs);
    }
}

// the same for an adaptive accumulation: q.n rounds of a sample that never changes take each pixel to
// adaptive_constant_count(), with no trace at all
template <bool HDR>
__global__ __launch_bounds__(256) void repeat_adaptive_kernel(const typename std::conditional<HDR, RepeatHdrOf<RepeatAdapt>, RepeatAdapt>::type q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= q.pixels) return;
    AdaptArgs s{};
    s.sums = q.sums;
    s.sq = q.sq;
    PixelState st = load_state(s, i);
    const uint32_t more = adaptive_constant_count(st.n, q.n, q.min) - st.n;
    add_repeat(q.frame_rgba[i], more, st);
    store_state(s, i, st);
    if constexpr (HDR) {
        HdrSum hs = load_hdr(q.hsum, i);
        add_hdr_repeat(q.hframe + (size_t)i * 3, more, hs);
        store_hdr(q.hsum, i, hs);
    }
}

}  // namespace accum
}  // namespace vrt
