// vrt_rays.hip.h -- pathTrace (comp:435-622) for rays the caller brings (include/vrt.h vrt_shade_rays): the fourth source of a
// sample's ray, after the accumulation's corner, jitter and lens sources (vrt_accum.hip.h). RaySource reads ray i's origin and
// direction from the caller's arrays, normalises the direction as pathTrace does on entry (comp:441: correctly rounded / and
// sqrt -- a caller's direction is in no proven range, so none of the in-range forms), looks the medium up at the lane's own
// floor(origin * u_voxelScale) (record_find()) and hands the LensRay to the shared trace_pixel<MODE, TRAV, false, true> /
// full::trace_pixel_full<TRAV, false, true>: the march, the shading and the path tracer are the frame's, not copies.
//
// One ray per lane, 64-lane workgroups, no LDS, no barrier. Nothing here is "at the eye": the kernels get a View with no first
// lookup, no ray tables and no miss mask, wide root 0 as uploaded (never tightened), and a traversal that is right for a start in
// any medium (v4::TravAny, v3, or the record-array traversals). KArgs::root0_only stays: find() applies it only to a ray whose own
// walk has been inside wide root 0, that moves forward on every axis and is in empty space -- conditions on the ray, not on where
// it started -- and never to a ray's first lookup ("Ray batches").
//
// Lane-to-ray mapping (ray_of_lane()): a batch that is an image -- rays::plan(): width >= 8 and at least two rows -- is cut into
// the frame kernels' 8 x 8 tiles, one per wave, because neighbouring pixels walk the same nodes; any other batch is a list, 64
// consecutive rays per wave. Either way ray i's random numbers are those of pixel (i % width, i / width).
//
// HDR forms (include/vrt.h vrt_shade_rays_hdr; template parameter HDR = true, arguments HdrArgs): the same kernels hand the float
// colour out of trace_pixel / trace_pixel_full, add h(c) of it to three float64 sums the lane keeps in registers -- read from
// HdrArgs::sums before the first sample and written back after the last, where the caller brings them -- and finish in the
// lane: mean, float store, tone map, bytes (finish_hdr()). No LDS: unlike the accumulation's 72- and 80-register sample kernels
// (vrt_accum.hip.h lds_put_hdr()) these run at 96 registers and more. Instantiated by vrt_launch_rays_hdr.hip alone.
#pragma once
#include "vrt_accum.hip.h"
#include "vrt_rays.h"

namespace vrt {
namespace rays {

// The kernel's third argument, re-read from the kernarg segment where it is used (as late_args() re-reads the first): it follows
// KArgs and ViewSet at its natural alignment
typedef const Args __attribute__((address_space(4))) *LateRays;
VRT_DEV LateRays late_rays() {
    constexpr size_t kViews = (sizeof(KArgs) + alignof(ViewSet) - 1) / alignof(ViewSet) * alignof(ViewSet);
    constexpr size_t kOffset = (kViews + sizeof(ViewSet) + alignof(Args) - 1) / alignof(Args) * alignof(Args);
    const char __attribute__((address_space(4))) *p = (const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr() + kOffset;
    asm volatile("" : "+s"(p));
    return (LateRays)p;
}

// This lane's ray i and its RNG pixel; false past the end of the batch
VRT_DEV bool ray_of_lane(const Args &q, uint32_t &i, int &px, int &py) {
    const uint32_t lane = threadIdx.x & 63u;
    if (q.tiles_x) {   // wave-uniform
        const uint32_t ty = blockIdx.x / q.tiles_x, tx = blockIdx.x - ty * q.tiles_x;
        const uint32_t x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
        const uint64_t at = (uint64_t)y * q.width + x;   // the last tile row may reach 8 * width past n: beyond 32 bits
        i = (uint32_t)at;
        px = (int)x; py = (int)y;
        return x < q.width && at < (uint64_t)q.n;
    }
    i = blockIdx.x * 64u + lane;
    const uint32_t y = i / q.width;
    px = (int)(i - y * q.width); py = (int)y;
    return i < q.n;
}

struct RaySource {
    // ray i as pathTrace takes it: eye0 / eye1 = the raw leaf words of the node that holds floor(origin * u_voxelScale)
    static VRT_DEV LensRay load(const KArgs &a, const Args &q, uint32_t i) {
        LensRay r;
        if (q.origin_stride == 0) {   // one origin for the batch: scalar loads
            r.o = F3{q.origins[0], q.origins[1], q.origins[2]};
        } else {
            const float *o = q.origins + (size_t)i * 3u;
            r.o = F3{o[0], o[1], o[2]};
        }
        const float *d = q.dirs + (size_t)i * 3u;
        const F3 dir{d[0], d[1], d[2]};
        r.dir = scale3(dir, 1.0f / __builtin_sqrtf(dot3(dir, dir)));   // comp:441
        record_find(a, floor_i3(scale3(r.o, a.voxel_scale)), r.eye0, r.eye1);
        return r;
    }
};

VRT_DEV void store(uint32_t i, uint32_t rgba, int2 idd) {
    const LateRays lq = late_rays();
    uint32_t *out_rgba = lq->out_rgba;
    int2 *out_id = lq->out_id;
    if (out_rgba) out_rgba[i] = rgba;
    if (out_id) out_id[i] = idd;
}

// HDR: the sums a lane starts from
VRT_DEV accum::HdrSum first_hdr(const double *sums, uint32_t i) {
    return sums ? accum::load_hdr(sums, i) : accum::HdrSum{0.0, 0.0, 0.0};
}

// HDR: the lane's sums after its last sample -> HdrArgs::sums, the mean over n_total, its tone-mapped bytes; the arguments re-read
// from the kernarg segment (HdrArgs begins with Args, at late_rays()'s place)
VRT_DEV void finish_hdr(uint32_t i, const accum::HdrSum &hs, int2 idd) {
    const HdrArgs __attribute__((address_space(4))) *lq = (const HdrArgs __attribute__((address_space(4))) *)late_rays();
    double *sums = lq->sums;
    float *out_rgb = lq->out_rgb;
    uint32_t *out_rgba = lq->out_rgba;
    int2 *out_id = lq->out_id;
    if (sums) accum::store_hdr(sums, i, hs);
    if (out_rgb || out_rgba) {
        const double n = (double)lq->n_total;
        const float m[3] = {(float)(hs.r / n), (float)(hs.g / n), (float)(hs.b / n)};
        if (out_rgb) { out_rgb[(size_t)i * 3 + 0] = m[0]; out_rgb[(size_t)i * 3 + 1] = m[1]; out_rgb[(size_t)i * 3 + 2] = m[2]; }
        if (out_rgba) {
            const int op = lq->op;
            const float e = lq->exposure;
            out_rgba[i] = unorm8(accum::tone_map(m[0], op, e)) | (unorm8(accum::tone_map(m[1], op, e)) << 8) |
                          (unorm8(accum::tone_map(m[2], op, e)) << 16) | (255u << 24);
        }
    }
    if (out_id) out_id[i] = idd;
}

// VRT_MODE_PRIMARY / _PRIMARY_SHADOW: no random number is drawn, so every sample is the same and one trace serves any n_samples
// (HDR: added as (double)h(c) * n_samples, accum::add_hdr_repeat())
template <int MODE, class TRAV, int WPE, bool HDR = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE))) void shade_rays_kernel(const KArgs a, const ViewSet vs, const ArgsOf<HDR> q) {
    typename TRAV::Ctx tc_;
    TRAV::block_init(a, tc_);
    uint32_t i;
    int px, py;
    if (!ray_of_lane(q, i, px, py)) return;
    const LensRay lr = RaySource::load(a, q, i);
    uint32_t rgba;
    int2 idd;
    LateOut lo;
    if constexpr (HDR) {
        float fc[3];
        trace_pixel<MODE, TRAV, false, true, false, true>(a, vs.v[0], tc_, px, py, rgba, idd, lo, nullptr, nullptr, 0u, &lr, 0u, fc);
        const HdrArgs __attribute__((address_space(4))) *lq = (const HdrArgs __attribute__((address_space(4))) *)late_rays();
        accum::HdrSum hs = first_hdr(lq->sums, i);
        accum::add_hdr_repeat(fc, lq->n_samples, hs);
        finish_hdr(i, hs, idd);
    } else {
        trace_pixel<MODE, TRAV, false, true>(a, vs.v[0], tc_, px, py, rgba, idd, lo, nullptr, nullptr, 0u, &lr);
        store(i, rgba, idd);
    }
}

// VRT_MODE_FULL, the general stack kernel (right for any scene and any origin). LOOP: samples first .. first + n_samples - 1 looped
// in the lane, the arguments and the ray re-read for every sample (held across the back edge they spill, vrt_accum.hip.h
// loop_args()); the medium's two words stay in registers. The mean is accum_resolve_kernel's: (sum + n / 2) / n per channel of the
// bytes each sample would store, alpha 255; the (voxel ID, dist) pair is the same for every sample.
// HDR: one add_hdr() per sample in sample order; LOOP carries the three float64 sums (six registers) across the back edge.
// X...: the argument of TRAV's family (vrt_common.hip.h: TRAV::Arg -- the Sun of SunPaths<...>, the Emit, EmitPower or EmitMis of the
// emitter families), a fourth argument of its own after the three that late_args(), late_view() and late_rays() re-read, which rides
// in the traversal's context; none for the plain traversals and DeepPaths<...>. One body for every family, as the accumulation's
// kernels take their Lens: under a shared __device__ body the kernel compiles to other code (profiles/sun_disc_codegen.txt), with
// the argument as a template parameter to the same (profiles/path_family_fold_codegen.txt).
template <class TRAV, int WPE, bool LOOP, bool HDR = false, class... X>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE))) void shade_rays_full_kernel(const KArgs a, const ViewSet vs, const ArgsOf<HDR> q, const X... arg) {
    typename TRAV::Ctx tc_;
    TRAV::block_init(a, tc_);
    if constexpr (sizeof...(X) != 0) TRAV::take(tc_, arg...);
    uint32_t i;
    int px, py;
    if (!ray_of_lane(q, i, px, py)) return;
    LensRay lr = RaySource::load(a, q, i);
    uint32_t rgba;
    int2 idd;
    LateOut lo;
    if constexpr (!LOOP && HDR) {
        float fc[3];
        full::trace_pixel_full<TRAV, false, true, true>(a, vs.v[0], tc_, px, py, rgba, idd, lo, q.first, &lr, fc);
        const HdrArgs __attribute__((address_space(4))) *lq = (const HdrArgs __attribute__((address_space(4))) *)late_rays();
        accum::HdrSum hs = first_hdr(lq->sums, i);
        accum::add_hdr(fc, hs);
        finish_hdr(i, hs, idd);
    } else if constexpr (!LOOP) {
        full::trace_pixel_full<TRAV, false, true>(a, vs.v[0], tc_, px, py, rgba, idd, lo, q.first, &lr);
    } else {
        const uint32_t eye0 = lr.eye0, eye1 = lr.eye1;
        uint32_t r = 0u, g = 0u, b = 0u;
        accum::HdrSum hs{};
        if constexpr (HDR) hs = first_hdr(q.sums, i);
        const uint32_t n = q.n_samples;
        for (uint32_t k = 0; k < n; ++k) {
#ifdef __HIP_DEVICE_COMPILE__
            const KArgs ak = *late_args();
            const View vk = *late_view();
            const Args qk = *late_rays();
#else
            const KArgs ak = a;
            const View vk = vs.v[0];
            const Args qk = q;
#endif
            const float *o = qk.origins + (qk.origin_stride ? (size_t)i * 3u : (size_t)0);
            const float *d = qk.dirs + (size_t)i * 3u;
            const F3 dir{d[0], d[1], d[2]};
            LensRay lk;
            lk.o = F3{o[0], o[1], o[2]};
            lk.dir = scale3(dir, 1.0f / __builtin_sqrtf(dot3(dir, dir)));
            lk.eye0 = eye0; lk.eye1 = eye1;
            if constexpr (HDR) {
                float fc[3];
                full::trace_pixel_full<TRAV, false, true, true>(ak, vk, tc_, px, py, rgba, idd, lo, qk.first + k, &lk, fc);
                accum::add_hdr(fc, hs);
            } else {
                full::trace_pixel_full<TRAV, false, true>(ak, vk, tc_, px, py, rgba, idd, lo, qk.first + k, &lk);
                r += rgba & 0xffu;
                g += (rgba >> 8) & 0xffu;
                b += (rgba >> 16) & 0xffu;
            }
        }
        if constexpr (HDR) {
            finish_hdr(i, hs, idd);
        } else {
            const uint32_t h = n >> 1;
            rgba = ((r + h) / n) | (((g + h) / n) << 8) | (((b + h) / n) << 16) | (255u << 24);
        }
    }
    if constexpr (!HDR) store(i, rgba, idd);
}

}  // namespace rays
}  // namespace vrt
