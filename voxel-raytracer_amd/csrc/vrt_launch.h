// vrt_launch.h -- the seam between the host code of libvrt_hip.so and its device code. Only the vrt_launch_*.hip files include
// kernel headers; everything else launches through these functions.
#pragma once
#include "vrt_internal.h"
#include "vrt_query.h"
#include "vrt_accum.h"
#include "vrt_rays.h"

namespace vrt {
namespace launch {

// trace_kernel<MODE, ...> for the variant the dispatcher settled on (vrt_launch_primary / _shadow / _full .hip). ev0 / ev1 (both
// or neither): events attached to THIS dispatch packet, so their elapsed time is the kernel's own begin-to-end time.
// hipErrorInvalidValue: no kernel of that shape.
hipError_t trace_primary(const Variant &v, const KArgs &a, const ViewSet &vs, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
hipError_t trace_shadow(const Variant &v, const KArgs &a, const ViewSet &vs, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
hipError_t trace_full(const Variant &v, const KArgs &a, const ViewSet &vs, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
// The full path tracer as two tile-coherent passes (vrt_full.hip.h bounce_pixel) for scenes the dispatcher has checked: pass 1 = the
// primary + shadow kernel leaving a seed per pixel in a.defer_rec, pass 2 = the diffuse bounce of the seeded pixels. ev0 rides on
// pass 1, ev1 on pass 2 (their elapsed time spans both).
// ... and the same two stages in ONE kernel, the seed in registers (no stack, no seed traffic, no second launch); wpe 5, 6 or 7
hipError_t trace_full_opaque(const KArgs &a, const ViewSet &vs, int grid, int wpe, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
hipError_t trace_full_two_pass(const KArgs &a, const ViewSet &vs, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
// pass 1 of the two-pass form alone (the progressive accumulation runs it once and the bounce once per sample)
hipError_t trace_full_pass1(const KArgs &a, const ViewSet &vs, int grid, hipStream_t s);
inline hipError_t trace(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    return mode == VRT_MODE_FULL ? trace_full(v, a, vs, grid, s, ev0, ev1)
                                 : (mode == VRT_MODE_PRIMARY ? trace_primary(v, a, vs, grid, s, ev0, ev1) : trace_shadow(v, a, vs, grid, s, ev0, ev1));
}

// vrt_launch_misc.hip
// tile_order_kernel: the per-tile ticks of one launch -> the group order of the next ones. raise_lds: set the kernel's dynamic-LDS
// ceiling first (once per device; needed above 48 KiB).
// wave_slots: waves the chip holds of the kernel the order is for (KArgs::split_count is 0 unless the heaviest tile outlasts its even share); 0: no split count
hipError_t tile_order(const uint32_t *d_cost, uint32_t n_groups, uint32_t *d_order, uint32_t wave_slots, bool raise_lds, size_t lds_ceiling, hipStream_t s);
// miss tiles (vrt_miss.h): d_mask = a header word, a spare word, then v.tiles_x * v.tiles_y bytes, none of which (header included)
// holds `stamp` before the build; writes `stamp` to the tiles the n boxes may be seen through, and to the header word when one of
// them reaches the eye's plane (every tile traced)
hipError_t miss_mask(const miss::ViewParams &v, const int *d_boxes, uint32_t n, uint32_t *d_mask, uint8_t stamp, hipStream_t s);
// checks on the device that the kernarg segment is laid out as late_args() / late_view() assume; *d_bad += mismatches
hipError_t kernarg_probe(const KArgs &a, const ViewSet &vs, uint32_t *d_bad, hipStream_t s);

// the display pass (vrt_denoise.hip.h): 32 x 16-pixel tiles, two pixels per lane (tiles_x / n_tiles: its tiling; whole_groups: a
// 1-D grid of whole scheduling groups that reads group_order / writes tile_cost when given).
struct Denoise {
    const void *rgba, *id;
    void *out;
    int width, height;
    const uint32_t *group_order;
    uint32_t *tile_cost;
    int rows_path = 0;   // denoise::Args::rows_path
};
void denoise_tiling(int width, int height, int &tiles_x, int &n_tiles);
hipError_t denoise(const Denoise &d, bool whole_groups, hipStream_t s);
// vrt_launch_denoise_hdr.hip: the same pass on a float image (include/vrt.h vrt_denoise_hdr): rgb in, the filtered floats and / or
// their tone-mapped bytes out (either may be null), the tiling and the scheduling arguments as above
struct DenoiseHdr {
    const void *rgb, *id;
    void *out_rgb, *out_rgba;
    int width, height;
    const uint32_t *group_order;
    uint32_t *tile_cost;
    int rows_path = 0;
    int op = 0;              // VRT_TONEMAP_*
    float exposure = 1.0f;
};
hipError_t denoise_hdr(const DenoiseHdr &d, bool whole_groups, hipStream_t s);

// vrt_launch_query.hip: the world queries (vrt_query.hip.h), one lane per ray / point; a carries the scene part of KArgs only
hipError_t cast_rays(const KArgs &a, const query::RayArgs &q, hipStream_t s);
hipError_t find_voxels(const KArgs &a, const query::PointArgs &q, hipStream_t s);

// vrt_launch_accum.hip: the progressive accumulation (vrt_accum.hip.h), whole frames, one 8 x 8 tile per wave. One launch per
// shape, for the ray source `src` (l: the lens of Source::kLens, read for that source only) and, with `adaptive`, the kernels'
// adaptive forms, which read all of q; the others read its Args part. hipErrorInvalidValue: no kernel of that shape.
// accum_primary: q.n samples of `mode` (0 or 1) from the jitter or lens source, `v` as the dispatcher normalises it for an
// accumulation (v4 64/7, v3 64/6, v2 or v1 256/1). accum_opaque: q.n samples of the opaque full path tracer from the jitter or
// lens source (v4, 64 lanes). accum_full: one sample (q.first) of the general full path tracer in the traversal and workgroup
// shape of `v` (grid = tiles / waves per workgroup); adaptive, it traces the tiles adaptive_tiles listed before it.
// accum_bounce: q.n samples of the diffuse bounce over pass 1's seeds in a.defer_rec (grid = tiles). accum_repeat: n frames'
// bytes. adaptive_resolve: by each pixel's own count. adaptive_counts: vrt_accum_counts.
hipError_t accum_primary(int mode, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q,
                         bool adaptive, const accum::Lens &l, int grid, hipStream_t s);
hipError_t accum_opaque(accum::Source src, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive, const accum::Lens &l,
                        int grid, hipStream_t s);
hipError_t accum_full(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive,
                      const accum::Lens &l, int grid, hipStream_t s);
hipError_t accum_bounce(const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive, int grid, hipStream_t s);
hipError_t accum_repeat(const accum::Repeat &q, hipStream_t s);
hipError_t accum_repeat(const accum::RepeatAdapt &q, hipStream_t s);
hipError_t accum_resolve(const accum::Resolve &q, hipStream_t s);
hipError_t adaptive_resolve(const accum::Resolve &q, hipStream_t s);
hipError_t adaptive_tiles(const accum::Tiles &t, hipStream_t s);
hipError_t adaptive_counts(const accum::Counts &c, hipStream_t s);

// vrt_launch_accum_hdr.hip: the same for HDR accumulations (include/vrt.h vrt_accum_keep_hdr), `q` with the float64 sums and the
// corner frame's float image. accum_frame_hdr: the frame of `mode` (0 or 1) from the corner with its float colour, in accum_primary's
// shapes; accum_pass1_hdr: pass 1 of the opaque path likewise (trace_full_pass1's outputs and the floats). accum_resolve_hdr: the
// float mean and its tone-mapped bytes.
hipError_t accum_primary_hdr(int mode, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q,
                             bool adaptive, const accum::Lens &l, int grid, hipStream_t s);
hipError_t accum_opaque_hdr(accum::Source src, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive, const accum::Lens &l,
                            int grid, hipStream_t s);
hipError_t accum_full_hdr(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive,
                          const accum::Lens &l, int grid, hipStream_t s);
hipError_t accum_bounce_hdr(const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive, int grid, hipStream_t s);
hipError_t accum_repeat_hdr(const accum::RepeatHdrOf<accum::Repeat> &q, hipStream_t s);
hipError_t accum_repeat_hdr(const accum::RepeatHdrOf<accum::RepeatAdapt> &q, hipStream_t s);
hipError_t accum_frame_hdr(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrFrame &q, int grid, hipStream_t s);
hipError_t accum_pass1_hdr(const KArgs &a, const ViewSet &vs, const accum::HdrFrame &q, int grid, hipStream_t s);
hipError_t accum_resolve_hdr(const accum::HdrResolve &q, hipStream_t s);
// One call per shape of a sample launch: `q` filled for either object, `hdr` picks it (the plain functions take q's AdaptArgs part)
inline hipError_t accum_primary(bool hdr, int mode, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs,
                                const accum::HdrArgs &q, bool adaptive, const accum::Lens &l, int grid, hipStream_t s) {
    return hdr ? accum_primary_hdr(mode, src, v, a, vs, q, adaptive, l, grid, s) : accum_primary(mode, src, v, a, vs, q, adaptive, l, grid, s);
}
inline hipError_t accum_opaque(bool hdr, accum::Source src, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive,
                               const accum::Lens &l, int grid, hipStream_t s) {
    return hdr ? accum_opaque_hdr(src, a, vs, q, adaptive, l, grid, s) : accum_opaque(src, a, vs, q, adaptive, l, grid, s);
}
inline hipError_t accum_full(bool hdr, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q,
                             bool adaptive, const accum::Lens &l, int grid, hipStream_t s) {
    return hdr ? accum_full_hdr(src, v, a, vs, q, adaptive, l, grid, s) : accum_full(src, v, a, vs, q, adaptive, l, grid, s);
}
inline hipError_t accum_bounce(bool hdr, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive, int grid, hipStream_t s) {
    return hdr ? accum_bounce_hdr(a, vs, q, adaptive, grid, s) : accum_bounce(a, vs, q, adaptive, grid, s);
}

// vrt_launch_accum_deep.hip, vrt_launch_accum_hdr_deep.hip: the sample launches of VRT_MODE_FULL at a path depth above 1 (include/vrt.h
// vrt_set_path_depth): the same shapes and arguments, kernels that read a.path_depth. accum_full_deep takes any variant and launches
// v4 for the wide traversals, v1 for the record-array ones (same workgroup shape, same bytes).
hipError_t accum_opaque_deep(accum::Source src, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive, const accum::Lens &l,
                             int grid, hipStream_t s);
hipError_t accum_full_deep(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive,
                           const accum::Lens &l, int grid, hipStream_t s);
hipError_t accum_bounce_deep(const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive, int grid, hipStream_t s);
hipError_t accum_opaque_hdr_deep(accum::Source src, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive, const accum::Lens &l,
                                 int grid, hipStream_t s);
hipError_t accum_full_hdr_deep(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive,
                               const accum::Lens &l, int grid, hipStream_t s);
hipError_t accum_bounce_hdr_deep(const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive, int grid, hipStream_t s);
inline hipError_t accum_opaque_deep(bool hdr, accum::Source src, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive,
                                    const accum::Lens &l, int grid, hipStream_t s) {
    return hdr ? accum_opaque_hdr_deep(src, a, vs, q, adaptive, l, grid, s) : accum_opaque_deep(src, a, vs, q, adaptive, l, grid, s);
}
inline hipError_t accum_full_deep(bool hdr, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q,
                                  bool adaptive, const accum::Lens &l, int grid, hipStream_t s) {
    return hdr ? accum_full_hdr_deep(src, v, a, vs, q, adaptive, l, grid, s) : accum_full_deep(src, v, a, vs, q, adaptive, l, grid, s);
}
inline hipError_t accum_bounce_deep(bool hdr, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive, int grid, hipStream_t s) {
    return hdr ? accum_bounce_hdr_deep(a, vs, q, adaptive, grid, s) : accum_bounce_deep(a, vs, q, adaptive, grid, s);
}

// vrt_launch_accum_sun.hip, vrt_launch_accum_hdr_sun.hip: the same launches with a sun disc (include/vrt.h vrt_set_sun_disc), at any
// path depth: kernels over SunPaths<...>, which take `sun` (vrt_sun.h sun_block()) as their last argument
hipError_t accum_opaque_sun(accum::Source src, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive, const accum::Lens &l,
                            const Sun &sun, int grid, hipStream_t s);
hipError_t accum_full_sun(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive,
                          const accum::Lens &l, const Sun &sun, int grid, hipStream_t s);
hipError_t accum_bounce_sun(const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive, const Sun &sun, int grid, hipStream_t s);
hipError_t accum_opaque_hdr_sun(accum::Source src, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive, const accum::Lens &l,
                                const Sun &sun, int grid, hipStream_t s);
hipError_t accum_full_hdr_sun(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive,
                              const accum::Lens &l, const Sun &sun, int grid, hipStream_t s);
hipError_t accum_bounce_hdr_sun(const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive, const Sun &sun, int grid, hipStream_t s);
inline hipError_t accum_opaque_sun(bool hdr, accum::Source src, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive,
                                   const accum::Lens &l, const Sun &sun, int grid, hipStream_t s) {
    return hdr ? accum_opaque_hdr_sun(src, a, vs, q, adaptive, l, sun, grid, s) : accum_opaque_sun(src, a, vs, q, adaptive, l, sun, grid, s);
}
inline hipError_t accum_full_sun(bool hdr, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q,
                                 bool adaptive, const accum::Lens &l, const Sun &sun, int grid, hipStream_t s) {
    return hdr ? accum_full_hdr_sun(src, v, a, vs, q, adaptive, l, sun, grid, s) : accum_full_sun(src, v, a, vs, q, adaptive, l, sun, grid, s);
}
inline hipError_t accum_bounce_sun(bool hdr, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive, const Sun &sun, int grid,
                                   hipStream_t s) {
    return hdr ? accum_bounce_hdr_sun(a, vs, q, adaptive, sun, grid, s) : accum_bounce_sun(a, vs, q, adaptive, sun, grid, s);
}

// vrt_launch_accum_emit.hip, vrt_launch_accum_hdr_emit.hip: one sample of the general full path tracer with emitter sampling
// (include/vrt.h vrt_set_emitter_sampling), at any path depth and sun radius: kernels over EmitPaths<...>, which take `em` -- the
// context's emitter list and the launch's Sun -- as their last argument. The opaque routes have no such form.
hipError_t accum_full_emit(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive,
                           const accum::Lens &l, const Emit &em, int grid, hipStream_t s);
hipError_t accum_full_hdr_emit(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive,
                               const accum::Lens &l, const Emit &em, int grid, hipStream_t s);
inline hipError_t accum_full_emit(bool hdr, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q,
                                  bool adaptive, const accum::Lens &l, const Emit &em, int grid, hipStream_t s) {
    return hdr ? accum_full_hdr_emit(src, v, a, vs, q, adaptive, l, em, grid, s) : accum_full_emit(src, v, a, vs, q, adaptive, l, em, grid, s);
}

// vrt_launch_accum_emitp.hip, vrt_launch_accum_hdr_emitp.hip: the same with VRT_EMIT_POWER (include/vrt.h vrt_set_emitter_importance):
// kernels over EmitPowerPaths<...>, which take `em` -- the Emit and the list's table of thresholds -- as their last argument
hipError_t accum_full_emitp(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive,
                            const accum::Lens &l, const EmitPower &em, int grid, hipStream_t s);
hipError_t accum_full_hdr_emitp(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive,
                                const accum::Lens &l, const EmitPower &em, int grid, hipStream_t s);
inline hipError_t accum_full_emitp(bool hdr, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q,
                                   bool adaptive, const accum::Lens &l, const EmitPower &em, int grid, hipStream_t s) {
    return hdr ? accum_full_hdr_emitp(src, v, a, vs, q, adaptive, l, em, grid, s) : accum_full_emitp(src, v, a, vs, q, adaptive, l, em, grid, s);
}

// vrt_launch_accum_emitm.hip, vrt_launch_accum_hdr_emitm.hip: the same with vrt_set_emitter_mis on top of VRT_EMIT_POWER (include/vrt.h):
// kernels over EmitMisPaths<...>, which take `em` -- the EmitPower and 1 / Wtot -- as their last argument
hipError_t accum_full_emitm(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q, bool adaptive,
                            const accum::Lens &l, const EmitMis &em, int grid, hipStream_t s);
hipError_t accum_full_hdr_emitm(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q, bool adaptive,
                                const accum::Lens &l, const EmitMis &em, int grid, hipStream_t s);
inline hipError_t accum_full_emitm(bool hdr, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrArgs &q,
                                   bool adaptive, const accum::Lens &l, const EmitMis &em, int grid, hipStream_t s) {
    return hdr ? accum_full_hdr_emitm(src, v, a, vs, q, adaptive, l, em, grid, s) : accum_full_emitm(src, v, a, vs, q, adaptive, l, em, grid, s);
}

// vrt_launch_rays.hip: pathTrace of `mode` for the q.n rays of a caller's batch (vrt_rays.hip.h), one lane per ray in the mapping
// rays::plan() chose (grid = its waves); `v`: the dispatcher's variant, of which only the traversal is taken -- every kernel here
// starts a ray in any medium. VRT_MODE_FULL loops q.n_samples samples in the lane. ev0 / ev1 as for trace_primary.
hipError_t shade_rays(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, uint32_t grid, hipStream_t s,
                      hipEvent_t ev0, hipEvent_t ev1);
// vrt_launch_rays_hdr.hip: the same kernels' HDR forms (include/vrt.h vrt_shade_rays_hdr): q.n_samples is the call's own in every
// mode, q.out_rgba takes the tone-mapped bytes of the mean
hipError_t shade_rays_hdr(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, uint32_t grid, hipStream_t s,
                          hipEvent_t ev0, hipEvent_t ev1);

// vrt_launch_rays_deep.hip, vrt_launch_rays_hdr_deep.hip: VRT_MODE_FULL of the two above at a path depth above 1 (kernels that read
// a.path_depth; v4 for the wide variants, v1 for the record-array ones)
hipError_t shade_rays_deep(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, uint32_t grid, hipStream_t s, hipEvent_t ev0,
                           hipEvent_t ev1);
hipError_t shade_rays_hdr_deep(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, uint32_t grid, hipStream_t s,
                               hipEvent_t ev0, hipEvent_t ev1);

// vrt_launch_rays_sun.hip, vrt_launch_rays_hdr_sun.hip: VRT_MODE_FULL of the same with a sun disc, at any path depth
hipError_t shade_rays_sun(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, const Sun &sun, uint32_t grid, hipStream_t s,
                          hipEvent_t ev0, hipEvent_t ev1);
hipError_t shade_rays_hdr_sun(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, const Sun &sun, uint32_t grid,
                              hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);

// vrt_launch_rays_emit.hip, vrt_launch_rays_hdr_emit.hip: VRT_MODE_FULL of the same with emitter sampling, at any path depth and sun radius
hipError_t shade_rays_emit(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, const Emit &em, uint32_t grid, hipStream_t s,
                           hipEvent_t ev0, hipEvent_t ev1);
hipError_t shade_rays_hdr_emit(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, const Emit &em, uint32_t grid,
                               hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);

// vrt_launch_rays_emitp.hip, vrt_launch_rays_hdr_emitp.hip: ... and with VRT_EMIT_POWER (vrt_set_emitter_importance)
hipError_t shade_rays_emitp(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, const EmitPower &em, uint32_t grid, hipStream_t s,
                            hipEvent_t ev0, hipEvent_t ev1);
hipError_t shade_rays_hdr_emitp(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, const EmitPower &em, uint32_t grid,
                                hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);

// vrt_launch_rays_emitm.hip, vrt_launch_rays_hdr_emitm.hip: ... and with vrt_set_emitter_mis on top of VRT_EMIT_POWER
hipError_t shade_rays_emitm(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, const EmitMis &em, uint32_t grid, hipStream_t s,
                            hipEvent_t ev0, hipEvent_t ev1);
hipError_t shade_rays_hdr_emitm(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, const EmitMis &em, uint32_t grid,
                                hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);

}  // namespace launch
}  // namespace vrt
