// vrt_launch.h -- the seam between the host code of libvrt_hip.so and its device code. Only the vrt_launch_*.hip files include
// kernel headers; everything else launches through these functions.
#pragma once
#include "vrt_internal.h"
#include "vrt_query.h"
#include "vrt_accum.h"
#include "vrt_rays.h"
#include "vrt_guides.h"
#include "vrt_filter.h"
#include "vrt_temporal.h"
#include "vrt_upsample.h"
#include "vrt_meter.h"
#include "vrt_bloom.h"

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

// The family of path tracer kernels a VRT_MODE_FULL sample launch takes (vrt_common.hip.h: the traversal itself, or its DeepPaths,
// SunPaths, EmitPaths, EmitPowerPaths or EmitMisPaths wrapper; each family honours what the ones before it do), and the argument
// block of the last one, which holds every other family's: EmitMis{EmitPower{Emit{Sun, list, n}, cdf}, inv_power}. A kernel is handed
// its own family's slice. select_paths() (vrt_scene.cpp) derives both from the settings a caller read (vrt_internal.h PathSetup).
enum class PathFamily { kPlain, kDeep, kSun, kEmit, kEmitPower, kEmitMis };
using PathArgs = EmitMis;
// `fam` and `pa` for a launch of `mode` whose light direction is light_dir. An empty list gives the launches of sampling off, the
// mode VRT_EMIT_POWER counts only with sampling, MIS only with that mode, a sun of radius 0 makes no block, the primary modes read
// none of it. false: emitter sampling on an opaque route (`opaque`), which has no such kernels.
bool select_paths(int mode, const vrt_internal::PathSetup &p, const float light_dir[3], bool opaque, PathFamily &fam, PathArgs &pa);

// vrt_launch_accum.hip: the progressive accumulation (vrt_accum.hip.h), whole frames, one 8 x 8 tile per wave. One launch per
// shape, for the ray source `src` (l: the lens of Source::kLens, read for that source only) and, with `adaptive`, the kernels'
// adaptive forms, which read all of q; the others read its Args part. `q` is filled for either object, `hdr` picks it (the plain
// functions take q's AdaptArgs part). hipErrorInvalidValue: no kernel of that shape.
// accum_primary: q.n samples of `mode` (0 or 1) from the jitter or lens source, `v` as the dispatcher normalises it for an
// accumulation (v4 64/7, v3 64/6, v2 or v1 256/1). accum_repeat: n frames' bytes. adaptive_resolve: by each pixel's own count.
// adaptive_counts: vrt_accum_counts.
hipError_t accum_primary(int mode, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::AdaptArgs &q,
                         bool adaptive, const accum::Lens &l, int grid, hipStream_t s);
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
hipError_t accum_repeat_hdr(const accum::RepeatHdrOf<accum::Repeat> &q, hipStream_t s);
hipError_t accum_repeat_hdr(const accum::RepeatHdrOf<accum::RepeatAdapt> &q, hipStream_t s);
hipError_t accum_frame_hdr(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::HdrFrame &q, int grid, hipStream_t s);
hipError_t accum_pass1_hdr(const KArgs &a, const ViewSet &vs, const accum::HdrFrame &q, int grid, hipStream_t s);
hipError_t accum_resolve_hdr(const accum::HdrResolve &q, hipStream_t s);
// vrt_launch_accum_mom.hip: the same for HDR accumulations that keep moments (include/vrt.h vrt_accum_keep_moments), `q` with the two
// moment sums too. accum_repeat_mom: the HDR repeat with (double)y * k and (double)q * k of the frame's float colour.
// accum_variance: M3, the sums -> the variance plane.
hipError_t accum_primary_mom(int mode, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::MomArgs &q,
                             bool adaptive, const accum::Lens &l, int grid, hipStream_t s);
hipError_t accum_repeat_mom(const accum::RepeatMomOf<accum::Repeat> &q, hipStream_t s);
hipError_t accum_repeat_mom(const accum::RepeatMomOf<accum::RepeatAdapt> &q, hipStream_t s);
hipError_t accum_variance(const accum::MomVariance &q, hipStream_t s);
inline hipError_t accum_primary(bool hdr, bool moments, int mode, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs,
                                const accum::MomArgs &q, bool adaptive, const accum::Lens &l, int grid, hipStream_t s) {
    if (hdr && moments) return accum_primary_mom(mode, src, v, a, vs, q, adaptive, l, grid, s);
    return hdr ? accum_primary_hdr(mode, src, v, a, vs, q, adaptive, l, grid, s) : accum_primary(mode, src, v, a, vs, q, adaptive, l, grid, s);
}

// The sample launches of VRT_MODE_FULL over the family F (vrt_launch_accum.hip.h), one explicit instantiation per object:
// vrt_launch_accum.hip and vrt_launch_accum_hdr.hip hold the plain family's, vrt_launch_accum{,_hdr}_{deep,sun,emit,emitp,emitm}.hip
// one other family's each. opaque: q.n samples of the opaque full path tracer from the jitter or lens source (v4, 64 lanes). full:
// one sample (q.first) of the general full path tracer in the traversal and workgroup shape of `v` (grid = tiles / waves per
// workgroup) -- every family but the plain one takes any variant and launches v4 for the wide traversals, v1 for the record-array
// ones (same workgroup shape, same bytes); adaptive, it traces the tiles adaptive_tiles listed before it. bounce: q.n samples of the
// diffuse bounce over pass 1's seeds in a.defer_rec (grid = tiles). The emitter families have `full` only.
// MOM (with HDR): the forms that keep moments, vrt_launch_accum_mom{,_deep,_sun,_emit,_emitp,_emitm}.hip.
template <bool HDR, PathFamily F, bool MOM = false>
struct AccumPaths {
    static hipError_t opaque(accum::Source src, const KArgs &a, const ViewSet &vs, const accum::MomArgs &q, bool adaptive, const accum::Lens &l,
                             const PathArgs &pa, int grid, hipStream_t s);
    static hipError_t full(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const accum::MomArgs &q, bool adaptive,
                           const accum::Lens &l, const PathArgs &pa, int grid, hipStream_t s);
    static hipError_t bounce(const KArgs &a, const ViewSet &vs, const accum::MomArgs &q, bool adaptive, const PathArgs &pa, int grid, hipStream_t s);
};
// ... and the one switch from the family as a value to those instantiations (vrt_scene.cpp, which sees none of the kernels): `q`
// filled for every object, `form` picks it
enum class AccumForm { kPlain, kHdr, kMoments };
inline AccumForm accum_form(bool hdr, bool moments) { return hdr ? (moments ? AccumForm::kMoments : AccumForm::kHdr) : AccumForm::kPlain; }
hipError_t accum_opaque(AccumForm form, PathFamily fam, const PathArgs &pa, accum::Source src, const KArgs &a, const ViewSet &vs,
                        const accum::MomArgs &q, bool adaptive, const accum::Lens &l, int grid, hipStream_t s);
hipError_t accum_full(AccumForm form, PathFamily fam, const PathArgs &pa, accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs,
                      const accum::MomArgs &q, bool adaptive, const accum::Lens &l, int grid, hipStream_t s);
hipError_t accum_bounce(AccumForm form, PathFamily fam, const PathArgs &pa, const KArgs &a, const ViewSet &vs, const accum::MomArgs &q,
                        bool adaptive, int grid, hipStream_t s);

// vrt_launch_rays.hip: pathTrace of `mode` (0 or 1) for the q.n rays of a caller's batch (vrt_rays.hip.h), one lane per ray in the
// mapping rays::plan() chose (grid = its waves); `v`: the dispatcher's variant, of which only the traversal is taken -- every kernel
// here starts a ray in any medium. ev0 / ev1 as for trace_primary.
hipError_t shade_rays(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const rays::Args &q, uint32_t grid, hipStream_t s,
                      hipEvent_t ev0, hipEvent_t ev1);
// vrt_launch_rays_hdr.hip: the same kernels' HDR forms (include/vrt.h vrt_shade_rays_hdr): q.n_samples is the call's own,
// q.out_rgba takes the tone-mapped bytes of the mean
hipError_t shade_rays_hdr(int mode, const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, uint32_t grid, hipStream_t s,
                          hipEvent_t ev0, hipEvent_t ev1);
// VRT_MODE_FULL of the two over the family F (vrt_launch_rays_paths.hip.h), q.n_samples samples looped in the lane; one explicit
// instantiation per object, vrt_launch_rays{,_hdr}{,_deep,_sun,_emit,_emitp,_emitm}.hip. The plain forms take q's Args part.
template <bool HDR, PathFamily F>
struct RayPaths {
    static hipError_t full(const Variant &v, const KArgs &a, const ViewSet &vs, const rays::HdrArgs &q, const PathArgs &pa, uint32_t grid,
                           hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
};
hipError_t shade_rays_full(bool hdr, PathFamily fam, const PathArgs &pa, const Variant &v, const KArgs &a, const ViewSet &vs,
                           const rays::HdrArgs &q, uint32_t grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);

// vrt_launch_guides.hip: the guide planes (vrt_guides.hip.h). accum_guides: samples q.first .. q.first + q.n - 1 of every pixel of a
// whole frame into the guide state, for the ray source `src` (l: the lens of Source::kLens), `v`, `a`, `vs` and `grid` as the
// dispatcher makes them for an accumulation's launch of VRT_MODE_PRIMARY. guides_resolve: the state -> the four float planes.
// guide_rays: one march per ray of a caller's batch, its planes stored at once (grid = rays::plan()'s waves; `v`: the traversal only).
hipError_t accum_guides(accum::Source src, const Variant &v, const KArgs &a, const ViewSet &vs, const guides::Args &q, const accum::Lens &l, bool glass,
                        int grid, hipStream_t s);
hipError_t guides_resolve(const guides::Resolve &q, hipStream_t s);
hipError_t guide_rays(const Variant &v, const KArgs &a, const ViewSet &vs, const guides::RayArgs &q, bool glass, uint32_t grid, hipStream_t s);

// vrt_launch_filter.hip: the guided filter and its variance-guided form (vrt_filter.hip.h), whole frames, one lane per pixel.
// filter_prepass: the caller's guide planes -> the packed planes; filter_variance: after it, the initial variance into the packed
// planes (q.variance null: the spatial estimate); filter_level: one level's taps at the step of q (first: reads the caller's image;
// last: writes the outputs), guide-only or variance-guided by the argument's type; filter_through: levels == 0.
hipError_t filter_prepass(const filter::Prepass &q, hipStream_t s);
hipError_t filter_variance(const filter::Variance &q, hipStream_t s);
hipError_t filter_level(const filter::Level &q, bool first, bool last, hipStream_t s);
hipError_t filter_level(const filter::LevelVar &q, bool first, bool last, hipStream_t s);
hipError_t filter_through(const filter::Through &q, hipStream_t s);

// vrt_launch_temporal.hip: the temporal pass (vrt_temporal.hip.h), a whole frame, one lane per pixel, one 8 x 8 tile per wave:
// T1-T6 of include/vrt.h vrt_temporal_hdr from q's planes and (where given) its previous history into the new one.
hipError_t temporal_pass(const temporal::Args &q, hipStream_t s);
// ... and the kernel's second form: T3s, T7 and T6m of vrt_temporal_hdr_mom
hipError_t temporal_pass_mom(const temporal::ArgsMom &q, hipStream_t s);

// vrt_launch_upsample.hip: the guided upsampling pass (vrt_upsample.hip.h), a whole HIGH frame, one lane per high pixel, one 8 x 8
// tile per wave: U1-U6 of include/vrt.h vrt_upsample_hdr from q's low image and planes and its high planes.
hipError_t upsample_pass(const upsample::Args &q, hipStream_t s);

// vrt_launch_meter.hip: light metering (vrt_meter.hip.h). meter_histogram: E1-E3 of include/vrt.h vrt_meter_hdr, the rows of q into
// q.histogram, which the caller has zeroed on s, on a capped grid; meter_finish: E4-E8, the histogram -> the record, one workgroup;
// meter_tonemap: E9, q.n pixels on a capped grid; vec: q.rgb and q.out_rgba are both multiples of 16.
hipError_t meter_histogram(const meter::HistArgs &q, hipStream_t s);
hipError_t meter_finish(const meter::FinishArgs &q, hipStream_t s);
hipError_t meter_tonemap(const meter::ToneArgs &q, bool vec, hipStream_t s);

// vrt_launch_bloom.hip: bloom (vrt_bloom.hip.h). bloom_down: one level of B4 of include/vrt.h vrt_bloom_hdr, a lane per destination
// pixel; first: q.rgb through the bright pass (B2, and B3 with karis), else q.src. bloom_up: one step of B6 in place, or with `last`
// the composite and the tone map (B7, B8).
hipError_t bloom_down(const bloom::DownArgs &q, bool first, bool karis, hipStream_t s);
hipError_t bloom_up(const bloom::UpArgs &q, bool last, hipStream_t s);

}  // namespace launch
}  // namespace vrt
