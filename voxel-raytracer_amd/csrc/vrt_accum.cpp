// vrt_accum.cpp -- progressive multi-sample accumulation (include/vrt.h vrt_accum_*): call-order checks, the restart rule, the
// context's buffers, the resolve and the display pass on it. The samples themselves are enqueued by the dispatcher
// (vrt_dispatch.cpp enqueue() with an AccumStep), which settles the variant and the shape the mode and scene allow as it does
// for a frame; launch_accum_step() below then picks the kernel of vrt_accum.hip.h by the sample's ray source (corner, jitter
// or thin lens) and fills its arguments from the context's buffers. A jittered
// accumulation, or one of VRT_MODE_PRIMARY / _SHADOW, first renders the mode's ordinary frame once: its id_dist is the resolve's,
// and without jitter its bytes are every sample's. So does one with a thin lens (vrt_set_lens, aperture > 0).
// An adaptive accumulation (vrt_accum_begin_adaptive) adds rounds instead of samples: the same paths with the kernels' adaptive
// forms, its per-pixel counts and Q beside the sums, the resolve by each pixel's count, and vrt_accum_counts.
// An HDR accumulation (vrt_accum_keep_hdr before the begin) keeps three float64 sums per pixel of the samples' float colours too:
// the kernels' HDR forms, 24 + 12 bytes per pixel allocated only then, and vrt_accum_resolve_hdr's mean and tone map. Where the
// samples are all one frame, that frame comes from the HDR frame kernel, which hands out its float colour.
// One that keeps moments too (vrt_accum_keep_moments): 16 bytes per pixel more for the two float64 sums of the samples' luminance and
// its square, the kernels' MOM forms, and vrt_accum_variance's plane (M3).
#include "vrt_stage.h"
#include "vrt_launch.h"

#include <cstring>

using namespace vrt_internal;

namespace {

using Accum = vrt_ctx::Accum;

// does the next sample still belong to the samples in the sums? (camera block, uniforms and tree as at the first of them)
// vrt_set_emitter_mis where a full-mode add reads it: sampling on, a list that is not empty (ensure_emitters() has run by then) and
// VRT_EMIT_POWER. Elsewhere the flag is no input: a change there does not restart.
bool mis_read(const vrt_ctx *c) {
    return c->emitter_mis && c->emitter_sampling && c->emitters.n > 0 && c->emitter_importance == VRT_EMIT_POWER;
}

bool same_inputs(const vrt_ctx *c, const Accum &ac) {
    return std::memcmp(ac.inv_proj, c->inv_proj, sizeof ac.inv_proj) == 0 && std::memcmp(ac.inv_view, c->inv_view, sizeof ac.inv_view) == 0 &&
           std::memcmp(ac.cam_pos, c->cam_pos, sizeof ac.cam_pos) == 0 && std::memcmp(&ac.params, &c->params, sizeof ac.params) == 0 &&
           std::memcmp(ac.lens, c->lens, sizeof ac.lens) == 0 && (ac.mode != VRT_MODE_FULL || (ac.path_depth == c->path_depth && ac.sun_disc == c->sun_disc && ac.emitter_sampling == c->emitter_sampling && ac.emitter_importance == c->emitter_importance && ac.emitter_mis == mis_read(c))) &&   // the primary modes ignore the depth, the sun disc, emitter sampling, its mode and its MIS
           ac.tree_gen == c->tree_gen;
}

void take_inputs(const vrt_ctx *c, Accum &ac) {
    std::memcpy(ac.inv_proj, c->inv_proj, sizeof ac.inv_proj);
    std::memcpy(ac.inv_view, c->inv_view, sizeof ac.inv_view);
    std::memcpy(ac.cam_pos, c->cam_pos, sizeof ac.cam_pos);
    std::memcpy(ac.lens, c->lens, sizeof ac.lens);
    ac.path_depth = c->path_depth;
    ac.sun_disc = c->sun_disc;
    ac.emitter_sampling = c->emitter_sampling;
    ac.emitter_importance = c->emitter_importance;
    ac.emitter_mis = mis_read(c);
    ac.params = c->params;
    ac.tree_gen = c->tree_gen;
}

// sums -> rgba8 into d_rgba, the frame's id_dist into d_id (either may be null), the display pass into d_shown (needs d_rgba)
int resolve_into(vrt_ctx *c, void *d_rgba, void *d_id, void *d_shown, hipStream_t s) {
    Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    if (d_rgba) {
        vrt::accum::Resolve q{ac.d_sums, static_cast<uint32_t *>(d_rgba), ac.total, (uint32_t)px};
        VRT_HIP(c, ac.adaptive ? vrt::launch::adaptive_resolve(q, s) : vrt::launch::accum_resolve(q, s));
    }
    if (d_id) VRT_HIP(c, hipMemcpyAsync(d_id, ac.d_id, px * 8, hipMemcpyDeviceToDevice, s));
    if (d_shown) return vrt_denoise(c, ac.width, ac.height, d_rgba, ac.d_id, d_shown, s);
    return VRT_OK;
}

// vrt_accum_resolve_hdr*: the call-order checks of a resolve, an HDR accumulation, a tone map the header defines
int resolve_hdr_state(vrt_ctx *c, const char *what, const vrt_tonemap *tm) {
    const int r = accum_state(c, what, true);
    return r ? r : check_tonemap(c, what, tm);
}

// vrt_accum_variance*: the call-order checks of an HDR resolve, an accumulation that keeps moments, an output
int variance_state(vrt_ctx *c, const char *what, const void *out) {
    const int r = accum_state(c, what, true);
    if (r) return r;
    if (!c->accum.moments)
        return vrt_fail(c, VRT_E_STATE, std::string(what) + ": the accumulation keeps no moments (vrt_accum_keep_moments before the begin)");
    return out ? VRT_OK : vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null output");
}

// float64 sums -> float mean into d_rgb, its tone-mapped rgba8 into d_rgba (either may be null), the display pass into d_shown
int resolve_hdr_into(vrt_ctx *c, float *d_rgb, const vrt_tonemap *tm, void *d_rgba, void *d_shown, hipStream_t s) {
    Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    if (d_rgb || d_rgba) {
        const vrt::accum::HdrResolve q{ac.d_hsum, ac.d_sums, d_rgb, static_cast<uint32_t *>(d_rgba), ac.total, ac.adaptive ? 1u : 0u,
                                       (uint32_t)px, tm ? tm->op : VRT_TONEMAP_CLAMP, tm ? tm->exposure : 1.0f};
        VRT_HIP(c, vrt::launch::accum_resolve_hdr(q, s));
    }
    if (d_shown) return vrt_denoise(c, ac.width, ac.height, d_rgba, ac.d_id, d_shown, s);
    return VRT_OK;
}

// vrt_accum_resolve_hdr_shown*: the float mean's scratch (12 bytes per pixel), the accumulation's own, made at the first such call --
// an HDR accumulation that never asks for the filtered mean keeps its footprint. Every use of it is ordered on the context's stream:
// a caller's stream is joined back through Accum::read.
// So is d_hrgb, the float image's way to the host (vrt_accum_resolve_hdr, _hdr_shown): made at the first call that asks for it.
int ensure_float_image(vrt_ctx *c, DevBuf<float> &buf, size_t px) {
    return px * 12 <= buf.bytes() ? VRT_OK : reserve_synced(c, {{&buf, px * 12}});
}

// The HDR display pass on the accumulation: the existing resolve launch writes the float mean (exactly vrt_accum_resolve_hdr's
// out_rgb) into the scratch, vrt_denoise_hdr filters it with the accumulation's id_dist image. Two launches on purpose: the display
// pass stages every pixel about eight times across its tiles' halos, and 28 bytes of sums and count per staged tap against 12 of
// mean -- with a float64 divide each -- loses to one more pass over the frame.
int resolve_hdr_shown_into(vrt_ctx *c, const vrt_tonemap *tm, void *d_shown_rgb, void *d_shown_rgba, hipStream_t s) {
    Accum &ac = c->accum;
    const int r = resolve_hdr_into(c, ac.d_hmean, tm, nullptr, nullptr, s);
    if (r) return r;
    return vrt_denoise_hdr(c, ac.width, ac.height, ac.d_hmean, ac.d_id, tm, d_shown_rgb, d_shown_rgba, s);
}

// vrt_accum_begin_ex, and with rule = {min, max, tolerance} vrt_accum_begin_adaptive
int begin(vrt_ctx *c, int width, int height, int mode, uint32_t first_sample, uint32_t flags, const uint32_t *rule) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (mode != VRT_MODE_PRIMARY && mode != VRT_MODE_PRIMARY_SHADOW && mode != VRT_MODE_FULL)
        return vrt_fail(c, VRT_E_INVALID, rule ? "vrt_accum_begin_adaptive: unknown mode" : "vrt_accum_begin_ex: unknown mode");
    if (flags & ~(uint32_t)VRT_ACCUM_JITTER) return vrt_fail(c, VRT_E_INVALID, rule ? "vrt_accum_begin_adaptive: unknown flags" : "vrt_accum_begin_ex: unknown flags");
    VRT_HIP(c, hipSetDevice(c->device));
    Accum &ac = c->accum;
    const size_t px = (size_t)width * (size_t)height;
    const size_t tiles = (size_t)((width + 7) / 8) * (size_t)((height + 7) / 8);
    // each group grows together, after the samples in flight that still write the old buffers (reserve_synced waits for them); a
    // begin that cannot have its buffers ends the accumulation
    if (px > ac.pixels || tiles > ac.seed_tiles) {
        ac.begun = false;
        if ((r = reserve_synced(c, {{&ac.d_sums, px * 16}, {&ac.d_pass1, px * 4}, {&ac.d_id, px * 8},
                                    {&ac.d_seed, tiles * 64 * vrt::kSeedPlanesHost * 4}})))
            return r;
        ac.pixels = px;
        ac.seed_tiles = tiles;
    }
    if (rule && (px > ac.sq_pixels || tiles > ac.tile_cap)) {   // the adaptive state: Q per pixel, the round's tile list
        ac.begun = false;
        if ((r = reserve_synced(c, {{&ac.d_sq, px * 8}, {&ac.d_tiles, (tiles + 2) * 4}}))) return r;
        ac.sq_pixels = px;
        ac.tile_cap = tiles;
    }
    if (c->accum_keep_hdr && px > ac.hdr_pixels) {   // the HDR state: the float64 sums, the corner frame's float colour
        ac.begun = false;
        if ((r = reserve_synced(c, {{&ac.d_hsum, px * 24}, {&ac.d_hframe, px * 12}}))) return r;
        ac.hdr_pixels = px;
    }
    if (c->accum_keep_hdr && c->accum_keep_moments && px > ac.mom_pixels) {   // the moments: S1 and S2
        ac.begun = false;
        if ((r = reserve_synced(c, {{&ac.d_msum, px * 16}}))) return r;
        ac.mom_pixels = px;
    }
    if (!ac.added) VRT_HIP(c, hipEventCreateWithFlags(&ac.added, hipEventDisableTiming));
    if (!ac.read) VRT_HIP(c, hipEventCreateWithFlags(&ac.read, hipEventDisableTiming));
    ac.begun = true;
    ++ac.epoch;   // the sums start: a guide state of earlier samples (vrt_guides.cpp) is void
    ac.width = width;
    ac.height = height;
    ac.first = first_sample;
    ac.mode = mode;
    ac.flags = flags;
    ac.total = 0;
    ac.pass1 = false;
    ac.frame = false;
    ac.adaptive = rule != nullptr;
    ac.min_samples = rule ? rule[0] : 0u;
    ac.max_samples = rule ? rule[1] : 0u;
    ac.tolerance = rule ? rule[2] : 0u;
    ac.hdr = c->accum_keep_hdr;
    ac.moments = ac.hdr && c->accum_keep_moments;
    ac.guide_glass = c->guide_glass;
    return VRT_OK;
}

}  // namespace

int vrt_internal::accum_variance_into(vrt_ctx *c, float *d_variance, hipStream_t s) {
    Accum &ac = c->accum;
    const vrt::accum::MomVariance q{ac.d_msum, ac.d_sums, d_variance, ac.total, ac.adaptive ? 1u : 0u, (uint32_t)((size_t)ac.width * (size_t)ac.height)};
    VRT_HIP(c, vrt::launch::accum_variance(q, s));
    return VRT_OK;
}

int vrt_internal::ensure_variance_plane(vrt_ctx *c) {
    Accum &ac = c->accum;
    const size_t bytes = (size_t)ac.width * (size_t)ac.height * 4;
    return bytes <= ac.d_mvar.bytes() ? VRT_OK : reserve_synced(c, {{&ac.d_mvar, bytes}});
}

bool vrt_internal::accum_inputs_current(const vrt_ctx *c) { return same_inputs(c, c->accum); }

int vrt_internal::accum_state(vrt_ctx *c, const char *what, bool need_hdr) {
    if (!c) return VRT_E_INVALID;
    if (!c->accum.begun) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": no accumulation (call vrt_accum_begin first)");
    if (c->accum.total == 0) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": the accumulation holds no samples (call vrt_accum_add first)");
    if (need_hdr && !c->accum.hdr)
        return vrt_fail(c, VRT_E_STATE, std::string(what) + ": the accumulation keeps no HDR sums (vrt_accum_keep_hdr before the begin)");
    return VRT_OK;
}

// the step's samples go into the context's sums; an adaptive accumulation (acc.adaptive) passes its rule and state too, to the
// kernels' adaptive forms, an HDR one (acc.hdr) its float64 sums, to the HDR object's
hipError_t vrt_internal::launch_accum_step(Accum &ac, vrt::KArgs &a, vrt::ViewSet &vs, const Variant &v, int mode, int grid, bool two_pass,
                                           const vrt::LensSel &lsel, const AccumStep &acc, hipStream_t s) {
    namespace launch = vrt::launch;
    vrt::accum::MomArgs q{};
    q.hsum = ac.d_hsum;
    q.hframe = ac.d_hframe;
    q.msum = ac.d_msum;
    const bool hdr = acc.hdr, adaptive = acc.adaptive;
    const launch::AccumForm form = launch::accum_form(hdr, acc.moments);
    // the kernels of VRT_MODE_FULL by the step's own snapshot (acc.paths: what the add that queued it read), not the context
    launch::PathFamily fam;
    launch::PathArgs pa;
    if (!launch::select_paths(mode, acc.paths, a.light_dir, two_pass, fam, pa)) return hipErrorInvalidValue;
    const vrt::accum::HdrFrame hf{ac.d_pass1, ac.d_id, ac.d_hframe};
    q.sums = ac.d_sums;
    q.pass1_rgba = ac.d_pass1;
    q.out_id = ac.d_id;
    q.first = acc.first;
    q.n = acc.n;
    if (adaptive) {
        q.sq = ac.d_sq; q.tiles = ac.d_tiles; q.n_tiles = ac.d_tiles + ac.tile_cap;
        q.min = ac.min_samples; q.max = ac.max_samples; q.tol = ac.tolerance;
    }
    using vrt::accum::Source;
    const Source src = acc.aperture > 0.0f ? Source::kLens : (acc.jitter ? Source::kJitter : Source::kCorner);
    const vrt::accum::Lens l{acc.aperture, acc.focus, acc.jitter ? 1u : 0u, lsel.eye_shared ? 0u : 1u};
    if (src != Source::kCorner) {   // every sample has a ray of its own: no per-projection tables
        vs.v[0].gen_x = vs.v[0].gen_y = nullptr;
        vs.v[0].gen_z = 0.0f;
        vs.v[0].gen_fast = 0u;
    }
    if (acc.guides)   // vrt_accum_guides: the samples' first hits into the guide state, none of the sums touched
        return launch::accum_guides(src, v, a, vs,
                                    vrt::guides::Args{acc.guide_state ? vrt::guides::state_of(acc.guide_state, (size_t)a.width * (size_t)a.height)
                                                                      : vrt::guides::state_of(ac.d_guides.get(), (size_t)ac.width * (size_t)ac.height),
                                                      acc.first, acc.n},
                                    l, acc.glass, grid, s);
    if (acc.frame_only)   // an HDR accumulation's corner frame of a primary mode, every sample of the repeat path
        return (hdr && mode != VRT_MODE_FULL && src == Source::kCorner) ? launch::accum_frame_hdr(mode, v, a, vs, hf, grid, s) : hipErrorInvalidValue;
    if (mode != VRT_MODE_FULL)   // one launch, the samples looped in the lanes
        return launch::accum_primary(hdr, acc.moments, mode, src, v, a, vs, q, adaptive, l, grid, s);
    if (two_pass && src != Source::kCorner)   // MODE 6's chain per sample, looped in the lanes
        return launch::accum_opaque(form, fam, pa, src, a, vs, q, adaptive, l, grid, s);
    hipError_t e = hipSuccess;
    if (two_pass) {   // pass 1 once per accumulation, then one launch of the sample-looped bounce
        a.defer_rec = reinterpret_cast<float *>(ac.d_seed.get());
        if (!ac.pass1) {
            vs.v[0].out_rgba = ac.d_pass1;
            vs.v[0].out_id = ac.d_id;
            // (HDR: the same pass with its float colour, for the pixels without a bounce)
            e = hdr ? launch::accum_pass1_hdr(a, vs, hf, grid, s) : launch::trace_full_pass1(a, vs, grid, s);
            if (e != hipSuccess) return e;
            ac.pass1 = true;
        }
        return launch::accum_bounce(form, fam, pa, a, vs, q, adaptive, grid, s);
    }
    // the general path tracer, one launch per sample; an adaptive round first lists the tiles with an active pixel
    const vrt::accum::Tiles tl{ac.d_sums, ac.d_sq, ac.d_tiles, ac.d_tiles + ac.tile_cap, a.width, a.height, ac.min_samples, ac.max_samples,
                               ac.tolerance};
    for (uint32_t k = 0; k < acc.n && e == hipSuccess; ++k) {
        q.first = acc.first + k;
        q.n = 1u;
        if (adaptive) e = launch::adaptive_tiles(tl, s);
        if (e == hipSuccess) e = launch::accum_full(form, fam, pa, src, v, a, vs, q, adaptive, l, grid, s);
    }
    return e;
}

extern "C" {

int vrt_accum_begin(vrt_ctx *c, int width, int height, uint32_t first_sample) {
    return vrt_accum_begin_ex(c, width, height, VRT_MODE_FULL, first_sample, 0u);
}

int vrt_accum_begin_ex(vrt_ctx *c, int width, int height, int mode, uint32_t first_sample, uint32_t flags) {
    return begin(c, width, height, mode, first_sample, flags, nullptr);
}

int vrt_accum_begin_adaptive(vrt_ctx *c, int width, int height, int mode, uint32_t first_sample, uint32_t flags,
                             uint32_t min_samples, uint32_t max_samples, uint32_t tolerance) {
    if (!c) return VRT_E_INVALID;
    if (min_samples < 2u || min_samples > max_samples || max_samples > vrt::accum::kMaxSamples)
        return vrt_fail(c, VRT_E_INVALID, "vrt_accum_begin_adaptive: need 2 <= min_samples <= max_samples <= 2^24");
    if (tolerance > 65535u) return vrt_fail(c, VRT_E_INVALID, "vrt_accum_begin_adaptive: tolerance must be at most 65535");
    const uint32_t rule[3] = {min_samples, max_samples, tolerance};
    return begin(c, width, height, mode, first_sample, flags, rule);
}

int vrt_accum_add(vrt_ctx *c, uint32_t n_samples, uint32_t *total_out) {
    if (!c) return VRT_E_INVALID;
    Accum &ac = c->accum;
    if (!ac.begun) return vrt_fail(c, VRT_E_STATE, "vrt_accum_add: no accumulation (call vrt_accum_begin first)");
    if (c->batch.open) return vrt_fail(c, VRT_E_STATE, "vrt_accum_add: a patch batch is open (call vrt_patch_end first)");
    if (!c->have_scene) return vrt_fail(c, VRT_E_STATE, "vrt_accum_add: no octree uploaded (call vrt_upload_octree first)");
    if (!c->have_camera) return vrt_fail(c, VRT_E_STATE, "vrt_accum_add: no camera set (call vrt_set_camera first)");
    if (n_samples == 0) return vrt_fail(c, VRT_E_INVALID, "vrt_accum_add: n_samples must be at least 1");
    // the restart rule: anything a sample depends on changed since the first sample in the sums -> the sums start again at `first`
    // emitter sampling (vrt_set_emitter_sampling): the list of the current tree, before anything is queued
    const bool sampling = ac.mode == VRT_MODE_FULL && c->emitter_sampling;
    if (sampling) {
        const int re = ensure_emitters(c, "vrt_accum_add", true);
        if (re) return re;
        ac.emit_list = c->emitters.d_list;
        ac.emit_n = (uint32_t)c->emitters.n;
        ac.emit_cdf = c->emitters.d_cdf;
        ac.emit_inv_power = emitter_inv_power(c->emitters.wtot);
    }
    const bool restart = ac.total == 0 || !same_inputs(c, ac);
    const uint32_t base = restart ? 0u : ac.total;
    if (n_samples > vrt::accum::kMaxSamples - base)   // an adaptive accumulation: rounds
        return vrt_fail(c, VRT_E_INVALID, "vrt_accum_add: at most 2^24 samples per accumulation");
    VRT_HIP(c, hipSetDevice(c->device));
    if (restart) {
        VRT_HIP(c, hipMemsetAsync(ac.d_sums, 0, (size_t)ac.width * (size_t)ac.height * 16, c->stream));
        if (ac.adaptive) VRT_HIP(c, hipMemsetAsync(ac.d_sq, 0, (size_t)ac.width * (size_t)ac.height * 8, c->stream));
        if (ac.hdr) VRT_HIP(c, hipMemsetAsync(ac.d_hsum, 0, (size_t)ac.width * (size_t)ac.height * 24, c->stream));   // +0.0
        if (ac.moments) VRT_HIP(c, hipMemsetAsync(ac.d_msum, 0, (size_t)ac.width * (size_t)ac.height * 16, c->stream));
        take_inputs(c, ac);
        ++ac.epoch;
        ac.total = 0;
        ac.pass1 = false;
        ac.frame = false;
    }
    const bool jitter = (ac.flags & VRT_ACCUM_JITTER) != 0u;
    const bool lens = ac.lens[0] != 0.0f;   // a thin lens (vrt_set_lens): every sample has an origin of its own
    int r = VRT_OK;
    if ((jitter || lens || ac.mode != VRT_MODE_FULL) && !ac.frame) {   // the mode's unjittered frame, once per accumulation
        if (ac.hdr && !jitter && !lens) {   // every sample is that frame: its float colour too, from the HDR frame kernel
            AccumStep fr{ac.first, 0u, false};
            fr.hdr = fr.frame_only = true;
            r = enqueue(c, ac.width, ac.height, 0, ac.height, ac.height, 0, 0, ac.mode, ac.d_pass1, ac.d_id, c->stream, nullptr, 1, &fr);
        } else {
            // a frame launch of the accumulation's own: like every other launch of vrt_accum_add it takes no profiling slot and
            // does not count towards the stride (include/vrt.h vrt_set_profiling)
            const bool profiling = c->profiling;
            c->profiling = false;
            r = enqueue(c, ac.width, ac.height, 0, ac.height, ac.height, 0, 0, ac.mode, ac.d_pass1, ac.d_id, c->stream);
            c->profiling = profiling;
        }
        ac.frame = r == VRT_OK;
    }
    if (r == VRT_OK && !jitter && !lens && ac.mode != VRT_MODE_FULL) {   // every sample is that frame
        const vrt::accum::Repeat q{ac.d_pass1, ac.d_sums, n_samples, (uint32_t)((size_t)ac.width * (size_t)ac.height)};
        hipError_t e;
        if (ac.adaptive) {   // each pixel's count goes to min(rounds, min_samples): no trace
            vrt::accum::RepeatMomOf<vrt::accum::RepeatAdapt> qa{};
            static_cast<vrt::accum::Repeat &>(qa) = q;
            qa.sq = ac.d_sq;
            qa.min = ac.min_samples;
            qa.hsum = ac.d_hsum;
            qa.hframe = ac.d_hframe;
            qa.msum = ac.d_msum;
            e = ac.moments ? vrt::launch::accum_repeat_mom(qa, c->stream)
                           : (ac.hdr ? vrt::launch::accum_repeat_hdr(qa, c->stream) : vrt::launch::accum_repeat(qa, c->stream));
        } else if (ac.hdr) {
            vrt::accum::RepeatMomOf<vrt::accum::Repeat> qh{};
            static_cast<vrt::accum::Repeat &>(qh) = q;
            qh.hsum = ac.d_hsum;
            qh.hframe = ac.d_hframe;
            qh.msum = ac.d_msum;
            e = ac.moments ? vrt::launch::accum_repeat_mom(qh, c->stream) : vrt::launch::accum_repeat_hdr(qh, c->stream);
        } else {
            e = vrt::launch::accum_repeat(q, c->stream);
        }
        if (e != hipSuccess) r = vrt_fail(c, VRT_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    } else if (r == VRT_OK) {
        AccumStep step{ac.first + base, n_samples, jitter, ac.lens[0], ac.lens[1], ac.adaptive, ac.hdr};
        step.moments = ac.moments;
        // the snapshot launch_accum_step() selects the kernels by: the depth and the sun as the sums took them, the emitter switches
        // (same_inputs() has found them unchanged) and the list as this add found it
        step.paths = PathSetup{ac.path_depth, ac.sun_disc, sampling, c->emitter_importance, c->emitter_mis,
                               ac.emit_list, ac.emit_n, ac.emit_cdf, ac.emit_inv_power};
        r = enqueue(c, ac.width, ac.height, 0, ac.height, ac.height, 0, 0, ac.mode, ac.d_pass1, ac.d_id, c->stream, nullptr, 1, &step);
    }
    if (r) {   // what this add left in the sums is unknown: the next add starts again
        ac.total = 0;
        return r;
    }
    ac.total = base + n_samples;
    if (total_out) *total_out = ac.total;
    return VRT_OK;
}

int vrt_accum_resolve(vrt_ctx *c, uint8_t *out_rgba8, int32_t *out_id_dist, uint8_t *out_shown_rgba8) {
    int r = accum_state(c, "vrt_accum_resolve", false);
    if (r) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    r = ensure_scratch(c, px);
    if (r) return r;
    const bool want_rgba = out_rgba8 || out_shown_rgba8;
    r = resolve_into(c, want_rgba ? c->d_rgba : nullptr, nullptr, out_shown_rgba8 ? c->d_shown : nullptr, c->stream);
    if (r) return r;
    vrt_stage::Stage st(4);
    st.out(px * 4, out_rgba8, c->d_rgba);
    st.out(px * 8, out_id_dist, ac.d_id);
    st.out(px * 4, out_shown_rgba8, c->d_shown);
    return st.download(c, c->stream);
}

int vrt_accum_resolve_device(vrt_ctx *c, void *d_rgba8, void *d_id_dist, void *d_shown_rgba8, void *stream) {
    int r = accum_state(c, "vrt_accum_resolve_device", false);
    if (r) return r;
    if (d_shown_rgba8 && !d_rgba8) return vrt_fail(c, VRT_E_INVALID, "vrt_accum_resolve_device: the display pass needs d_rgba8");
    VRT_HIP(c, hipSetDevice(c->device));
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return accum_joined(c, s, [&] { return resolve_into(c, d_rgba8, d_id_dist, d_shown_rgba8, s); });
}

int vrt_accum_keep_hdr(vrt_ctx *c, int enable) {
    if (!c) return VRT_E_INVALID;
    if (enable != 0 && enable != 1) return vrt_fail(c, VRT_E_INVALID, "vrt_accum_keep_hdr: enable must be 0 or 1");
    c->accum_keep_hdr = enable == 1;
    return VRT_OK;
}

int vrt_accum_keep_moments(vrt_ctx *c, int enable) {
    if (!c) return VRT_E_INVALID;
    if (enable != 0 && enable != 1) return vrt_fail(c, VRT_E_INVALID, "vrt_accum_keep_moments: enable must be 0 or 1");
    c->accum_keep_moments = enable == 1;
    return VRT_OK;
}

int vrt_accum_variance(vrt_ctx *c, float *out_variance) {
    int r = variance_state(c, "vrt_accum_variance", out_variance);
    if (r) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    Accum &ac = c->accum;
    if ((r = ensure_variance_plane(c)) || (r = accum_variance_into(c, ac.d_mvar, c->stream))) return r;
    vrt_stage::Stage st(4);
    st.out((size_t)ac.width * (size_t)ac.height * 4, out_variance, ac.d_mvar);
    return st.download(c, c->stream);
}

int vrt_accum_variance_device(vrt_ctx *c, void *d_variance, void *stream) {
    const int r = variance_state(c, "vrt_accum_variance_device", d_variance);
    if (r) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return accum_joined(c, s, [&] { return accum_variance_into(c, static_cast<float *>(d_variance), s); });
}

int vrt_accum_resolve_hdr(vrt_ctx *c, float *out_rgb, const vrt_tonemap *tm, uint8_t *out_rgba8, uint8_t *out_shown_rgba8) {
    int r = resolve_hdr_state(c, "vrt_accum_resolve_hdr", tm);
    if (r) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    r = ensure_scratch(c, px);
    if (r) return r;
    if (out_rgb && (r = ensure_float_image(c, ac.d_hrgb, px))) return r;
    const bool want_rgba = out_rgba8 || out_shown_rgba8;
    r = resolve_hdr_into(c, out_rgb ? ac.d_hrgb : nullptr, tm, want_rgba ? c->d_rgba : nullptr, out_shown_rgba8 ? c->d_shown : nullptr, c->stream);
    if (r) return r;
    vrt_stage::Stage st(4);
    st.out(px * 12, out_rgb, ac.d_hrgb);
    st.out(px * 4, out_rgba8, c->d_rgba);
    st.out(px * 4, out_shown_rgba8, c->d_shown);
    return st.download(c, c->stream);
}

int vrt_accum_resolve_hdr_device(vrt_ctx *c, void *d_rgb, const vrt_tonemap *tm, void *d_rgba8, void *d_shown_rgba8, void *stream) {
    int r = resolve_hdr_state(c, "vrt_accum_resolve_hdr_device", tm);
    if (r) return r;
    if (d_shown_rgba8 && !d_rgba8) return vrt_fail(c, VRT_E_INVALID, "vrt_accum_resolve_hdr_device: the display pass needs d_rgba8");
    VRT_HIP(c, hipSetDevice(c->device));
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return accum_joined(c, s, [&] { return resolve_hdr_into(c, static_cast<float *>(d_rgb), tm, d_rgba8, d_shown_rgba8, s); });
}

int vrt_accum_resolve_hdr_shown(vrt_ctx *c, const vrt_tonemap *tm, float *out_shown_rgb, uint8_t *out_shown_rgba8) {
    int r = resolve_hdr_state(c, "vrt_accum_resolve_hdr_shown", tm);
    if (r) return r;
    if (!out_shown_rgb && !out_shown_rgba8) return vrt_fail(c, VRT_E_INVALID, "vrt_accum_resolve_hdr_shown: both outputs null");
    VRT_HIP(c, hipSetDevice(c->device));
    Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    if ((r = ensure_scratch(c, px)) || (r = ensure_float_image(c, ac.d_hmean, px))) return r;
    if (out_shown_rgb && (r = ensure_float_image(c, ac.d_hrgb, px))) return r;
    r = resolve_hdr_shown_into(c, tm, out_shown_rgb ? ac.d_hrgb : nullptr, out_shown_rgba8 ? c->d_shown : nullptr, c->stream);
    if (r) return r;
    vrt_stage::Stage st(4);
    st.out(px * 12, out_shown_rgb, ac.d_hrgb);
    st.out(px * 4, out_shown_rgba8, c->d_shown);
    return st.download(c, c->stream);
}

int vrt_accum_resolve_hdr_shown_device(vrt_ctx *c, const vrt_tonemap *tm, void *d_shown_rgb, void *d_shown_rgba8, void *stream) {
    int r = resolve_hdr_state(c, "vrt_accum_resolve_hdr_shown_device", tm);
    if (r) return r;
    if (!d_shown_rgb && !d_shown_rgba8) return vrt_fail(c, VRT_E_INVALID, "vrt_accum_resolve_hdr_shown_device: both outputs null");
    VRT_HIP(c, hipSetDevice(c->device));
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    Accum &ac = c->accum;
    if ((r = ensure_float_image(c, ac.d_hmean, (size_t)ac.width * (size_t)ac.height))) return r;
    return accum_joined(c, s, [&] { return resolve_hdr_shown_into(c, tm, d_shown_rgb, d_shown_rgba8, s); });
}

int vrt_accum_counts(vrt_ctx *c, uint32_t *out_counts) {
    if (!c) return VRT_E_INVALID;
    Accum &ac = c->accum;
    if (!ac.begun) return vrt_fail(c, VRT_E_STATE, "vrt_accum_counts: no accumulation (call vrt_accum_begin_adaptive first)");
    if (!ac.adaptive) return vrt_fail(c, VRT_E_STATE, "vrt_accum_counts: the accumulation is not adaptive");
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    if (ac.total == 0) {   // no round yet: every pixel active with zero samples
        if (out_counts) std::memset(out_counts, 0, px * 4);
        return (int)px;
    }
    VRT_HIP(c, hipSetDevice(c->device));
    int r = ensure_scratch(c, px);
    if (r) return r;
    uint32_t *d_active = ac.d_tiles + ac.tile_cap + 1;
    const vrt::accum::Counts q{ac.d_sums, ac.d_sq, static_cast<uint32_t *>(c->d_rgba.get()), d_active, (uint32_t)px, ac.min_samples,
                               ac.max_samples, ac.tolerance};
    VRT_HIP(c, vrt::launch::adaptive_counts(q, c->stream));
    uint32_t active = 0;
    vrt_stage::Stage st(4);
    st.out(px * 4, out_counts, c->d_rgba);
    st.out(4, &active, d_active);
    return (r = st.download(c, c->stream)) ? r : (int)active;
}

}  // extern "C"
