// vrt_filter.cpp -- the guided filter (include/vrt.h vrt_filter_hdr and its host and accumulation forms): validation, the context's
// scratch, the prepass and the level loop, and the route from an HDR accumulation -- its float mean (vrt_accum_resolve_hdr_device)
// and its own guide planes (vrt_accum_guides_device, which brings the guide state up to date) into the accumulation's scratch, then
// the stateless filter on them. The variance-guided forms (vrt_filter_hdr_var and its host and accumulation forms) follow the same
// routes with the same scratch: the prepass, then the variance kernel, then their own level kernels. Host code; the kernels are
// behind vrt_launch.h. Nothing here touches the accumulation's sums.
#include "vrt_internal.h"
#include "vrt_launch.h"

#include <cmath>

using namespace vrt_internal;

namespace {

// Mean or caller's image, the four planes, the float output and the bytes: 3 + 3 + 4 + 1 + 1 + 3 + 1 words per pixel, the layout
// of both staging blocks (the context's for vrt_filter_hdr_host, the accumulation's for its filtered resolve)
constexpr size_t kStageBytes = 64;
// ... and, for the variance-guided forms, the variance plane in and out behind them: 2 more words
constexpr size_t kStageVarBytes = 72;
struct Stage {
    float *rgb, *normal, *albedo, *depth, *coverage, *out_rgb;
    uint32_t *out_rgba;
    float *variance, *out_variance;   // inside the block only where it was sized with kStageVarBytes
};
Stage stage_of(float *base, size_t px) {
    return Stage{base, base + px * 3, base + px * 6, base + px * 10, base + px * 11, base + px * 12, reinterpret_cast<uint32_t *>(base + px * 15),
                 base + px * 16, base + px * 17};
}

struct Checked {
    vrt_filter f;
    float kn, ka;
};

// the filter a call runs with (NULL: the defaults), or VRT_E_INVALID in the name of `what`; needs no device
int check_filter(vrt_ctx *c, const char *what, const vrt_filter *f, Checked &out) {
    if (f) out.f = *f;
    else vrt_filter_default(&out.f);
    const vrt_filter &g = out.f;
    if (g.levels < 0 || g.levels > VRT_FILTER_MAX_LEVELS)
        return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": levels must be in 0..VRT_FILTER_MAX_LEVELS");
    if (g.flags & ~(uint32_t)VRT_FILTER_DEMODULATE) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": unknown flags");
    for (const float sg : {g.sigma_normal, g.sigma_albedo, g.sigma_depth})
        if (!(sg > 0.0f) || !(sg <= 3.402823466e38f)) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": every sigma must be finite and > 0");
    out.kn = 1.0f / (g.sigma_normal * g.sigma_normal);
    out.ka = 1.0f / (g.sigma_albedo * g.sigma_albedo);
    if (!(out.kn <= 3.402823466e38f) || !(out.ka <= 3.402823466e38f))   // sigma * sigma went to 0: 0 * kn at the centre tap would be NaN
        return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": sigma_normal or sigma_albedo too small (1 / sigma^2 is not finite)");
    return VRT_OK;
}

struct CheckedVar {
    vrt_filter_var f;
    Checked k;
};

// the same for a vrt_filter_var (NULL: vrt_filter_var_default)
int check_filter_var(vrt_ctx *c, const char *what, const vrt_filter_var *f, CheckedVar &out) {
    if (f) out.f = *f;
    else vrt_filter_var_default(&out.f);
    const vrt_filter_var &g = out.f;
    const vrt_filter guide{g.levels, g.flags, g.sigma_normal, g.sigma_albedo, g.sigma_depth};
    const int r = check_filter(c, what, &guide, out.k);
    if (r) return r;
    if (!(g.sigma_lum > 0.0f) || !(g.sigma_lum <= 3.402823466e38f)) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": every sigma must be finite and > 0");
    return VRT_OK;
}

// room in the context's scratch for a frame of px pixels at `levels`. The blocks may still be in use by an earlier call on any
// stream, so growth waits for the device.
int ensure_level_scratch(vrt_ctx *c, size_t px, int levels) {
    vrt_ctx::FilterScratch &fs = c->filter;
    const size_t pack = levels >= 1 ? px * vrt::filter::kPackBytes : 0, ping = levels >= 2 ? px * vrt::filter::kImageBytes : 0,
                 pong = levels >= 3 ? px * vrt::filter::kImageBytes : 0;
    if (!fs.done) VRT_HIP(c, hipEventCreateWithFlags(&fs.done, hipEventDisableTiming));
    if (pack <= fs.d_pack.bytes() && ping <= fs.d_ping.bytes() && pong <= fs.d_pong.bytes()) return VRT_OK;
    VRT_HIP(c, hipDeviceSynchronize());
    VRT_HIP(c, fs.d_pack.reserve(pack));
    VRT_HIP(c, fs.d_ping.reserve(ping));
    VRT_HIP(c, fs.d_pong.reserve(pong));
    return VRT_OK;
}

int ensure_stage(vrt_ctx *c, DevBuf<float> &buf, size_t px, size_t bytes_per_pixel = kStageBytes) {
    return px * bytes_per_pixel <= buf.bytes() ? VRT_OK : reserve_synced(c, {{&buf, px * bytes_per_pixel}});
}

int check_outputs(vrt_ctx *c, const char *what, const void *out_rgb, const void *out_rgba8) {
    if (!out_rgb && !out_rgba8) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": both outputs null");
    return VRT_OK;
}

// the call-order checks of the accumulation forms: those of vrt_accum_guides, then vrt_accum_resolve_hdr's
int filtered_state(vrt_ctx *c, const char *what) {
    if (!c->accum.begun) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": no accumulation (call vrt_accum_begin first)");
    if (c->accum.total == 0) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": the accumulation holds no samples (call vrt_accum_add first)");
    if (!c->accum.hdr) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": the accumulation keeps no HDR sums (vrt_accum_keep_hdr before the begin)");
    return VRT_OK;
}

// mean and planes into the accumulation's stage and the filter on them, all on stream s; d_rgb / d_rgba: where the outputs go
int filtered_into(vrt_ctx *c, const vrt_filter *f, const vrt_tonemap *tm, const Stage &st, void *d_rgb, void *d_rgba, hipStream_t s) {
    vrt_ctx::Accum &ac = c->accum;
    int r = vrt_accum_guides_device(c, st.normal, st.albedo, st.depth, st.coverage, s);   // brings the guide state up to date first
    if (r) return r;
    if ((r = vrt_accum_resolve_hdr_device(c, st.rgb, tm, nullptr, nullptr, s))) return r;
    // the stage belongs to the accumulation, whose every use the context's stream orders: a caller's stream is joined back
    return accum_joined(c, s, [&] {
        return vrt_filter_hdr(c, ac.width, ac.height, st.rgb, st.normal, st.albedo, st.depth, st.coverage, f, tm, d_rgb, d_rgba, s);
    });
}

// the same for the variance-guided filter; the accumulation has no variance of its own: the spatial estimate
int filtered_into_var(vrt_ctx *c, const vrt_filter_var *f, const vrt_tonemap *tm, const Stage &st, void *d_rgb, void *d_rgba, void *d_variance,
                      hipStream_t s) {
    vrt_ctx::Accum &ac = c->accum;
    int r = vrt_accum_guides_device(c, st.normal, st.albedo, st.depth, st.coverage, s);
    if (r) return r;
    if ((r = vrt_accum_resolve_hdr_device(c, st.rgb, tm, nullptr, nullptr, s))) return r;
    return accum_joined(c, s, [&] {
        return vrt_filter_hdr_var(c, ac.width, ac.height, st.rgb, st.normal, st.albedo, st.depth, st.coverage, nullptr, f, tm, d_rgb, d_rgba,
                                  d_variance, s);
    });
}

}  // namespace

extern "C" {

void vrt_filter_default(vrt_filter *f) {
    if (!f) return;
    f->levels = 1;
    f->flags = VRT_FILTER_DEMODULATE;
    f->sigma_normal = 1.0f;
    f->sigma_albedo = 0.05f;
    f->sigma_depth = 2.0f;
}

int vrt_filter_hdr(vrt_ctx *c, int width, int height, const void *d_rgb, const void *d_normal, const void *d_albedo, const void *d_depth,
                   const void *d_coverage, const vrt_filter *f, const vrt_tonemap *tm, void *d_out_rgb, void *d_out_rgba8, void *stream) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (!d_rgb || !d_normal || !d_albedo || !d_depth || !d_coverage) return vrt_fail(c, VRT_E_INVALID, "vrt_filter_hdr: null input");
    if ((r = check_outputs(c, "vrt_filter_hdr", d_out_rgb, d_out_rgba8))) return r;
    if (d_out_rgb && (d_out_rgb == d_rgb || d_out_rgb == d_normal || d_out_rgb == d_albedo || d_out_rgb == d_depth || d_out_rgb == d_coverage))
        return vrt_fail(c, VRT_E_INVALID, "vrt_filter_hdr: d_out_rgb must not alias an input");
    Checked k;
    if ((r = check_filter(c, "vrt_filter_hdr", f, k))) return r;
    if ((r = check_tonemap(c, "vrt_filter_hdr", tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    const int levels = k.f.levels;
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const uint32_t demod = (k.f.flags & VRT_FILTER_DEMODULATE) ? 1u : 0u;
    const int op = tm ? tm->op : VRT_TONEMAP_CLAMP;
    const float exposure = tm ? tm->exposure : 1.0f;
    const vrt::filter::Guides g{static_cast<const float *>(d_normal), static_cast<const float *>(d_albedo), static_cast<const float *>(d_depth),
                                static_cast<const float *>(d_coverage)};
    if (levels == 0) {
        const vrt::filter::Through q{static_cast<const float *>(d_rgb), g, static_cast<float *>(d_out_rgb), static_cast<uint32_t *>(d_out_rgba8),
                                     (uint32_t)px, demod, op, exposure};
        VRT_HIP(c, vrt::launch::filter_through(q, s));
        return VRT_OK;
    }
    if ((r = ensure_level_scratch(c, px, levels))) return r;
    vrt_ctx::FilterScratch &fs = c->filter;
    if (fs.used && fs.last != s) VRT_HIP(c, hipStreamWaitEvent(s, fs.done, 0));   // the scratch is still the last call's
    VRT_HIP(c, vrt::launch::filter_prepass(vrt::filter::Prepass{g, fs.d_pack, width, height}, s));
    vrt::filter::Level q{};
    q.rgb = static_cast<const float *>(d_rgb);
    q.pack = fs.d_pack;
    q.width = width;
    q.height = height;
    q.kn = k.kn;
    q.ka = k.ka;
    q.sigma_depth = k.f.sigma_depth;
    q.demodulate = demod;
    q.op = op;
    q.exposure = exposure;
    for (int i = 0; i < levels; ++i) {
        const bool first = i == 0, last = i == levels - 1;
        q.step = 1 << i;
        q.src = first ? nullptr : ((i & 1) ? fs.d_ping.get() : fs.d_pong.get());   // level 0 writes ping, level 1 pong, ...
        q.dst = last ? nullptr : ((i & 1) ? fs.d_pong.get() : fs.d_ping.get());
        q.out_rgb = last ? static_cast<float *>(d_out_rgb) : nullptr;
        q.out_rgba = last ? static_cast<uint32_t *>(d_out_rgba8) : nullptr;
        VRT_HIP(c, vrt::launch::filter_level(q, first, last, s));
    }
    VRT_HIP(c, hipEventRecord(fs.done, s));
    fs.last = s;
    fs.used = true;
    return VRT_OK;
}

int vrt_filter_hdr_host(vrt_ctx *c, int width, int height, const float *rgb, const float *normal, const float *albedo, const float *depth,
                        const float *coverage, const vrt_filter *f, const vrt_tonemap *tm, float *out_rgb, uint8_t *out_rgba8) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (!rgb || !normal || !albedo || !depth || !coverage) return vrt_fail(c, VRT_E_INVALID, "vrt_filter_hdr_host: null input");
    if ((r = check_outputs(c, "vrt_filter_hdr_host", out_rgb, out_rgba8))) return r;
    Checked k;
    if ((r = check_filter(c, "vrt_filter_hdr_host", f, k))) return r;
    if ((r = check_tonemap(c, "vrt_filter_hdr_host", tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    if ((r = ensure_stage(c, c->filter.d_host, px))) return r;
    const Stage st = stage_of(c->filter.d_host, px);
    VRT_HIP(c, hipMemcpyAsync(st.rgb, rgb, px * 12, hipMemcpyHostToDevice, c->stream));
    VRT_HIP(c, hipMemcpyAsync(st.normal, normal, px * 12, hipMemcpyHostToDevice, c->stream));
    VRT_HIP(c, hipMemcpyAsync(st.albedo, albedo, px * 16, hipMemcpyHostToDevice, c->stream));
    VRT_HIP(c, hipMemcpyAsync(st.depth, depth, px * 4, hipMemcpyHostToDevice, c->stream));
    VRT_HIP(c, hipMemcpyAsync(st.coverage, coverage, px * 4, hipMemcpyHostToDevice, c->stream));
    r = vrt_filter_hdr(c, width, height, st.rgb, st.normal, st.albedo, st.depth, st.coverage, &k.f, tm, out_rgb ? st.out_rgb : nullptr,
                       out_rgba8 ? st.out_rgba : nullptr, nullptr);
    if (r) return r;
    if (out_rgb) VRT_HIP(c, hipMemcpyAsync(out_rgb, st.out_rgb, px * 12, hipMemcpyDeviceToHost, c->stream));
    if (out_rgba8) VRT_HIP(c, hipMemcpyAsync(out_rgba8, st.out_rgba, px * 4, hipMemcpyDeviceToHost, c->stream));
    VRT_HIP(c, hipStreamSynchronize(c->stream));
    return VRT_OK;
}

int vrt_accum_resolve_hdr_filtered(vrt_ctx *c, const vrt_filter *f, const vrt_tonemap *tm, float *out_rgb, uint8_t *out_rgba8) {
    if (!c) return VRT_E_INVALID;
    int r = filtered_state(c, "vrt_accum_resolve_hdr_filtered");
    if (r) return r;
    if ((r = check_outputs(c, "vrt_accum_resolve_hdr_filtered", out_rgb, out_rgba8))) return r;
    Checked k;
    if ((r = check_filter(c, "vrt_accum_resolve_hdr_filtered", f, k))) return r;
    if ((r = check_tonemap(c, "vrt_accum_resolve_hdr_filtered", tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt_ctx::Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    if ((r = ensure_stage(c, ac.d_filter, px))) return r;
    const Stage st = stage_of(ac.d_filter, px);
    if ((r = filtered_into(c, &k.f, tm, st, out_rgb ? st.out_rgb : nullptr, out_rgba8 ? st.out_rgba : nullptr, c->stream))) return r;
    if (out_rgb) VRT_HIP(c, hipMemcpyAsync(out_rgb, st.out_rgb, px * 12, hipMemcpyDeviceToHost, c->stream));
    if (out_rgba8) VRT_HIP(c, hipMemcpyAsync(out_rgba8, st.out_rgba, px * 4, hipMemcpyDeviceToHost, c->stream));
    VRT_HIP(c, hipStreamSynchronize(c->stream));
    return VRT_OK;
}

int vrt_accum_resolve_hdr_filtered_device(vrt_ctx *c, const vrt_filter *f, const vrt_tonemap *tm, void *d_rgb, void *d_rgba8, void *stream) {
    if (!c) return VRT_E_INVALID;
    int r = filtered_state(c, "vrt_accum_resolve_hdr_filtered_device");
    if (r) return r;
    if ((r = check_outputs(c, "vrt_accum_resolve_hdr_filtered_device", d_rgb, d_rgba8))) return r;
    Checked k;
    if ((r = check_filter(c, "vrt_accum_resolve_hdr_filtered_device", f, k))) return r;
    if ((r = check_tonemap(c, "vrt_accum_resolve_hdr_filtered_device", tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt_ctx::Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    if ((r = ensure_stage(c, ac.d_filter, px))) return r;
    return filtered_into(c, &k.f, tm, stage_of(ac.d_filter, px), d_rgb, d_rgba8, stream ? (hipStream_t)stream : c->stream);
}

// ---- the variance-guided forms (include/vrt.h vrt_filter_hdr_var, V1-V4) ----
void vrt_filter_var_default(vrt_filter_var *f) {
    if (!f) return;
    f->levels = 3;
    f->flags = VRT_FILTER_DEMODULATE;
    f->sigma_normal = 0.5f;
    f->sigma_albedo = 0.05f;
    f->sigma_depth = 2.0f;
    f->sigma_lum = 4.0f;
}

int vrt_filter_hdr_var(vrt_ctx *c, int width, int height, const void *d_rgb, const void *d_normal, const void *d_albedo, const void *d_depth,
                       const void *d_coverage, const void *d_variance, const vrt_filter_var *f, const vrt_tonemap *tm, void *d_out_rgb,
                       void *d_out_rgba8, void *d_out_variance, void *stream) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (!d_rgb || !d_normal || !d_albedo || !d_depth || !d_coverage) return vrt_fail(c, VRT_E_INVALID, "vrt_filter_hdr_var: null input");
    if ((r = check_outputs(c, "vrt_filter_hdr_var", d_out_rgb, d_out_rgba8))) return r;
    for (const void *out : {static_cast<const void *>(d_out_rgb), static_cast<const void *>(d_out_variance)})
        if (out && (out == d_rgb || out == d_normal || out == d_albedo || out == d_depth || out == d_coverage || out == d_variance))
            return vrt_fail(c, VRT_E_INVALID, "vrt_filter_hdr_var: d_out_rgb and d_out_variance must not alias an input");
    CheckedVar k;
    if ((r = check_filter_var(c, "vrt_filter_hdr_var", f, k))) return r;
    if ((r = check_tonemap(c, "vrt_filter_hdr_var", tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    const int levels = k.f.levels;
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const uint32_t demod = (k.f.flags & VRT_FILTER_DEMODULATE) ? 1u : 0u;
    const int op = tm ? tm->op : VRT_TONEMAP_CLAMP;
    const float exposure = tm ? tm->exposure : 1.0f;
    const vrt::filter::Guides g{static_cast<const float *>(d_normal), static_cast<const float *>(d_albedo), static_cast<const float *>(d_depth),
                                static_cast<const float *>(d_coverage)};
    if (levels == 0) {   // the colours are vrt_filter_hdr's (the second identity)
        const vrt::filter::Through q{static_cast<const float *>(d_rgb), g, static_cast<float *>(d_out_rgb), static_cast<uint32_t *>(d_out_rgba8),
                                     (uint32_t)px, demod, op, exposure};
        VRT_HIP(c, vrt::launch::filter_through(q, s));
        if (!d_out_variance) return VRT_OK;
    }
    if ((r = ensure_level_scratch(c, px, levels ? levels : 1))) return r;
    vrt_ctx::FilterScratch &fs = c->filter;
    if (fs.used && fs.last != s) VRT_HIP(c, hipStreamWaitEvent(s, fs.done, 0));   // the scratch is still the last call's
    VRT_HIP(c, vrt::launch::filter_prepass(vrt::filter::Prepass{g, fs.d_pack, width, height}, s));
    vrt::filter::LevelVar q{};
    q.l.rgb = static_cast<const float *>(d_rgb);
    q.l.pack = fs.d_pack;
    q.l.width = width;
    q.l.height = height;
    q.l.kn = k.k.kn;
    q.l.ka = k.k.ka;
    q.l.sigma_depth = k.f.sigma_depth;
    q.l.demodulate = demod;
    q.l.op = op;
    q.l.exposure = exposure;
    q.sigma_lum = k.f.sigma_lum;
    VRT_HIP(c, vrt::launch::filter_variance(vrt::filter::Variance{q.l, reinterpret_cast<float *>(fs.d_pack.get()), static_cast<const float *>(d_variance),
                                                                  levels == 0 ? static_cast<float *>(d_out_variance) : nullptr},
                                            s));
    for (int i = 0; i < levels; ++i) {
        const bool first = i == 0, last = i == levels - 1;
        q.l.step = 1 << i;
        q.l.src = first ? nullptr : ((i & 1) ? fs.d_ping.get() : fs.d_pong.get());   // level 0 writes ping, level 1 pong, ...
        q.l.dst = last ? nullptr : ((i & 1) ? fs.d_pong.get() : fs.d_ping.get());
        q.l.out_rgb = last ? static_cast<float *>(d_out_rgb) : nullptr;
        q.l.out_rgba = last ? static_cast<uint32_t *>(d_out_rgba8) : nullptr;
        q.out_variance = last ? static_cast<float *>(d_out_variance) : nullptr;
        VRT_HIP(c, vrt::launch::filter_var_level(q, first, last, s));
    }
    VRT_HIP(c, hipEventRecord(fs.done, s));
    fs.last = s;
    fs.used = true;
    return VRT_OK;
}

int vrt_filter_hdr_var_host(vrt_ctx *c, int width, int height, const float *rgb, const float *normal, const float *albedo, const float *depth,
                            const float *coverage, const float *variance, const vrt_filter_var *f, const vrt_tonemap *tm, float *out_rgb,
                            uint8_t *out_rgba8, float *out_variance) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (!rgb || !normal || !albedo || !depth || !coverage) return vrt_fail(c, VRT_E_INVALID, "vrt_filter_hdr_var_host: null input");
    if ((r = check_outputs(c, "vrt_filter_hdr_var_host", out_rgb, out_rgba8))) return r;
    CheckedVar k;
    if ((r = check_filter_var(c, "vrt_filter_hdr_var_host", f, k))) return r;
    if ((r = check_tonemap(c, "vrt_filter_hdr_var_host", tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    if ((r = ensure_stage(c, c->filter.d_host, px, kStageVarBytes))) return r;
    const Stage st = stage_of(c->filter.d_host, px);
    VRT_HIP(c, hipMemcpyAsync(st.rgb, rgb, px * 12, hipMemcpyHostToDevice, c->stream));
    VRT_HIP(c, hipMemcpyAsync(st.normal, normal, px * 12, hipMemcpyHostToDevice, c->stream));
    VRT_HIP(c, hipMemcpyAsync(st.albedo, albedo, px * 16, hipMemcpyHostToDevice, c->stream));
    VRT_HIP(c, hipMemcpyAsync(st.depth, depth, px * 4, hipMemcpyHostToDevice, c->stream));
    VRT_HIP(c, hipMemcpyAsync(st.coverage, coverage, px * 4, hipMemcpyHostToDevice, c->stream));
    if (variance) VRT_HIP(c, hipMemcpyAsync(st.variance, variance, px * 4, hipMemcpyHostToDevice, c->stream));
    r = vrt_filter_hdr_var(c, width, height, st.rgb, st.normal, st.albedo, st.depth, st.coverage, variance ? st.variance : nullptr, &k.f, tm,
                           out_rgb ? st.out_rgb : nullptr, out_rgba8 ? st.out_rgba : nullptr, out_variance ? st.out_variance : nullptr, nullptr);
    if (r) return r;
    if (out_rgb) VRT_HIP(c, hipMemcpyAsync(out_rgb, st.out_rgb, px * 12, hipMemcpyDeviceToHost, c->stream));
    if (out_rgba8) VRT_HIP(c, hipMemcpyAsync(out_rgba8, st.out_rgba, px * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_variance) VRT_HIP(c, hipMemcpyAsync(out_variance, st.out_variance, px * 4, hipMemcpyDeviceToHost, c->stream));
    VRT_HIP(c, hipStreamSynchronize(c->stream));
    return VRT_OK;
}

int vrt_accum_resolve_hdr_filtered_var(vrt_ctx *c, const vrt_filter_var *f, const vrt_tonemap *tm, float *out_rgb, uint8_t *out_rgba8,
                                       float *out_variance) {
    if (!c) return VRT_E_INVALID;
    int r = filtered_state(c, "vrt_accum_resolve_hdr_filtered_var");
    if (r) return r;
    if ((r = check_outputs(c, "vrt_accum_resolve_hdr_filtered_var", out_rgb, out_rgba8))) return r;
    CheckedVar k;
    if ((r = check_filter_var(c, "vrt_accum_resolve_hdr_filtered_var", f, k))) return r;
    if ((r = check_tonemap(c, "vrt_accum_resolve_hdr_filtered_var", tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt_ctx::Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    if ((r = ensure_stage(c, ac.d_filter, px, kStageVarBytes))) return r;
    const Stage st = stage_of(ac.d_filter, px);
    if ((r = filtered_into_var(c, &k.f, tm, st, out_rgb ? st.out_rgb : nullptr, out_rgba8 ? st.out_rgba : nullptr,
                               out_variance ? st.out_variance : nullptr, c->stream)))
        return r;
    if (out_rgb) VRT_HIP(c, hipMemcpyAsync(out_rgb, st.out_rgb, px * 12, hipMemcpyDeviceToHost, c->stream));
    if (out_rgba8) VRT_HIP(c, hipMemcpyAsync(out_rgba8, st.out_rgba, px * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_variance) VRT_HIP(c, hipMemcpyAsync(out_variance, st.out_variance, px * 4, hipMemcpyDeviceToHost, c->stream));
    VRT_HIP(c, hipStreamSynchronize(c->stream));
    return VRT_OK;
}

int vrt_accum_resolve_hdr_filtered_var_device(vrt_ctx *c, const vrt_filter_var *f, const vrt_tonemap *tm, void *d_rgb, void *d_rgba8,
                                              void *d_variance_out, void *stream) {
    if (!c) return VRT_E_INVALID;
    int r = filtered_state(c, "vrt_accum_resolve_hdr_filtered_var_device");
    if (r) return r;
    if ((r = check_outputs(c, "vrt_accum_resolve_hdr_filtered_var_device", d_rgb, d_rgba8))) return r;
    CheckedVar k;
    if ((r = check_filter_var(c, "vrt_accum_resolve_hdr_filtered_var_device", f, k))) return r;
    if ((r = check_tonemap(c, "vrt_accum_resolve_hdr_filtered_var_device", tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt_ctx::Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    if ((r = ensure_stage(c, ac.d_filter, px, kStageVarBytes))) return r;
    return filtered_into_var(c, &k.f, tm, stage_of(ac.d_filter, px), d_rgb, d_rgba8, d_variance_out, stream ? (hipStream_t)stream : c->stream);
}

}  // extern "C"
