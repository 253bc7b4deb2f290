// vrt_filter.cpp -- the guided filter and its variance-guided form (include/vrt.h vrt_filter_hdr, vrt_filter_hdr_var and their host
// and accumulation forms). One route serves both (filter_frame): validation, the context's scratch, the prepass, the variance kernel
// of the variance-guided form, the level loop. One helper stages host planes around it (filter_host), one brings an HDR
// accumulation's float mean (vrt_accum_resolve_hdr_device) and its own guide planes (vrt_accum_guides_device, which brings the guide
// state up to date) into the accumulation's scratch and runs it on them (filter_accum). The entry points are thin callers: the
// guide-only ones pass no variance input, no variance output and no luminance width. Host code; the kernels are behind
// vrt_launch.h. Nothing here touches the accumulation's sums.
#include "vrt_stage.h"
#include "vrt_launch.h"

#include <cmath>

using namespace vrt_internal;

namespace {

// The filter a call runs with, in one shape for both forms: the guide-only one has no sigma_lum (var false). kn, ka: check_filter's.
struct Params {
    vrt_filter_var f;
    bool var;
    float kn, ka;
};
Params params_of(const vrt_filter *f) {   // NULL: vrt_filter_default
    vrt_filter d;
    vrt_filter_default(&d);
    if (f) d = *f;
    return Params{{d.levels, d.flags, d.sigma_normal, d.sigma_albedo, d.sigma_depth, 0.0f}, false, 0.0f, 0.0f};
}
Params params_of(const vrt_filter_var *f) {   // NULL: vrt_filter_var_default
    Params k{{}, true, 0.0f, 0.0f};
    if (f) k.f = *f;
    else vrt_filter_var_default(&k.f);
    return k;
}

// VRT_E_INVALID in the name of `what` unless the call's filter is one the header allows; fills kn and ka. Needs no device.
int check_filter(vrt_ctx *c, const char *what, Params &k) {
    const vrt_filter_var &g = k.f;
    if (g.levels < 0 || g.levels > VRT_FILTER_MAX_LEVELS)
        return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": levels must be in 0..VRT_FILTER_MAX_LEVELS");
    if (g.flags & ~(uint32_t)VRT_FILTER_DEMODULATE) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": unknown flags");
    for (const float sg : {g.sigma_normal, g.sigma_albedo, g.sigma_depth})
        if (!(sg > 0.0f) || !(sg <= 3.402823466e38f)) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": every sigma must be finite and > 0");
    k.kn = 1.0f / (g.sigma_normal * g.sigma_normal);
    k.ka = 1.0f / (g.sigma_albedo * g.sigma_albedo);
    if (!(k.kn <= 3.402823466e38f) || !(k.ka <= 3.402823466e38f))   // sigma * sigma went to 0: 0 * kn at the centre tap would be NaN
        return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": sigma_normal or sigma_albedo too small (1 / sigma^2 is not finite)");
    if (k.var && (!(g.sigma_lum > 0.0f) || !(g.sigma_lum <= 3.402823466e38f)))
        return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": every sigma must be finite and > 0");
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

int check_outputs(vrt_ctx *c, const char *what, const void *out_rgb, const void *out_rgba8) {
    if (!out_rgb && !out_rgba8) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": both outputs null");
    return VRT_OK;
}

// a frame's planes, in device memory or (filter_host) the caller's; variance and out_variance: the variance-guided form's, may be null
struct Planes {
    const void *rgb, *normal, *albedo, *depth, *coverage, *variance;
    void *out_rgb, *out_rgba8, *out_variance;
};

// what every form checks of its arguments before anything else, in this order; k: filled by check_filter
int check_call(vrt_ctx *c, const char *what, const Planes *io, void *out_rgb, void *out_rgba8, Params &k, const vrt_tonemap *tm, bool device) {
    if (io && (!io->rgb || !io->normal || !io->albedo || !io->depth || !io->coverage)) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null input");
    int r = check_outputs(c, what, out_rgb, out_rgba8);
    if (r) return r;
    if (io && device)
        for (const void *out : {static_cast<const void *>(io->out_rgb), static_cast<const void *>(io->out_variance)})
            if (out && (out == io->rgb || out == io->normal || out == io->albedo || out == io->depth || out == io->coverage || out == io->variance))
                return vrt_fail(c, VRT_E_INVALID,
                                std::string(what) + (k.var ? ": d_out_rgb and d_out_variance must not alias an input" : ": d_out_rgb must not alias an input"));
    if ((r = check_filter(c, what, k))) return r;
    return check_tonemap(c, what, tm);
}

// The stateless filter on device planes, stream-ordered, in the name of `what`: vrt_filter_hdr with k.var false (d.variance and
// d.out_variance null), else vrt_filter_hdr_var
int filter_frame(vrt_ctx *c, const char *what, int width, int height, const Planes &d, Params k, const vrt_tonemap *tm, void *stream) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if ((r = check_call(c, what, &d, d.out_rgb, d.out_rgba8, k, tm, true))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    const int levels = k.f.levels;
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    float *const out_rgb = static_cast<float *>(d.out_rgb), *const out_variance = static_cast<float *>(d.out_variance);
    uint32_t *const out_rgba = static_cast<uint32_t *>(d.out_rgba8);
    const vrt::filter::Guides g{static_cast<const float *>(d.normal), static_cast<const float *>(d.albedo), static_cast<const float *>(d.depth),
                                static_cast<const float *>(d.coverage)};
    vrt::filter::LevelVar q{};
    q.l.rgb = static_cast<const float *>(d.rgb);
    q.l.width = width;
    q.l.height = height;
    q.l.kn = k.kn;
    q.l.ka = k.ka;
    q.l.sigma_depth = k.f.sigma_depth;
    q.l.demodulate = (k.f.flags & VRT_FILTER_DEMODULATE) ? 1u : 0u;
    q.l.op = tm ? tm->op : VRT_TONEMAP_CLAMP;
    q.l.exposure = tm ? tm->exposure : 1.0f;
    q.sigma_lum = k.f.sigma_lum;
    if (levels == 0) {   // the colours are the same in both forms
        const vrt::filter::Through t{q.l.rgb, g, out_rgb, out_rgba, (uint32_t)px, q.l.demodulate, q.l.op, q.l.exposure};
        VRT_HIP(c, vrt::launch::filter_through(t, s));
        if (!out_variance) return VRT_OK;   // else V2's variance is the output: scratch for one level, the prepass, the variance kernel
    }
    if ((r = ensure_level_scratch(c, px, levels ? levels : 1))) return r;
    vrt_ctx::FilterScratch &fs = c->filter;
    if (fs.used && fs.last != s) VRT_HIP(c, hipStreamWaitEvent(s, fs.done, 0));   // the scratch is still the last call's
    VRT_HIP(c, vrt::launch::filter_prepass(vrt::filter::Prepass{g, fs.d_pack, width, height}, s));
    q.l.pack = fs.d_pack;
    if (k.var)
        VRT_HIP(c, vrt::launch::filter_variance(vrt::filter::Variance{q.l, reinterpret_cast<float *>(fs.d_pack.get()),
                                                                      static_cast<const float *>(d.variance), levels == 0 ? out_variance : nullptr},
                                                s));
    for (int i = 0; i < levels; ++i) {
        const bool first = i == 0, last = i == levels - 1;
        q.l.step = 1 << i;
        q.l.src = first ? nullptr : ((i & 1) ? fs.d_ping.get() : fs.d_pong.get());   // level 0 writes ping, level 1 pong, ...
        q.l.dst = last ? nullptr : ((i & 1) ? fs.d_pong.get() : fs.d_ping.get());
        q.l.out_rgb = last ? out_rgb : nullptr;
        q.l.out_rgba = last ? out_rgba : nullptr;
        q.out_variance = last ? out_variance : nullptr;
        if (k.var) VRT_HIP(c, vrt::launch::filter_level(q, first, last, s));
        else VRT_HIP(c, vrt::launch::filter_level(q.l, first, last, s));
    }
    VRT_HIP(c, hipEventRecord(fs.done, s));
    fs.last = s;
    fs.used = true;
    return VRT_OK;
}

// The layout of both staging blocks (the context's for the host forms, the accumulation's for its filtered resolves): mean or caller's
// image, the four planes, the float output and the bytes; for the variance-guided forms (var) the variance plane in and out behind
// them. u: the caller's planes; `in`: what the first five are -- the caller's, or (kKept) made on the device. The variance input is
// the caller's or none.
enum { kRgb, kNormal, kAlbedo, kDepth, kCoverage, kOutRgb, kOutRgba, kVariance, kOutVariance };
void declare(vrt_stage::Stage &st, size_t px, bool var, vrt_stage::Dir in, const Planes &u) {
    st.add(in, px * 12, u.rgb);
    st.add(in, px * 12, u.normal);
    st.add(in, px * 16, u.albedo);
    st.add(in, px * 4, u.depth);
    st.add(in, px * 4, u.coverage);
    st.out(px * 12, u.out_rgb);
    st.out(px * 4, u.out_rgba8);
    st.in(var ? px * 4 : 0, u.variance);
    st.out(var ? px * 4 : 0, u.out_variance);
}
Planes planes_of(const vrt_stage::Stage &st) {   // ... as a launch gets them
    return Planes{st.at(kRgb), st.at(kNormal), st.at(kAlbedo), st.at(kDepth), st.at(kCoverage), st.at(kVariance), st.at(kOutRgb), st.at(kOutRgba),
                  st.at(kOutVariance)};
}

// the host forms: the caller's planes h through the context's staging block, on the context's stream
int filter_host(vrt_ctx *c, const char *what, int width, int height, const Planes &h, Params k, const vrt_tonemap *tm) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if ((r = check_call(c, what, &h, h.out_rgb, h.out_rgba8, k, tm, false))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    vrt_stage::Stage st(4);
    declare(st, px, k.var, vrt_stage::kIn, h);
    if ((r = st.reserve_synced(c, c->filter.d_host)) || (r = st.upload(c, c->stream))) return r;
    r = filter_frame(c, what, width, height, planes_of(st), k, tm, nullptr);
    return r ? r : st.download(c, c->stream);
}

// The accumulation forms: mean and planes into the accumulation's stage and the filter on them. to_host: the outputs are the caller's
// host buffers, filled on the context's stream before the return; else device memory, written in the order of `stream`. The
// variance-guided form takes the variance an accumulation that keeps moments has measured (vrt_accum_variance_device's plane, M3,
// through the accumulation's own four bytes per pixel) once every pixel holds two samples; any other accumulation has none of its
// own, and the form estimates it spatially.
int filter_accum(vrt_ctx *c, const char *what, Params k, const vrt_tonemap *tm, bool to_host, void *out_rgb, void *out_rgba8, void *out_variance,
                 void *stream) {
    int r = accum_state(c, what, true);   // the call-order checks: those of vrt_accum_guides, then vrt_accum_resolve_hdr's
    if (r || (r = check_call(c, what, nullptr, out_rgb, out_rgba8, k, tm, false))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt_ctx::Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    vrt_stage::Stage st(4, to_host);
    declare(st, px, k.var, vrt_stage::kKept, Planes{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out_rgb, out_rgba8, out_variance});
    if ((r = st.reserve_synced(c, ac.d_filter))) return r;
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((r = vrt_accum_guides_device(c, st.at(kNormal), st.at(kAlbedo), st.at(kDepth), st.at(kCoverage), s))) return r;   // brings the guide state up to date first
    if ((r = vrt_accum_resolve_hdr_device(c, st.at(kRgb), tm, nullptr, nullptr, s))) return r;
    Planes p = planes_of(st);
    if (k.var && ac.moments && ac.total >= 2u) {   // (adaptive: min_samples >= 2, so every pixel holds two samples)
        if ((r = ensure_variance_plane(c)) || (r = vrt_accum_variance_device(c, ac.d_mvar, s))) return r;
        p.variance = ac.d_mvar;
    }
    // the stage belongs to the accumulation, whose every use the context's stream orders: a caller's stream is joined back
    r = accum_joined(c, s, [&] { return filter_frame(c, what, ac.width, ac.height, p, k, tm, s); });
    return r ? r : st.download(c, c->stream);
}

}  // namespace

namespace vrt_internal {

int filter_var_check(vrt_ctx *c, const char *what, const vrt_filter_var *f, const vrt_tonemap *tm, const void *out_rgb, const void *out_rgba8) {
    Params k = params_of(f);
    return check_call(c, what, nullptr, const_cast<void *>(out_rgb), const_cast<void *>(out_rgba8), k, tm, false);
}

int filter_var_frame(vrt_ctx *c, const char *what, int width, int height, const void *d_rgb, const void *d_normal, const void *d_albedo,
                     const void *d_depth, const void *d_coverage, const void *d_variance, const vrt_filter_var *f, const vrt_tonemap *tm,
                     void *d_out_rgb, void *d_out_rgba8, void *d_out_variance, void *stream) {
    const Planes d{d_rgb, d_normal, d_albedo, d_depth, d_coverage, d_variance, d_out_rgb, d_out_rgba8, d_out_variance};
    return filter_frame(c, what, width, height, d, params_of(f), tm, stream);
}

}  // namespace vrt_internal

extern "C" {

void vrt_filter_default(vrt_filter *f) {
    if (!f) return;
    f->levels = 1;
    f->flags = VRT_FILTER_DEMODULATE;
    f->sigma_normal = 1.0f;
    f->sigma_albedo = 0.05f;
    f->sigma_depth = 2.0f;
}

void vrt_filter_var_default(vrt_filter_var *f) {
    if (!f) return;
    f->levels = 3;
    f->flags = VRT_FILTER_DEMODULATE;
    f->sigma_normal = 0.5f;
    f->sigma_albedo = 0.05f;
    f->sigma_depth = 2.0f;
    f->sigma_lum = 4.0f;
}

int vrt_filter_hdr(vrt_ctx *c, int width, int height, const void *d_rgb, const void *d_normal, const void *d_albedo, const void *d_depth,
                   const void *d_coverage, const vrt_filter *f, const vrt_tonemap *tm, void *d_out_rgb, void *d_out_rgba8, void *stream) {
    const Planes d{d_rgb, d_normal, d_albedo, d_depth, d_coverage, nullptr, d_out_rgb, d_out_rgba8, nullptr};
    return filter_frame(c, "vrt_filter_hdr", width, height, d, params_of(f), tm, stream);
}

int vrt_filter_hdr_var(vrt_ctx *c, int width, int height, const void *d_rgb, const void *d_normal, const void *d_albedo, const void *d_depth,
                       const void *d_coverage, const void *d_variance, const vrt_filter_var *f, const vrt_tonemap *tm, void *d_out_rgb,
                       void *d_out_rgba8, void *d_out_variance, void *stream) {
    const Planes d{d_rgb, d_normal, d_albedo, d_depth, d_coverage, d_variance, d_out_rgb, d_out_rgba8, d_out_variance};
    return filter_frame(c, "vrt_filter_hdr_var", width, height, d, params_of(f), tm, stream);
}

int vrt_filter_hdr_host(vrt_ctx *c, int width, int height, const float *rgb, const float *normal, const float *albedo, const float *depth,
                        const float *coverage, const vrt_filter *f, const vrt_tonemap *tm, float *out_rgb, uint8_t *out_rgba8) {
    const Planes h{rgb, normal, albedo, depth, coverage, nullptr, out_rgb, out_rgba8, nullptr};
    return filter_host(c, "vrt_filter_hdr_host", width, height, h, params_of(f), tm);
}

int vrt_filter_hdr_var_host(vrt_ctx *c, int width, int height, const float *rgb, const float *normal, const float *albedo, const float *depth,
                            const float *coverage, const float *variance, const vrt_filter_var *f, const vrt_tonemap *tm, float *out_rgb,
                            uint8_t *out_rgba8, float *out_variance) {
    const Planes h{rgb, normal, albedo, depth, coverage, variance, out_rgb, out_rgba8, out_variance};
    return filter_host(c, "vrt_filter_hdr_var_host", width, height, h, params_of(f), tm);
}

int vrt_accum_resolve_hdr_filtered(vrt_ctx *c, const vrt_filter *f, const vrt_tonemap *tm, float *out_rgb, uint8_t *out_rgba8) {
    return filter_accum(c, "vrt_accum_resolve_hdr_filtered", params_of(f), tm, true, out_rgb, out_rgba8, nullptr, nullptr);
}

int vrt_accum_resolve_hdr_filtered_device(vrt_ctx *c, const vrt_filter *f, const vrt_tonemap *tm, void *d_rgb, void *d_rgba8, void *stream) {
    return filter_accum(c, "vrt_accum_resolve_hdr_filtered_device", params_of(f), tm, false, d_rgb, d_rgba8, nullptr, stream);
}

int vrt_accum_resolve_hdr_filtered_var(vrt_ctx *c, const vrt_filter_var *f, const vrt_tonemap *tm, float *out_rgb, uint8_t *out_rgba8,
                                       float *out_variance) {
    return filter_accum(c, "vrt_accum_resolve_hdr_filtered_var", params_of(f), tm, true, out_rgb, out_rgba8, out_variance, nullptr);
}

int vrt_accum_resolve_hdr_filtered_var_device(vrt_ctx *c, const vrt_filter_var *f, const vrt_tonemap *tm, void *d_rgb, void *d_rgba8,
                                              void *d_variance_out, void *stream) {
    return filter_accum(c, "vrt_accum_resolve_hdr_filtered_var_device", params_of(f), tm, false, d_rgb, d_rgba8, d_variance_out, stream);
}

}  // extern "C"
