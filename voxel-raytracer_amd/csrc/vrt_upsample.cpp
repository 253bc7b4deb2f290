// vrt_upsample.cpp -- guided upsampling (include/vrt.h vrt_upsample_hdr, its host form and the accumulation forms). One route serves
// all four (upsample_frame): validation and the one launch; it reads no context state and keeps no scratch. One helper stages host
// planes around it (upsample_host), one brings an HDR accumulation's float mean and its own guide planes -- the LOW side -- and the
// guide planes of the frame r times its size (vrt_guides.cpp guide_frame_planes) into the accumulation's stage and runs the pass on
// them (upsample_accum). Host code; the kernel is behind vrt_launch.h. Nothing here touches the accumulation's sums.
#include "vrt_stage.h"
#include "vrt_launch.h"

#include <cmath>

using namespace vrt_internal;

namespace {

bool in_range(float v, float lo, float hi) { return v >= lo && v <= hi; }   // false for NaN

// a call's planes, in device memory or (the host form) the caller's
struct Io {
    const void *rgb, *normal, *albedo, *depth, *coverage;   // low
    const void *hi_normal, *hi_albedo, *hi_depth, *hi_coverage;
    void *out_rgb, *out_rgba8, *out_unresolved;
};

// The parameters a call runs with (NULL: vrt_upsample_default) and kn, ka, which check_params fills
struct Params {
    vrt_upsample u;
    float kn = 0.0f, ka = 0.0f;
    explicit Params(const vrt_upsample *p) {
        if (p) u = *p;
        else vrt_upsample_default(&u);
    }
};

// VRT_E_INVALID in the name of `what` unless k.u is one the header allows. Needs no device.
int check_params(vrt_ctx *c, const char *what, Params &k) {
    const std::string w(what);
    const vrt_upsample &u = k.u;
    if (u.factor < 1 || u.factor > VRT_UPSAMPLE_MAX_FACTOR) return vrt_fail(c, VRT_E_INVALID, w + ": factor must be in 1..VRT_UPSAMPLE_MAX_FACTOR");
    if (u.flags & ~(uint32_t)VRT_UPSAMPLE_DEMODULATE) return vrt_fail(c, VRT_E_INVALID, w + ": unknown flags");
    for (const float sg : {u.sigma_normal, u.sigma_albedo, u.sigma_depth})
        if (!(sg > 0.0f) || !(sg <= 3.402823466e38f)) return vrt_fail(c, VRT_E_INVALID, w + ": every sigma must be finite and > 0");
    k.kn = 1.0f / (u.sigma_normal * u.sigma_normal);
    k.ka = 1.0f / (u.sigma_albedo * u.sigma_albedo);
    if (!(k.kn <= 3.402823466e38f) || !(k.ka <= 3.402823466e38f))
        return vrt_fail(c, VRT_E_INVALID, w + ": sigma_normal or sigma_albedo too small (1 / sigma^2 is not finite)");
    if (!(u.min_weight >= 0.0f && u.min_weight < 1.0f)) return vrt_fail(c, VRT_E_INVALID, w + ": min_weight must be in [0, 1)");
    if (!in_range(u.offset_lo_x, 0.0f, 1.0f) || !in_range(u.offset_lo_y, 0.0f, 1.0f) || !in_range(u.offset_hi_x, 0.0f, 1.0f) ||
        !in_range(u.offset_hi_y, 0.0f, 1.0f))
        return vrt_fail(c, VRT_E_INVALID, w + ": every offset must be in [0, 1]");
    return VRT_OK;
}

// what every form checks of its outputs, parameters and tone map before anything is enqueued
int check_call(vrt_ctx *c, const char *what, const void *out_rgb, const void *out_rgba8, Params &k, const vrt_tonemap *tm) {
    if (!out_rgb && !out_rgba8) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": both colour outputs null");
    const int r = check_params(c, what, k);
    return r ? r : check_tonemap(c, what, tm);
}

// ... and of its pointers; device: equal pointers alias
int check_io(vrt_ctx *c, const char *what, const Io &io, bool device) {
    const std::string w(what);
    const void *const ins[9] = {io.rgb, io.normal, io.albedo, io.depth, io.coverage, io.hi_normal, io.hi_albedo, io.hi_depth, io.hi_coverage};
    for (const void *in : ins)
        if (!in) return vrt_fail(c, VRT_E_INVALID, w + ": null input");
    if (!device) return VRT_OK;
    const void *const outs[3] = {io.out_rgb, io.out_rgba8, io.out_unresolved};
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        for (const void *in : ins)
            if (outs[i] == in) return vrt_fail(c, VRT_E_INVALID, w + ": an output must not alias an input");
        for (int j = 0; j < i; ++j)
            if (outs[i] == outs[j]) return vrt_fail(c, VRT_E_INVALID, w + ": the outputs must not alias each other");
    }
    return VRT_OK;
}

// the frame-size rule for the low frame and the high one, whose sides are r times the low one's
int check_sizes(vrt_ctx *c, const char *what, int width, int height, int factor) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (width > 0x7fffffff / factor || height > 0x7fffffff / factor)
        return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": the high frame is too large");
    return check_frame(c, width * factor, height * factor);
}

// The stateless pass on device planes, stream-ordered, in the name of `what`; k: checked
int upsample_launch(vrt_ctx *c, int width, int height, const Io &d, const Params &k, const vrt_tonemap *tm, hipStream_t s) {
    vrt::upsample::Args q{};
    q.rgb = static_cast<const float *>(d.rgb);
    q.normal = static_cast<const float *>(d.normal);
    q.albedo = static_cast<const float *>(d.albedo);
    q.depth = static_cast<const float *>(d.depth);
    q.coverage = static_cast<const float *>(d.coverage);
    q.hi_normal = static_cast<const float *>(d.hi_normal);
    q.hi_albedo = static_cast<const float *>(d.hi_albedo);
    q.hi_depth = static_cast<const float *>(d.hi_depth);
    q.hi_coverage = static_cast<const float *>(d.hi_coverage);
    q.out_rgb = static_cast<float *>(d.out_rgb);
    q.out_rgba = static_cast<uint32_t *>(d.out_rgba8);
    q.out_unresolved = static_cast<uint8_t *>(d.out_unresolved);
    q.width = width;
    q.height = height;
    q.factor = k.u.factor;
    q.demodulate = (k.u.flags & VRT_UPSAMPLE_DEMODULATE) ? 1u : 0u;
    q.kn = k.kn;
    q.ka = k.ka;
    q.sigma_depth = k.u.sigma_depth;
    q.min_weight = k.u.min_weight;
    q.offset_lo_x = k.u.offset_lo_x;
    q.offset_lo_y = k.u.offset_lo_y;
    q.offset_hi_x = k.u.offset_hi_x;
    q.offset_hi_y = k.u.offset_hi_y;
    q.op = tm ? tm->op : VRT_TONEMAP_CLAMP;
    q.exposure = tm ? tm->exposure : 1.0f;
    VRT_HIP(c, vrt::launch::upsample_pass(q, s));
    return VRT_OK;
}

int upsample_frame(vrt_ctx *c, const char *what, int width, int height, const Io &d, Params k, const vrt_tonemap *tm, hipStream_t s) {
    int r = check_io(c, what, d, true);
    if (r || (r = check_call(c, what, d.out_rgb, d.out_rgba8, k, tm)) || (r = check_sizes(c, what, width, height, k.u.factor))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    return upsample_launch(c, width, height, d, k, tm, s);
}

// The host form: the caller's planes staged around the pass on the context's stream, synchronous
int upsample_host(vrt_ctx *c, const char *what, int width, int height, const Io &h, Params k, const vrt_tonemap *tm) {
    int r = check_io(c, what, h, false);
    if (r || (r = check_call(c, what, h.out_rgb, h.out_rgba8, k, tm)) || (r = check_sizes(c, what, width, height, k.u.factor))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height, hpx = px * (size_t)k.u.factor * (size_t)k.u.factor;
    vrt_stage::Stage st(4);
    const int rgb = st.in(px * 12, h.rgb), normal = st.in(px * 12, h.normal), albedo = st.in(px * 16, h.albedo), depth = st.in(px * 4, h.depth);
    const int coverage = st.in(px * 4, h.coverage);
    const int hn = st.in(hpx * 12, h.hi_normal), ha = st.in(hpx * 16, h.hi_albedo), hz = st.in(hpx * 4, h.hi_depth), hc = st.in(hpx * 4, h.hi_coverage);
    const int o_rgb = st.out(hpx * 12, h.out_rgb), o_rgba = st.out(hpx * 4, h.out_rgba8), o_un = st.out(hpx, h.out_unresolved);
    if ((r = st.reserve_synced(c, c->d_upsample)) || (r = st.upload(c, c->stream))) return r;
    const Io d{st.at(rgb), st.at(normal), st.at(albedo), st.at(depth), st.at(coverage), st.at(hn), st.at(ha), st.at(hz), st.at(hc),
               st.at(o_rgb), st.at(o_rgba), st.at(o_un)};
    r = upsample_launch(c, width, height, d, k, tm, c->stream);
    return r ? r : st.download(c, c->stream);
}

// The accumulation forms. to_host: the outputs are the caller's host buffers, filled on the context's stream before the return; else
// device memory, written in the order of `stream`.
int upsample_accum(vrt_ctx *c, const char *what, Params k, const vrt_tonemap *tm, bool to_host, void *out_rgb, void *out_rgba8,
                   void *out_unresolved, void *stream) {
    int r = accum_state(c, what, true);   // the call-order checks: those of vrt_accum_guides, then vrt_accum_resolve_hdr's
    if (r || (r = check_call(c, what, out_rgb, out_rgba8, k, tm))) return r;
    vrt_ctx::Accum &ac = c->accum;
    if ((r = check_sizes(c, what, ac.width, ac.height, k.u.factor))) return r;
    // the high planes are marched now, with the context's inputs: they must still be those of the samples in the sums
    if (!accum_inputs_current(c))
        return vrt_fail(c, VRT_E_STATE, std::string(what) + ": camera, uniforms, tree or lens changed since the last vrt_accum_add");
    VRT_HIP(c, hipSetDevice(c->device));
    const int f = k.u.factor;
    const size_t px = (size_t)ac.width * (size_t)ac.height, hpx = px * (size_t)f * (size_t)f;
    k.u.offset_lo_x = k.u.offset_lo_y = (ac.flags & VRT_ACCUM_JITTER) ? 0.5f : 0.0f;
    k.u.offset_hi_x = k.u.offset_hi_y = 0.0f;
    // the accumulation's stage: the mean, its planes, the high planes, the outputs
    vrt_stage::Stage st(4, to_host);
    const int mean = st.kept(px * 12), normal = st.kept(px * 12), albedo = st.kept(px * 16), depth = st.kept(px * 4), coverage = st.kept(px * 4);
    const int hn = st.kept(hpx * 12), ha = st.kept(hpx * 16), hz = st.kept(hpx * 4), hc = st.kept(hpx * 4);
    const int o_rgb = st.out(hpx * 12, out_rgb), o_rgba = st.out(hpx * 4, out_rgba8), o_un = st.out(hpx, out_unresolved);
    if ((r = st.reserve_synced(c, ac.d_filter))) return r;
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((r = vrt_accum_guides_device(c, st.at(normal), st.at(albedo), st.at(depth), st.at(coverage), s))) return r;   // brings the guide state up to date first
    if ((r = vrt_accum_resolve_hdr_device(c, st.at(mean), tm, nullptr, nullptr, s))) return r;
    if ((r = guide_frame_planes(c, what, ac.width * f, ac.height * f, ac.guide_glass, st.at<float>(hn), st.at<float>(ha), st.at<float>(hz),
                                st.at<float>(hc), s)))
        return r;
    const Io d{st.at(mean), st.at(normal), st.at(albedo), st.at(depth), st.at(coverage), st.at(hn), st.at(ha), st.at(hz), st.at(hc),
               st.at(o_rgb), st.at(o_rgba), st.at(o_un)};
    // the stage belongs to the accumulation, whose every use the context's stream orders: a caller's stream is joined back
    r = accum_joined(c, s, [&] { return upsample_launch(c, ac.width, ac.height, d, k, tm, s); });
    return r ? r : st.download(c, c->stream);
}

}  // namespace

extern "C" {

void vrt_upsample_default(vrt_upsample *u) {
    if (!u) return;
    u->factor = 2;
    u->flags = VRT_UPSAMPLE_DEMODULATE;
    u->sigma_normal = 0.5f;   // profiles/upsample_quality.txt's best row
    u->sigma_albedo = 0.05f;
    u->sigma_depth = 0.5f;
    u->min_weight = 0.0f;
    u->offset_lo_x = u->offset_lo_y = u->offset_hi_x = u->offset_hi_y = 0.0f;
}

int vrt_upsample_hdr(vrt_ctx *c, int width, int height, const void *d_rgb, const void *d_normal, const void *d_albedo, const void *d_depth,
                     const void *d_coverage, const void *d_hi_normal, const void *d_hi_albedo, const void *d_hi_depth,
                     const void *d_hi_coverage, const vrt_upsample *u, const vrt_tonemap *tm, void *d_out_rgb, void *d_out_rgba8,
                     void *d_out_unresolved, void *stream) {
    if (!c) return VRT_E_INVALID;
    const Io d{d_rgb, d_normal, d_albedo, d_depth, d_coverage, d_hi_normal, d_hi_albedo, d_hi_depth, d_hi_coverage, d_out_rgb, d_out_rgba8,
               d_out_unresolved};
    return upsample_frame(c, "vrt_upsample_hdr", width, height, d, Params(u), tm, stream ? (hipStream_t)stream : c->stream);
}

int vrt_upsample_hdr_host(vrt_ctx *c, int width, int height, const float *rgb, const float *normal, const float *albedo, const float *depth,
                          const float *coverage, const float *hi_normal, const float *hi_albedo, const float *hi_depth,
                          const float *hi_coverage, const vrt_upsample *u, const vrt_tonemap *tm, float *out_rgb, uint8_t *out_rgba8,
                          uint8_t *out_unresolved) {
    if (!c) return VRT_E_INVALID;
    const Io h{rgb, normal, albedo, depth, coverage, hi_normal, hi_albedo, hi_depth, hi_coverage, out_rgb, out_rgba8, out_unresolved};
    return upsample_host(c, "vrt_upsample_hdr_host", width, height, h, Params(u), tm);
}

int vrt_accum_resolve_hdr_upsampled(vrt_ctx *c, const vrt_upsample *u, const vrt_tonemap *tm, float *out_rgb, uint8_t *out_rgba8,
                                    uint8_t *out_unresolved) {
    return upsample_accum(c, "vrt_accum_resolve_hdr_upsampled", Params(u), tm, true, out_rgb, out_rgba8, out_unresolved, nullptr);
}

int vrt_accum_resolve_hdr_upsampled_device(vrt_ctx *c, const vrt_upsample *u, const vrt_tonemap *tm, void *d_rgb, void *d_rgba8,
                                           void *d_unresolved, void *stream) {
    return upsample_accum(c, "vrt_accum_resolve_hdr_upsampled_device", Params(u), tm, false, d_rgb, d_rgba8, d_unresolved, stream);
}

}  // extern "C"
