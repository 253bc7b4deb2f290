// vrt_temporal.cpp -- the temporal pass (include/vrt.h vrt_temporal_hdr, its host form and the accumulation forms that chain it with
// vrt_filter_hdr_var) and its measured-variance form (vrt_temporal_hdr_mom and its three: a Mom beside the parameters, a variance
// plane among the inputs). One route serves all eight (temporal_frame): validation and the one launch; it reads no context state and
// keeps no scratch. One helper stages host planes and histories around it (vrt_temporal_hdr_host), one brings an HDR accumulation's
// float mean and its own guide planes into the accumulation's filter stage, runs the pass on them with the context's current camera
// block and the variance-guided filter on what it returns (temporal_accum). Host code; the kernel is behind vrt_launch.h. Nothing
// here touches the accumulation's sums.
#include "vrt_stage.h"
#include "vrt_launch.h"

#include <cmath>
#include <cstddef>
#include <cstring>

using namespace vrt_internal;

namespace {

constexpr size_t kHistory = vrt::temporal::kHistoryBytes;

bool all_finite(const float *v, int n) {
    for (int i = 0; i < n; ++i)
        if (!(std::fabs(v[i]) <= 3.402823466e38f)) return false;
    return true;
}
bool in_range(float v, float lo, float hi) { return v >= lo && v <= hi; }   // false for NaN

// a frame's planes and histories, in device memory or (the host form) the caller's
struct Io {
    const void *rgb, *normal, *depth, *coverage, *history_in;
    void *history_out, *out_rgb, *out_variance;
    const void *variance = nullptr;   // the measured-variance form's input, may be null there
};

// what vrt_temporal_mom adds to vrt_temporal; null for the calls that take a vrt_temporal
struct Mom {
    int32_t measured_below, search;
};

// a vrt_temporal_mom as the vrt_temporal it begins with and its Mom
static_assert(offsetof(vrt_temporal_mom, measured_below) == sizeof(vrt_temporal) && sizeof(vrt_temporal_mom) == sizeof(vrt_temporal) + sizeof(Mom),
              "vrt_temporal_mom is vrt_temporal's fields in their order, then two");
struct Split {
    vrt_temporal t{};
    Mom m{};
    const vrt_temporal *tp = nullptr;   // null where the caller's pointer was
    explicit Split(const vrt_temporal_mom *tm) {
        if (!tm) return;
        std::memcpy(&t, tm, sizeof t);
        m = Mom{tm->measured_below, tm->search};
        tp = &t;
    }
};

// VRT_E_INVALID in the name of `what` unless t is one the header allows; the previous camera only where a history comes in
int check_params(vrt_ctx *c, const char *what, const vrt_temporal *t, const Mom *m, bool have_history) {
    const std::string w(what);
    if (!t) return vrt_fail(c, VRT_E_INVALID, w + ": null vrt_temporal");
    if (m && (m->measured_below < 1 || m->measured_below > 32769)) return vrt_fail(c, VRT_E_INVALID, w + ": measured_below must be in 1..32769");
    if (m && m->search != 0 && m->search != 1) return vrt_fail(c, VRT_E_INVALID, w + ": search must be 0 or 1");
    if (t->max_history < 1 || t->max_history > 32768) return vrt_fail(c, VRT_E_INVALID, w + ": max_history must be in 1..32768");
    if (!in_range(t->alpha_min, 0.0f, 1.0f) || !in_range(t->alpha_moments_min, 0.0f, 1.0f))
        return vrt_fail(c, VRT_E_INVALID, w + ": alpha_min and alpha_moments_min must be in [0, 1]");
    if (!in_range(t->normal_min, -1.0f, 1.0f)) return vrt_fail(c, VRT_E_INVALID, w + ": normal_min must be in [-1, 1]");
    if (!(t->depth_tol > 0.0f) || !(t->depth_tol <= 3.402823466e38f)) return vrt_fail(c, VRT_E_INVALID, w + ": depth_tol must be finite and > 0");
    if (!in_range(t->offset_x, 0.0f, 1.0f) || !in_range(t->offset_y, 0.0f, 1.0f))
        return vrt_fail(c, VRT_E_INVALID, w + ": offset_x and offset_y must be in [0, 1]");
    if (have_history && (!all_finite(t->prev_view_proj, 16) || !all_finite(t->prev_camera_pos, 3)))
        return vrt_fail(c, VRT_E_INVALID, w + ": prev_view_proj or prev_camera_pos is not finite");
    return VRT_OK;
}

int check_camera(vrt_ctx *c, const char *what, const float *inv_proj, const float *inv_view, const float *cam_pos) {
    if (!inv_proj || !inv_view || !cam_pos) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null camera");
    if (!all_finite(inv_proj, 16) || !all_finite(inv_view, 16) || !all_finite(cam_pos, 3))
        return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": the camera block is not finite");
    return VRT_OK;
}

// what every form checks of a call's pointers; device: equal pointers alias, and a history must hold whole 16-byte words
int check_io(vrt_ctx *c, const char *what, const Io &io, bool device) {
    const std::string w(what);
    if (!io.rgb || !io.normal || !io.depth || !io.coverage) return vrt_fail(c, VRT_E_INVALID, w + ": null input");
    if (!io.history_out) return vrt_fail(c, VRT_E_INVALID, w + ": null history_out");
    if (!device) return VRT_OK;
    const void *const ins[6] = {io.rgb, io.normal, io.depth, io.coverage, io.history_in, io.variance};
    const void *const outs[3] = {io.history_out, io.out_rgb, io.out_variance};
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        for (const void *in : ins)
            if (outs[i] == in) return vrt_fail(c, VRT_E_INVALID, w + ": d_history_out, d_out_rgb and d_out_variance must not alias an input");
        for (int j = 0; j < i; ++j)
            if (outs[i] == outs[j]) return vrt_fail(c, VRT_E_INVALID, w + ": the outputs must not alias each other");
    }
    if (((uintptr_t)io.history_in | (uintptr_t)io.history_out) & 15u) return vrt_fail(c, VRT_E_INVALID, w + ": a history must be 16-byte aligned");
    return VRT_OK;
}

// The stateless pass on device planes, stream-ordered, in the name of `what`; m: the kernel's second form
int temporal_frame(vrt_ctx *c, const char *what, int width, int height, const float *inv_proj, const float *inv_view, const float *cam_pos,
                   const Io &d, const vrt_temporal *t, const Mom *m, hipStream_t s) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if ((r = check_io(c, what, d, true))) return r;
    if ((r = check_params(c, what, t, m, d.history_in != nullptr))) return r;
    if ((r = check_camera(c, what, inv_proj, inv_view, cam_pos))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt::temporal::ArgsMom q{};
    q.rgb = static_cast<const float *>(d.rgb);
    q.normal = static_cast<const float *>(d.normal);
    q.depth = static_cast<const float *>(d.depth);
    q.coverage = static_cast<const float *>(d.coverage);
    q.history_in = static_cast<const float4 *>(d.history_in);
    q.history_out = static_cast<float4 *>(d.history_out);
    q.out_rgb = static_cast<float *>(d.out_rgb);
    q.out_variance = static_cast<float *>(d.out_variance);
    q.width = width;
    q.height = height;
    std::memcpy(q.inv_proj, inv_proj, sizeof q.inv_proj);
    std::memcpy(q.inv_view, inv_view, sizeof q.inv_view);
    std::memcpy(q.cam_pos, cam_pos, sizeof q.cam_pos);
    if (d.history_in) {   // else never read: zeros
        std::memcpy(q.prev_view_proj, t->prev_view_proj, sizeof q.prev_view_proj);
        std::memcpy(q.prev_cam_pos, t->prev_camera_pos, sizeof q.prev_cam_pos);
    }
    q.offset_x = t->offset_x;
    q.offset_y = t->offset_y;
    q.max_history = (float)t->max_history;
    q.alpha_min = t->alpha_min;
    q.alpha_moments_min = t->alpha_moments_min;
    q.normal_min = t->normal_min;
    q.depth_tol = t->depth_tol;
    if (!m) {
        VRT_HIP(c, vrt::launch::temporal_pass(q, s));   // the Args it begins with
        return VRT_OK;
    }
    q.variance_in = static_cast<const float *>(d.variance);
    q.measured_below = (float)m->measured_below;
    q.search = m->search;
    VRT_HIP(c, vrt::launch::temporal_pass_mom(q, s));
    return VRT_OK;
}

// The accumulation forms: mean and planes into the accumulation's stage, the pass on them, the filter on its outputs. to_host: the
// histories and the outputs are the caller's host buffers, staged behind the stage's planes and filled on the context's stream
// before the return; else device memory, read and written in the order of `stream`.
int temporal_accum(vrt_ctx *c, const char *what, const vrt_temporal *t, const Mom *m, const vrt_filter_var *f, const vrt_tonemap *tm, bool to_host,
                   const void *history_in, void *history_out, void *out_integrated, void *out_rgb, void *out_rgba8, void *out_variance,
                   void *stream) {
    int r = accum_state(c, what, true);   // the call-order checks: those of vrt_accum_guides, then vrt_accum_resolve_hdr's
    if (r) return r;
    if (!history_out) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null history_out");
    if (history_out == history_in) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": history_out must differ from history_in");
    if ((r = check_params(c, what, t, m, history_in != nullptr))) return r;
    if ((r = filter_var_check(c, what, f, tm, out_rgb, out_rgba8))) return r;
    if ((r = check_camera(c, what, c->inv_proj, c->inv_view, c->cam_pos))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt_ctx::Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    // the accumulation's stage: the mean, its planes, the pass's integrated image and variance, the filter's outputs; the host form's
    // histories behind them, as the 16-byte words the pass reads -- device histories are the caller's and take no room
    vrt_stage::Stage st(4, to_host);
    const int mean = st.kept(px * 12), normal = st.kept(px * 12), albedo = st.kept(px * 16), depth = st.kept(px * 4), coverage = st.kept(px * 4);
    const int integrated = st.kept(px * 12, out_integrated), variance = st.kept(px * 4);
    const int f_rgb = st.out(px * 12, out_rgb), f_rgba = st.out(px * 4, out_rgba8), f_var = st.out(px * 4, out_variance);
    if (to_host) st.align = 16;
    const int hin = st.in(to_host ? px * kHistory : 0, history_in), hout = st.out(to_host ? px * kHistory : 0, history_out);
    if ((r = st.reserve_synced(c, ac.d_filter))) return r;
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((r = vrt_accum_guides_device(c, st.at(normal), st.at(albedo), st.at(depth), st.at(coverage), s))) return r;   // brings the guide state up to date first
    if ((r = vrt_accum_resolve_hdr_device(c, st.at(mean), tm, nullptr, nullptr, s))) return r;
    vrt_temporal tt = *t;
    tt.offset_x = tt.offset_y = (ac.flags & VRT_ACCUM_JITTER) ? 0.5f : 0.0f;
    if ((r = st.upload(c, s))) return r;
    Io d{st.at(mean), st.at(normal), st.at(depth), st.at(coverage), st.at(hin), st.at(hout), st.at(integrated), st.at(variance)};
    if (m && ac.moments) {   // the measured variance of this pose's mean: M3's plane, through the accumulation's own four bytes per pixel
        if ((r = ensure_variance_plane(c)) || (r = vrt_accum_variance_device(c, ac.d_mvar, s))) return r;
        d.variance = ac.d_mvar;
    }
    // the stage belongs to the accumulation, whose every use the context's stream orders: a caller's stream is joined back
    r = accum_joined(c, s, [&] {
        const int rt = temporal_frame(c, what, ac.width, ac.height, c->inv_proj, c->inv_view, c->cam_pos, d, &tt, m, s);
        if (rt) return rt;
        return filter_var_frame(c, what, ac.width, ac.height, d.out_rgb, d.normal, st.at(albedo), d.depth, d.coverage, d.out_variance, f, tm,
                                st.at(f_rgb), st.at(f_rgba), st.at(f_var), s);
    });
    return r ? r : st.download(c, c->stream);
}

// The host forms: the caller's planes and histories staged around the pass on the context's stream, synchronous. The measured-variance
// form stages its variance plane behind the others, four bytes per pixel more.
int temporal_host(vrt_ctx *c, const char *what, int width, int height, const float *inv_projection, const float *inv_view, const float *camera_pos,
                  const Io &h, const vrt_temporal *t, const Mom *m) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if ((r = check_io(c, what, h, false))) return r;
    if (h.history_out == h.history_in) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": history_out must differ from history_in");
    if ((r = check_params(c, what, t, m, h.history_in != nullptr))) return r;
    if ((r = check_camera(c, what, inv_projection, inv_view, camera_pos))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    vrt_stage::Stage st(4);   // both histories, the inputs, the integrated image and the variance
    const int hin = st.in(px * kHistory, h.history_in), hout = st.out(px * kHistory, h.history_out);
    const int s_rgb = st.in(px * 12, h.rgb), s_normal = st.in(px * 12, h.normal), s_depth = st.in(px * 4, h.depth), s_cov = st.in(px * 4, h.coverage);
    const int s_out = st.out(px * 12, h.out_rgb), s_var = st.out(px * 4, h.out_variance);
    const int s_vin = st.in(m ? px * 4 : 0, h.variance);
    if ((r = st.reserve_synced(c, c->d_temporal)) || (r = st.upload(c, c->stream))) return r;
    const Io d{st.at(s_rgb), st.at(s_normal), st.at(s_depth), st.at(s_cov), st.at(hin), st.at(hout), st.at(s_out), st.at(s_var), st.at(s_vin)};
    r = temporal_frame(c, what, width, height, inv_projection, inv_view, camera_pos, d, t, m, c->stream);
    return r ? r : st.download(c, c->stream);
}

}  // namespace

extern "C" {

void vrt_temporal_default(vrt_temporal *t) {
    if (!t) return;
    std::memset(t, 0, sizeof *t);
    t->max_history = 8;
    t->alpha_min = 0.4f;
    t->alpha_moments_min = 0.6f;
    t->normal_min = 0.0f;
    t->depth_tol = 0.4f;
}

int vrt_temporal_hdr(vrt_ctx *c, int width, int height, const float inv_projection[16], const float inv_view[16], const float camera_pos[4],
                     const void *d_rgb, const void *d_normal, const void *d_depth, const void *d_coverage, const void *d_history_in,
                     const vrt_temporal *t, void *d_history_out, void *d_out_rgb, void *d_out_variance, void *stream) {
    if (!c) return VRT_E_INVALID;
    const Io d{d_rgb, d_normal, d_depth, d_coverage, d_history_in, d_history_out, d_out_rgb, d_out_variance};
    return temporal_frame(c, "vrt_temporal_hdr", width, height, inv_projection, inv_view, camera_pos, d, t, nullptr, stream ? (hipStream_t)stream : c->stream);
}

int vrt_temporal_hdr_mom(vrt_ctx *c, int width, int height, const float inv_projection[16], const float inv_view[16], const float camera_pos[4],
                         const void *d_rgb, const void *d_normal, const void *d_depth, const void *d_coverage, const void *d_variance_in,
                         const void *d_history_in, const vrt_temporal_mom *t, void *d_history_out, void *d_out_rgb, void *d_out_variance,
                         void *stream) {
    if (!c) return VRT_E_INVALID;
    const Split k(t);
    const Io d{d_rgb, d_normal, d_depth, d_coverage, d_history_in, d_history_out, d_out_rgb, d_out_variance, d_variance_in};
    return temporal_frame(c, "vrt_temporal_hdr_mom", width, height, inv_projection, inv_view, camera_pos, d, k.tp, &k.m,
                          stream ? (hipStream_t)stream : c->stream);
}

int vrt_temporal_hdr_host(vrt_ctx *c, int width, int height, const float inv_projection[16], const float inv_view[16], const float camera_pos[4],
                          const float *rgb, const float *normal, const float *depth, const float *coverage, const void *history_in,
                          const vrt_temporal *t, void *history_out, float *out_rgb, float *out_variance) {
    const Io h{rgb, normal, depth, coverage, history_in, history_out, out_rgb, out_variance};
    return temporal_host(c, "vrt_temporal_hdr_host", width, height, inv_projection, inv_view, camera_pos, h, t, nullptr);
}

int vrt_temporal_hdr_mom_host(vrt_ctx *c, int width, int height, const float inv_projection[16], const float inv_view[16],
                              const float camera_pos[4], const float *rgb, const float *normal, const float *depth, const float *coverage,
                              const float *variance_in, const void *history_in, const vrt_temporal_mom *t, void *history_out, float *out_rgb,
                              float *out_variance) {
    const Split k(t);
    const Io h{rgb, normal, depth, coverage, history_in, history_out, out_rgb, out_variance, variance_in};
    return temporal_host(c, "vrt_temporal_hdr_mom_host", width, height, inv_projection, inv_view, camera_pos, h, k.tp, &k.m);
}

int vrt_accum_resolve_hdr_temporal(vrt_ctx *c, const vrt_temporal *t, const vrt_filter_var *f, const vrt_tonemap *tm, const void *history_in,
                                   void *history_out, float *out_integrated, float *out_rgb, uint8_t *out_rgba8, float *out_variance) {
    return temporal_accum(c, "vrt_accum_resolve_hdr_temporal", t, nullptr, f, tm, true, history_in, history_out, out_integrated, out_rgb, out_rgba8,
                          out_variance, nullptr);
}

int vrt_accum_resolve_hdr_temporal_device(vrt_ctx *c, const vrt_temporal *t, const vrt_filter_var *f, const vrt_tonemap *tm,
                                          const void *d_history_in, void *d_history_out, void *d_integrated, void *d_rgb, void *d_rgba8,
                                          void *d_variance_out, void *stream) {
    return temporal_accum(c, "vrt_accum_resolve_hdr_temporal_device", t, nullptr, f, tm, false, d_history_in, d_history_out, d_integrated, d_rgb, d_rgba8,
                          d_variance_out, stream);
}

void vrt_temporal_mom_default(vrt_temporal_mom *t) {
    if (!t) return;
    vrt_temporal base;
    vrt_temporal_default(&base);
    std::memcpy(t, &base, sizeof base);
    t->measured_below = 2;   // profiles/temporal_mom_quality.txt's best row
    t->search = 1;
}

int vrt_accum_resolve_hdr_temporal_mom(vrt_ctx *c, const vrt_temporal_mom *t, const vrt_filter_var *f, const vrt_tonemap *tm,
                                       const void *history_in, void *history_out, float *out_integrated, float *out_rgb, uint8_t *out_rgba8,
                                       float *out_variance) {
    const Split k(t);
    return temporal_accum(c, "vrt_accum_resolve_hdr_temporal_mom", k.tp, &k.m, f, tm, true, history_in, history_out, out_integrated, out_rgb,
                          out_rgba8, out_variance, nullptr);
}

int vrt_accum_resolve_hdr_temporal_mom_device(vrt_ctx *c, const vrt_temporal_mom *t, const vrt_filter_var *f, const vrt_tonemap *tm,
                                              const void *d_history_in, void *d_history_out, void *d_integrated, void *d_rgb, void *d_rgba8,
                                              void *d_variance_out, void *stream) {
    const Split k(t);
    return temporal_accum(c, "vrt_accum_resolve_hdr_temporal_mom_device", k.tp, &k.m, f, tm, false, d_history_in, d_history_out, d_integrated,
                          d_rgb, d_rgba8, d_variance_out, stream);
}

}  // extern "C"
