// vrt_temporal.cpp -- the temporal pass (include/vrt.h vrt_temporal_hdr, its host form and the accumulation forms that chain it with
// vrt_filter_hdr_var). One route serves all four (temporal_frame): validation and the one launch; it reads no context state and
// keeps no scratch. One helper stages host planes and histories around it (vrt_temporal_hdr_host), one brings an HDR accumulation's
// float mean and its own guide planes into the accumulation's filter stage, runs the pass on them with the context's current camera
// block and the variance-guided filter on what it returns (temporal_accum). Host code; the kernel is behind vrt_launch.h. Nothing
// here touches the accumulation's sums.
#include "vrt_internal.h"
#include "vrt_launch.h"

#include <cmath>
#include <cstring>

using namespace vrt_internal;

namespace {

constexpr size_t kHistory = vrt::temporal::kHistoryBytes;
// the staging of the host form: both histories, rgb, normal, depth, coverage, the integrated image and the variance
constexpr size_t kHostStageBytes = 2 * kHistory + 12 + 12 + 4 + 4 + 12 + 4;
// the accumulation's stage: mean 3, normal 3, albedo 4, depth, coverage, integrated 3, variance, out_rgb 3, out_rgba8, out_variance
constexpr size_t kAccumStageFloats = 21;

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
};

// VRT_E_INVALID in the name of `what` unless t is one the header allows; the previous camera only where a history comes in
int check_params(vrt_ctx *c, const char *what, const vrt_temporal *t, bool have_history) {
    const std::string w(what);
    if (!t) return vrt_fail(c, VRT_E_INVALID, w + ": null vrt_temporal");
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
    const void *const ins[5] = {io.rgb, io.normal, io.depth, io.coverage, io.history_in};
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

// The stateless pass on device planes, stream-ordered, in the name of `what`
int temporal_frame(vrt_ctx *c, const char *what, int width, int height, const float *inv_proj, const float *inv_view, const float *cam_pos,
                   const Io &d, const vrt_temporal *t, hipStream_t s) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if ((r = check_io(c, what, d, true))) return r;
    if ((r = check_params(c, what, t, d.history_in != nullptr))) return r;
    if ((r = check_camera(c, what, inv_proj, inv_view, cam_pos))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt::temporal::Args q{};
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
    VRT_HIP(c, vrt::launch::temporal_pass(q, s));
    return VRT_OK;
}

inline size_t align16(size_t b) { return (b + 15u) & ~(size_t)15u; }

// The accumulation forms: mean and planes into the accumulation's stage, the pass on them, the filter on its outputs. to_host: the
// histories and the outputs are the caller's host buffers, staged behind the stage's planes and filled on the context's stream
// before the return; else device memory, read and written in the order of `stream`.
int temporal_accum(vrt_ctx *c, const char *what, const vrt_temporal *t, const vrt_filter_var *f, const vrt_tonemap *tm, bool to_host,
                   const void *history_in, void *history_out, void *out_integrated, void *out_rgb, void *out_rgba8, void *out_variance,
                   void *stream) {
    if (!c) return VRT_E_INVALID;
    // the call-order checks: those of vrt_accum_guides, then vrt_accum_resolve_hdr's
    if (!c->accum.begun) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": no accumulation (call vrt_accum_begin first)");
    if (c->accum.total == 0) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": the accumulation holds no samples (call vrt_accum_add first)");
    if (!c->accum.hdr) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": the accumulation keeps no HDR sums (vrt_accum_keep_hdr before the begin)");
    if (!history_out) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null history_out");
    if (history_out == history_in) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": history_out must differ from history_in");
    int r = check_params(c, what, t, history_in != nullptr);
    if (r) return r;
    if ((r = filter_var_check(c, what, f, tm, out_rgb, out_rgba8))) return r;
    if ((r = check_camera(c, what, c->inv_proj, c->inv_view, c->cam_pos))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt_ctx::Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    const size_t plane_bytes = px * kAccumStageFloats * sizeof(float);
    const size_t bytes = to_host ? align16(plane_bytes) + 2 * px * kHistory : plane_bytes;
    if (bytes > ac.d_filter.bytes() && (r = reserve_synced(c, {{&ac.d_filter, bytes}}))) return r;
    float *const base = ac.d_filter;
    float *const mean = base, *const normal = base + px * 3, *const albedo = base + px * 6, *const depth = base + px * 10,
                 *const coverage = base + px * 11, *const st_integ = base + px * 12, *const variance = base + px * 15,
                 *const st_rgb = base + px * 16, *const st_rgba = base + px * 19, *const st_var = base + px * 20;
    char *const st_hin = reinterpret_cast<char *>(base) + align16(plane_bytes), *const st_hout = st_hin + px * kHistory;
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((r = vrt_accum_guides_device(c, normal, albedo, depth, coverage, s))) return r;   // brings the guide state up to date first
    if ((r = vrt_accum_resolve_hdr_device(c, mean, tm, nullptr, nullptr, s))) return r;
    vrt_temporal tt = *t;
    tt.offset_x = tt.offset_y = (ac.flags & VRT_ACCUM_JITTER) ? 0.5f : 0.0f;
    Io d{mean, normal, depth, coverage, history_in, history_out, out_integrated ? out_integrated : st_integ, variance};
    void *f_rgb = out_rgb, *f_rgba = out_rgba8, *f_var = out_variance;
    if (to_host) {
        if (history_in) VRT_HIP(c, hipMemcpyAsync(st_hin, history_in, px * kHistory, hipMemcpyHostToDevice, s));
        d.history_in = history_in ? st_hin : nullptr;
        d.history_out = st_hout;
        d.out_rgb = st_integ;
        f_rgb = out_rgb ? st_rgb : nullptr;
        f_rgba = out_rgba8 ? st_rgba : nullptr;
        f_var = out_variance ? st_var : nullptr;
    }
    // the stage belongs to the accumulation, whose every use the context's stream orders: a caller's stream is joined back
    r = accum_joined(c, s, [&] {
        const int rt = temporal_frame(c, what, ac.width, ac.height, c->inv_proj, c->inv_view, c->cam_pos, d, &tt, s);
        if (rt) return rt;
        return filter_var_frame(c, what, ac.width, ac.height, d.out_rgb, normal, albedo, depth, coverage, variance, f, tm, f_rgb, f_rgba, f_var, s);
    });
    if (r || !to_host) return r;
    VRT_HIP(c, hipMemcpyAsync(history_out, st_hout, px * kHistory, hipMemcpyDeviceToHost, c->stream));
    if (out_integrated) VRT_HIP(c, hipMemcpyAsync(out_integrated, st_integ, px * 12, hipMemcpyDeviceToHost, c->stream));
    if (out_rgb) VRT_HIP(c, hipMemcpyAsync(out_rgb, st_rgb, px * 12, hipMemcpyDeviceToHost, c->stream));
    if (out_rgba8) VRT_HIP(c, hipMemcpyAsync(out_rgba8, st_rgba, px * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_variance) VRT_HIP(c, hipMemcpyAsync(out_variance, st_var, px * 4, hipMemcpyDeviceToHost, c->stream));
    VRT_HIP(c, hipStreamSynchronize(c->stream));
    return VRT_OK;
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
    return temporal_frame(c, "vrt_temporal_hdr", width, height, inv_projection, inv_view, camera_pos, d, t, stream ? (hipStream_t)stream : c->stream);
}

int vrt_temporal_hdr_host(vrt_ctx *c, int width, int height, const float inv_projection[16], const float inv_view[16], const float camera_pos[4],
                          const float *rgb, const float *normal, const float *depth, const float *coverage, const void *history_in,
                          const vrt_temporal *t, void *history_out, float *out_rgb, float *out_variance) {
    const char *what = "vrt_temporal_hdr_host";
    int r = check_frame(c, width, height);
    if (r) return r;
    const Io h{rgb, normal, depth, coverage, history_in, history_out, out_rgb, out_variance};
    if ((r = check_io(c, what, h, false))) return r;
    if (history_out == history_in) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": history_out must differ from history_in");
    if ((r = check_params(c, what, t, history_in != nullptr))) return r;
    if ((r = check_camera(c, what, inv_projection, inv_view, camera_pos))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    if (px * kHostStageBytes > c->d_temporal.bytes() && (r = reserve_synced(c, {{&c->d_temporal, px * kHostStageBytes}}))) return r;
    char *const base = reinterpret_cast<char *>(c->d_temporal.get());
    char *const st_hin = base, *const st_hout = base + px * kHistory;
    float *const st_rgb = reinterpret_cast<float *>(base + 2 * px * kHistory), *const st_normal = st_rgb + px * 3, *const st_depth = st_rgb + px * 6,
                 *const st_cov = st_rgb + px * 7, *const st_out = st_rgb + px * 8, *const st_var = st_rgb + px * 11;
    if (history_in) VRT_HIP(c, hipMemcpyAsync(st_hin, history_in, px * kHistory, hipMemcpyHostToDevice, c->stream));
    VRT_HIP(c, hipMemcpyAsync(st_rgb, rgb, px * 12, hipMemcpyHostToDevice, c->stream));
    VRT_HIP(c, hipMemcpyAsync(st_normal, normal, px * 12, hipMemcpyHostToDevice, c->stream));
    VRT_HIP(c, hipMemcpyAsync(st_depth, depth, px * 4, hipMemcpyHostToDevice, c->stream));
    VRT_HIP(c, hipMemcpyAsync(st_cov, coverage, px * 4, hipMemcpyHostToDevice, c->stream));
    const Io d{st_rgb, st_normal, st_depth, st_cov, history_in ? st_hin : nullptr, st_hout, out_rgb ? st_out : nullptr, out_variance ? st_var : nullptr};
    if ((r = temporal_frame(c, what, width, height, inv_projection, inv_view, camera_pos, d, t, c->stream))) return r;
    VRT_HIP(c, hipMemcpyAsync(history_out, st_hout, px * kHistory, hipMemcpyDeviceToHost, c->stream));
    if (out_rgb) VRT_HIP(c, hipMemcpyAsync(out_rgb, st_out, px * 12, hipMemcpyDeviceToHost, c->stream));
    if (out_variance) VRT_HIP(c, hipMemcpyAsync(out_variance, st_var, px * 4, hipMemcpyDeviceToHost, c->stream));
    VRT_HIP(c, hipStreamSynchronize(c->stream));
    return VRT_OK;
}

int vrt_accum_resolve_hdr_temporal(vrt_ctx *c, const vrt_temporal *t, const vrt_filter_var *f, const vrt_tonemap *tm, const void *history_in,
                                   void *history_out, float *out_integrated, float *out_rgb, uint8_t *out_rgba8, float *out_variance) {
    return temporal_accum(c, "vrt_accum_resolve_hdr_temporal", t, f, tm, true, history_in, history_out, out_integrated, out_rgb, out_rgba8,
                          out_variance, nullptr);
}

int vrt_accum_resolve_hdr_temporal_device(vrt_ctx *c, const vrt_temporal *t, const vrt_filter_var *f, const vrt_tonemap *tm,
                                          const void *d_history_in, void *d_history_out, void *d_integrated, void *d_rgb, void *d_rgba8,
                                          void *d_variance_out, void *stream) {
    return temporal_accum(c, "vrt_accum_resolve_hdr_temporal_device", t, f, tm, false, d_history_in, d_history_out, d_integrated, d_rgb, d_rgba8,
                          d_variance_out, stream);
}

}  // extern "C"
