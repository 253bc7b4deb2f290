// vrt_meter.cpp -- auto-exposure (include/vrt.h vrt_meter_hdr, vrt_tonemap_hdr, their host forms, vrt_accum_resolve_hdr_metered*
// and the host's vrt_meter_resolve). Validation, the one launch seam of each pass (meter_launch: the memset, the histogram pass, the
// finishing step; tone_launch), the host forms staged around them, and the accumulation forms on the accumulation's own stage. The
// rule E4-E8 is vrt_meter.h's, which the finishing kernel evaluates too. Host code; the kernels are behind vrt_launch.h. Nothing
// here reads context state or touches the accumulation's sums.
#include "vrt_stage.h"
#include "vrt_launch.h"

using namespace vrt_internal;
namespace meter = vrt::meter;

namespace {

bool finite_positive(float v) { return v > 0.0f && v <= 3.402823466e38f; }   // false for NaN
bool aligned4(const void *p) { return ((uintptr_t)p & 3u) == 0u; }

// The parameters a call runs with (NULL: vrt_meter_default)
struct Params {
    vrt_meter m;
    explicit Params(const vrt_meter *p) {
        if (p) m = *p;
        else vrt_meter_default(&m);
    }
};

// VRT_E_INVALID in the name of `what` unless m is one the header allows. Needs no device (c may be null: vrt_meter_resolve).
int check_params(vrt_ctx *c, const char *what, const vrt_meter &m) {
    const std::string w(what);
    if (!finite_positive(m.key)) return vrt_fail(c, VRT_E_INVALID, w + ": key must be finite and > 0");
    if (!(m.low_permille >= 0 && m.low_permille < m.high_permille && m.high_permille <= 1000))
        return vrt_fail(c, VRT_E_INVALID, w + ": the rank window must be 0 <= low_permille < high_permille <= 1000");
    if (!finite_positive(m.min_exposure) || !finite_positive(m.max_exposure) || !(m.min_exposure <= m.max_exposure))
        return vrt_fail(c, VRT_E_INVALID, w + ": min_exposure and max_exposure must be finite with 0 < min_exposure <= max_exposure");
    if (!(m.adapt > 0.0f && m.adapt <= 1.0f)) return vrt_fail(c, VRT_E_INVALID, w + ": adapt must be in (0, 1]");
    return VRT_OK;
}

// ... and its rectangle in a width x height frame; all four 0: the whole frame, which this writes into m
int check_rect(vrt_ctx *c, const char *what, int width, int height, vrt_meter &m) {
    if (m.x0 == 0 && m.y0 == 0 && m.x1 == 0 && m.y1 == 0) {
        m.x1 = width;
        m.y1 = height;
        return VRT_OK;
    }
    if (!(m.x0 >= 0 && m.x0 < m.x1 && m.x1 <= width && m.y0 >= 0 && m.y0 < m.y1 && m.y1 <= height))
        return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": the rectangle must be all zeros or 0 <= x0 < x1 <= width, 0 <= y0 < y1 <= height");
    return VRT_OK;
}

// what the device forms check of their pointers: `ins` and `outs` (null entries of outs: not given), equal pointers alias
int check_pointers(vrt_ctx *c, const char *what, std::initializer_list<const void *> ins, std::initializer_list<const void *> outs) {
    const std::string w(what);
    for (const void *p : ins)
        if (p && !aligned4(p)) return vrt_fail(c, VRT_E_INVALID, w + ": every device pointer must be a multiple of 4");
    for (auto o = outs.begin(); o != outs.end(); ++o) {
        if (!*o) continue;
        if (!aligned4(*o)) return vrt_fail(c, VRT_E_INVALID, w + ": every device pointer must be a multiple of 4");
        for (const void *p : ins)
            if (*o == p) return vrt_fail(c, VRT_E_INVALID, w + ": an output must not alias an input");
        for (auto o2 = outs.begin(); o2 != o; ++o2)
            if (*o == *o2) return vrt_fail(c, VRT_E_INVALID, w + ": the outputs must not alias each other");
    }
    return VRT_OK;
}

// E1-E8 on device memory, stream-ordered: the histogram zeroed, the pass over m's rectangle (checked, filled in), the finishing step
int meter_launch(vrt_ctx *c, int width, const void *d_rgb, const vrt_meter &m, void *d_histogram, void *d_exposure, hipStream_t s) {
    meter::HistArgs q{};
    q.rgb = static_cast<const float *>(d_rgb);
    q.histogram = static_cast<uint32_t *>(d_histogram);
    const uint32_t w = (uint32_t)(m.x1 - m.x0), h = (uint32_t)(m.y1 - m.y0);
    q.first = (uint32_t)m.y0 * (uint32_t)width + (uint32_t)m.x0;
    q.stride = (uint32_t)width;
    if (w == (uint32_t)width) {   // whole rows: one run of pixels
        q.len = w * h;
        q.rows = 1u;
    } else {
        q.len = w;
        q.rows = h;
    }
    // pixel p lies at d_rgb + 12 p: a multiple of 16 exactly when p = (d_rgb / 4) mod 4
    q.phase = (4u - (uint32_t)(((uintptr_t)d_rgb >> 2) & 3u)) & 3u;
    VRT_HIP(c, hipMemsetAsync(d_histogram, 0, meter::kBins * sizeof(uint32_t), s));
    VRT_HIP(c, vrt::launch::meter_histogram(q, s));
    meter::FinishArgs f{};
    f.histogram = q.histogram;
    f.record = static_cast<vrt_exposure *>(d_exposure);
    f.m = m;
    VRT_HIP(c, vrt::launch::meter_finish(f, s));
    return VRT_OK;
}

// E9 on device memory; tm: checked
int tone_launch(vrt_ctx *c, size_t n, const void *d_rgb, const vrt_tonemap *tm, const void *d_exposure, void *d_out, hipStream_t s) {
    meter::ToneArgs q{};
    q.rgb = static_cast<const float *>(d_rgb);
    q.record = static_cast<const vrt_exposure *>(d_exposure);
    q.out_rgba = static_cast<uint32_t *>(d_out);
    q.n = n;
    q.op = tm ? tm->op : VRT_TONEMAP_CLAMP;
    q.exposure = tm ? tm->exposure : 1.0f;
    const bool vec = (((uintptr_t)d_rgb | (uintptr_t)d_out) & 15u) == 0u;
    VRT_HIP(c, vrt::launch::meter_tonemap(q, vec, s));
    return VRT_OK;
}

int check_count(vrt_ctx *c, const char *what, size_t n) {
    if (n < 1u || n > meter::kMaxPixels) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": n must be in 1..2^30");
    return VRT_OK;
}

// The accumulation forms. to_host: record, histogram, mean and bytes are the caller's host buffers, filled on the context's stream
// before the return; else device memory, written in the order of `stream`.
int meter_accum(vrt_ctx *c, const char *what, Params k, const vrt_tonemap *tm, bool to_host, void *record, void *histogram, void *out_rgb,
                void *out_rgba8, void *stream) {
    int r = accum_state(c, what, true);   // vrt_accum_resolve_hdr's call-order checks
    if (r) return r;
    if (!record) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null exposure record");
    if ((r = check_params(c, what, k.m)) || (r = check_tonemap(c, what, tm))) return r;
    vrt_ctx::Accum &ac = c->accum;
    if ((r = check_rect(c, what, ac.width, ac.height, k.m))) return r;
    if (!to_host && (r = check_pointers(c, what, {}, {record, histogram, out_rgb, out_rgba8}))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    // the accumulation's stage: the mean, the histogram, the record, the bytes
    vrt_stage::Stage st(16, to_host);
    const int mean = st.kept(px * 12, out_rgb), hist = st.kept(meter::kBins * sizeof(uint32_t), histogram);
    const int rec = st.kept(sizeof(vrt_exposure), record), bytes = st.kept(px * 4, out_rgba8);
    if ((r = st.reserve_synced(c, ac.d_filter))) return r;
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (to_host) VRT_HIP(c, hipMemcpyAsync(st.at(rec), record, sizeof(vrt_exposure), hipMemcpyHostToDevice, s));   // in and out: the stage only brings it back
    if ((r = vrt_accum_resolve_hdr_device(c, st.at(mean), tm, nullptr, nullptr, s))) return r;
    // the stage belongs to the accumulation, whose every use the context's stream orders: a caller's stream is joined back
    r = accum_joined(c, s, [&] {
        const int e = meter_launch(c, ac.width, st.at(mean), k.m, st.at(hist), st.at(rec), s);
        return e ? e : tone_launch(c, px, st.at(mean), tm, st.at(rec), st.at(bytes), s);
    });
    return r ? r : st.download(c, c->stream);
}

}  // namespace

extern "C" {

void vrt_meter_default(vrt_meter *m) {
    if (!m) return;
    m->key = 0.18f;
    m->low_permille = 500;
    m->high_permille = 950;
    m->min_exposure = 0x1p-10f;
    m->max_exposure = 0x1p10f;
    m->adapt = 1.0f;
    m->x0 = m->y0 = m->x1 = m->y1 = 0;
}

int vrt_meter_resolve(const uint32_t *histogram, const vrt_meter *m, vrt_exposure *io) {
    if (!histogram || !io) return VRT_E_INVALID;
    const Params k(m);
    if (check_params(nullptr, "vrt_meter_resolve", k.m)) return VRT_E_INVALID;
    return meter::resolve(histogram, k.m, *io) ? VRT_OK : VRT_E_INVALID;
}

int vrt_meter_hdr(vrt_ctx *c, int width, int height, const void *d_rgb, const vrt_meter *m, void *d_histogram, void *d_exposure,
                  void *stream) {
    if (!c) return VRT_E_INVALID;
    const char *what = "vrt_meter_hdr";
    Params k(m);
    if (!d_rgb || !d_histogram || !d_exposure) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null pointer");
    int r = check_pointers(c, what, {d_rgb}, {d_histogram, d_exposure});
    if (r || (r = check_params(c, what, k.m)) || (r = check_frame(c, width, height)) || (r = check_rect(c, what, width, height, k.m))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    return meter_launch(c, width, d_rgb, k.m, d_histogram, d_exposure, stream ? (hipStream_t)stream : c->stream);
}

int vrt_meter_hdr_host(vrt_ctx *c, int width, int height, const float *rgb, const vrt_meter *m, uint32_t *out_histogram, vrt_exposure *io) {
    if (!c) return VRT_E_INVALID;
    const char *what = "vrt_meter_hdr_host";
    Params k(m);
    if (!rgb || !io) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null pointer");
    int r = check_params(c, what, k.m);
    if (r || (r = check_frame(c, width, height)) || (r = check_rect(c, what, width, height, k.m))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    vrt_stage::Stage st(16);
    const int in = st.in(px * 12, rgb), rec_in = st.in(sizeof(vrt_exposure), io);
    const int hist = st.kept(meter::kBins * sizeof(uint32_t), out_histogram);
    if ((r = st.reserve_synced(c, c->d_meter)) || (r = st.upload(c, c->stream))) return r;
    st.out(sizeof(vrt_exposure), io, st.device(rec_in));   // the record goes back from where it came up
    if ((r = meter_launch(c, width, st.at(in), k.m, st.at(hist), st.at(rec_in), c->stream))) return r;
    return st.download(c, c->stream);
}

int vrt_tonemap_hdr(vrt_ctx *c, size_t n, const void *d_rgb, const vrt_tonemap *tm, const void *d_exposure, void *d_out_rgba8, void *stream) {
    if (!c) return VRT_E_INVALID;
    const char *what = "vrt_tonemap_hdr";
    if (!d_rgb || !d_out_rgba8) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null pointer");
    int r = check_pointers(c, what, {d_rgb, d_exposure}, {d_out_rgba8});
    if (r || (r = check_count(c, what, n)) || (r = check_tonemap(c, what, tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    return tone_launch(c, n, d_rgb, tm, d_exposure, d_out_rgba8, stream ? (hipStream_t)stream : c->stream);
}

int vrt_tonemap_hdr_host(vrt_ctx *c, size_t n, const float *rgb, const vrt_tonemap *tm, const vrt_exposure *e, uint8_t *out_rgba8) {
    if (!c) return VRT_E_INVALID;
    const char *what = "vrt_tonemap_hdr_host";
    if (!rgb || !out_rgba8) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null pointer");
    int r = check_count(c, what, n);
    if (r || (r = check_tonemap(c, what, tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt_stage::Stage st(16);
    const int in = st.in(n * 12, rgb), rec = st.in(sizeof(vrt_exposure), e), out = st.out(n * 4, out_rgba8);
    if ((r = st.reserve_synced(c, c->d_meter)) || (r = st.upload(c, c->stream))) return r;
    if ((r = tone_launch(c, n, st.at(in), tm, st.at(rec), st.at(out), c->stream))) return r;
    return st.download(c, c->stream);
}

int vrt_accum_resolve_hdr_metered(vrt_ctx *c, const vrt_meter *m, const vrt_tonemap *tm, vrt_exposure *io, float *out_rgb, uint8_t *out_rgba8,
                                  uint32_t *out_histogram) {
    return meter_accum(c, "vrt_accum_resolve_hdr_metered", Params(m), tm, true, io, out_histogram, out_rgb, out_rgba8, nullptr);
}

int vrt_accum_resolve_hdr_metered_device(vrt_ctx *c, const vrt_meter *m, const vrt_tonemap *tm, void *d_exposure, void *d_histogram, void *d_rgb,
                                         void *d_rgba8, void *stream) {
    return meter_accum(c, "vrt_accum_resolve_hdr_metered_device", Params(m), tm, false, d_exposure, d_histogram, d_rgb, d_rgba8, stream);
}

}  // extern "C"
