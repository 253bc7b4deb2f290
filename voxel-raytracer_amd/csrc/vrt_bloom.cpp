// vrt_bloom.cpp -- bloom (include/vrt.h vrt_bloom_hdr, its host form and vrt_accum_resolve_hdr_bloomed*). Validation, the one launch
// seam (bloom_launch: the 2 L launches of a call), the host form staged around it, and the accumulation forms on the accumulation's own
// stage. The level sizes and the workspace's layout are vrt_bloom.h's, which vrt_bloom_workspace_bytes evaluates too. Host code; the
// kernels are behind vrt_launch.h. Nothing here reads context state or touches the accumulation's sums.
#include "vrt_stage.h"
#include "vrt_launch.h"

using namespace vrt_internal;
namespace bloom = vrt::bloom;

namespace {

constexpr float kHdrMax = 65504.0f;   // h(c)'s upper bound: no pixel is brighter, so no larger threshold or gain means anything

bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) == 0u; }

// The parameters a call runs with (NULL: vrt_bloom_default)
struct Params {
    vrt_bloom b;
    explicit Params(const vrt_bloom *p) {
        if (p) b = *p;
        else vrt_bloom_default(&b);
    }
};

// VRT_E_INVALID in the name of `what` unless b is one the header allows (every comparison is false for a NaN)
int check_params(vrt_ctx *c, const char *what, const vrt_bloom &b) {
    const std::string w(what);
    if (b.levels < 1 || b.levels > bloom::kMaxLevels) return vrt_fail(c, VRT_E_INVALID, w + ": levels must be in 1..VRT_BLOOM_MAX_LEVELS");
    if (b.flags & ~VRT_BLOOM_KARIS) return vrt_fail(c, VRT_E_INVALID, w + ": unknown flags");
    if (!(b.knee >= 0.0f && b.knee <= b.threshold && b.threshold <= kHdrMax))
        return vrt_fail(c, VRT_E_INVALID, w + ": threshold and knee must satisfy 0 <= knee <= threshold <= 65504");
    if (!(b.intensity >= 0.0f && b.intensity <= kHdrMax)) return vrt_fail(c, VRT_E_INVALID, w + ": intensity must be in [0, 65504]");
    return VRT_OK;
}

// what the device forms check of their pointers: `ins` (null entries: not given), the workspace (null: the call's own) and `outs`, of
// which one at least must be given; equal pointers alias
int check_pointers(vrt_ctx *c, const char *what, std::initializer_list<const void *> ins, const void *workspace,
                   std::initializer_list<const void *> outs) {
    const std::string w(what);
    if (workspace && !aligned(workspace, 16)) return vrt_fail(c, VRT_E_INVALID, w + ": the workspace must be a multiple of 16");
    for (const void *p : ins)
        if (p && !aligned(p, 4)) return vrt_fail(c, VRT_E_INVALID, w + ": every device pointer must be a multiple of 4");
    bool any = false;
    for (auto o = outs.begin(); o != outs.end(); ++o) {
        if (!*o) continue;
        any = true;
        if (!aligned(*o, 4)) return vrt_fail(c, VRT_E_INVALID, w + ": every device pointer must be a multiple of 4");
        for (const void *p : ins)
            if (*o == p) return vrt_fail(c, VRT_E_INVALID, w + ": an output must not alias an input");
        if (*o == workspace) return vrt_fail(c, VRT_E_INVALID, w + ": an output must not alias the workspace");
        for (auto o2 = outs.begin(); o2 != o; ++o2)
            if (*o == *o2) return vrt_fail(c, VRT_E_INVALID, w + ": the outputs must not alias each other");
    }
    if (!any) return vrt_fail(c, VRT_E_INVALID, w + ": one of the two outputs must be given");
    return VRT_OK;
}

// B0-B8 on device memory, stream-ordered: levels down-sampling launches, levels - 1 steps of the chain, the composite. b, tm and the
// frame: checked. d_exposure, d_out_rgb, d_out_rgba8: each may be null.
int bloom_launch(vrt_ctx *c, int width, int height, const void *d_rgb, const vrt_bloom &b, const vrt_tonemap *tm, const void *d_exposure,
                 void *d_workspace, void *d_out_rgb, void *d_out_rgba8, hipStream_t s) {
    bloom::Pyramid p;
    if (!bloom::pyramid(width, height, b.levels, p)) return vrt_fail(c, VRT_E_INVALID, "bloom: no pyramid for this frame");
    const auto level = [&](int l) { return reinterpret_cast<float *>(static_cast<char *>(d_workspace) + p.offset[l]); };
    const float exposure = tm ? tm->exposure : 1.0f;
    const bool karis = (b.flags & VRT_BLOOM_KARIS) != 0u;
    for (int l = 1; l <= p.levels; ++l) {
        bloom::DownArgs q{};
        q.rgb = l == 1 ? static_cast<const float *>(d_rgb) : nullptr;
        q.src = l == 1 ? nullptr : level(l - 1);
        q.dst = level(l);
        q.sw = p.w[l - 1];
        q.sh = p.h[l - 1];
        q.dw = p.w[l];
        q.dh = p.h[l];
        q.bright = bloom::Bright{static_cast<const vrt_exposure *>(d_exposure), exposure, b.threshold, b.knee};
        VRT_HIP(c, vrt::launch::bloom_down(q, l == 1, karis, s));
    }
    for (int l = p.levels - 1; l >= 0; --l) {   // l == 0: the composite
        bloom::UpArgs q{};
        q.src = level(l + 1);
        q.sw = p.w[l + 1];
        q.sh = p.h[l + 1];
        q.dw = p.w[l];
        q.dh = p.h[l];
        if (l > 0) {
            q.dst = level(l);
        } else {
            q.rgb = static_cast<const float *>(d_rgb);
            q.out_rgb = static_cast<float *>(d_out_rgb);
            q.out_rgba = static_cast<uint32_t *>(d_out_rgba8);
            q.record = static_cast<const vrt_exposure *>(d_exposure);
            q.exposure = exposure;
            q.op = tm ? tm->op : VRT_TONEMAP_CLAMP;
            q.intensity = b.intensity;
            q.inv_levels = 1.0f / (float)p.levels;
        }
        VRT_HIP(c, vrt::launch::bloom_up(q, l == 0, s));
    }
    return VRT_OK;
}

// The accumulation forms. to_host: record, f and bytes are the caller's host buffers, filled on the context's stream before the
// return; else device memory, written in the order of `stream`. record null: no metering and no record.
int bloom_accum(vrt_ctx *c, const char *what, const vrt_meter *m, Params k, const vrt_tonemap *tm, bool to_host, void *record, void *out_rgb,
                void *out_rgba8, void *stream) {
    int r = accum_state(c, what, true);   // vrt_accum_resolve_hdr's call-order checks
    if (r) return r;
    if ((r = check_params(c, what, k.b)) || (r = check_tonemap(c, what, tm))) return r;
    vrt_ctx::Accum &ac = c->accum;
    if (to_host) {
        if (!out_rgb && !out_rgba8) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": one of the two outputs must be given");
    } else if ((r = check_pointers(c, what, {record}, nullptr, {out_rgb, out_rgba8}))) {
        return r;
    }
    if (record) {
        // vrt_meter_hdr's own checks of m, before anything is enqueued: its rule on an empty histogram, and the rectangle in this frame
        const uint32_t none[VRT_METER_BINS] = {};
        vrt_exposure scratch{};
        const bool whole = !m || (m->x0 == 0 && m->y0 == 0 && m->x1 == 0 && m->y1 == 0);
        if (vrt_meter_resolve(none, m, &scratch) != VRT_OK ||
            !(whole || (m->x0 >= 0 && m->x0 < m->x1 && m->x1 <= ac.width && m->y0 >= 0 && m->y0 < m->y1 && m->y1 <= ac.height)))
            return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": a vrt_meter that vrt_meter_hdr refuses for this frame");
    }
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    // the accumulation's stage: the mean, the histogram, the record, the pyramid, f, the bytes
    vrt_stage::Stage st(16, to_host);
    const int mean = st.kept(px * 12), hist = st.kept(VRT_METER_BINS * sizeof(uint32_t)), rec = st.kept(sizeof(vrt_exposure), record);
    const int ws = st.kept(vrt_bloom_workspace_bytes(ac.width, ac.height, k.b.levels));
    const int f = st.out(px * 12, out_rgb), bytes = st.out(px * 4, out_rgba8);
    if ((r = st.reserve_synced(c, ac.d_filter))) return r;
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (to_host && record) VRT_HIP(c, hipMemcpyAsync(st.at(rec), record, sizeof(vrt_exposure), hipMemcpyHostToDevice, s));   // in and out
    if ((r = vrt_accum_resolve_hdr_device(c, st.at(mean), tm, nullptr, nullptr, s))) return r;
    // the stage belongs to the accumulation, whose every use the context's stream orders: a caller's stream is joined back
    void *const d_rec = record ? st.at(rec) : nullptr;
    r = accum_joined(c, s, [&] {
        const int e = d_rec ? vrt_meter_hdr(c, ac.width, ac.height, st.at(mean), m, st.at(hist), d_rec, s) : VRT_OK;
        return e ? e : bloom_launch(c, ac.width, ac.height, st.at(mean), k.b, tm, d_rec, st.at(ws), st.at(f), st.at(bytes), s);
    });
    return r ? r : st.download(c, c->stream);
}

}  // namespace

extern "C" {

void vrt_bloom_default(vrt_bloom *b) {
    if (!b) return;
    b->levels = 5;
    b->flags = VRT_BLOOM_KARIS;
    b->threshold = 1.0f;
    b->knee = 0.5f;
    b->intensity = 0.2f;
}

size_t vrt_bloom_workspace_bytes(int width, int height, int levels) {
    bloom::Pyramid p;
    return bloom::pyramid(width, height, levels, p) ? p.bytes : 0u;
}

int vrt_bloom_hdr(vrt_ctx *c, int width, int height, const void *d_rgb, const vrt_bloom *b, const vrt_tonemap *tm, const void *d_exposure,
                  void *d_workspace, void *d_out_rgb, void *d_out_rgba8, void *stream) {
    if (!c) return VRT_E_INVALID;
    const char *what = "vrt_bloom_hdr";
    const Params k(b);
    if (!d_rgb || !d_workspace) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null pointer");
    int r = check_pointers(c, what, {d_rgb, d_exposure}, d_workspace, {d_out_rgb, d_out_rgba8});
    if (r || (r = check_frame(c, width, height)) || (r = check_params(c, what, k.b)) || (r = check_tonemap(c, what, tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    return bloom_launch(c, width, height, d_rgb, k.b, tm, d_exposure, d_workspace, d_out_rgb, d_out_rgba8, stream ? (hipStream_t)stream : c->stream);
}

int vrt_bloom_hdr_host(vrt_ctx *c, int width, int height, const float *rgb, const vrt_bloom *b, const vrt_tonemap *tm, const vrt_exposure *e,
                       float *out_rgb, uint8_t *out_rgba8) {
    if (!c) return VRT_E_INVALID;
    const char *what = "vrt_bloom_hdr_host";
    const Params k(b);
    if (!rgb) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null pointer");
    if (!out_rgb && !out_rgba8) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": one of the two outputs must be given");
    int r = check_frame(c, width, height);
    if (r || (r = check_params(c, what, k.b)) || (r = check_tonemap(c, what, tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    vrt_stage::Stage st(16);
    const int in = st.in(px * 12, rgb), rec = st.in(sizeof(vrt_exposure), e);
    const int ws = st.kept(vrt_bloom_workspace_bytes(width, height, k.b.levels));
    const int f = st.out(px * 12, out_rgb), bytes = st.out(px * 4, out_rgba8);
    if ((r = st.reserve_synced(c, c->d_bloom)) || (r = st.upload(c, c->stream))) return r;
    if ((r = bloom_launch(c, width, height, st.at(in), k.b, tm, st.at(rec), st.at(ws), st.at(f), st.at(bytes), c->stream))) return r;
    return st.download(c, c->stream);
}

int vrt_accum_resolve_hdr_bloomed(vrt_ctx *c, const vrt_meter *m, const vrt_bloom *b, const vrt_tonemap *tm, vrt_exposure *io, float *out_rgb,
                                  uint8_t *out_rgba8) {
    return bloom_accum(c, "vrt_accum_resolve_hdr_bloomed", m, Params(b), tm, true, io, out_rgb, out_rgba8, nullptr);
}

int vrt_accum_resolve_hdr_bloomed_device(vrt_ctx *c, const vrt_meter *m, const vrt_bloom *b, const vrt_tonemap *tm, void *d_exposure, void *d_rgb,
                                         void *d_rgba8, void *stream) {
    return bloom_accum(c, "vrt_accum_resolve_hdr_bloomed_device", m, Params(b), tm, false, d_exposure, d_rgb, d_rgba8, stream);
}

}  // extern "C"
