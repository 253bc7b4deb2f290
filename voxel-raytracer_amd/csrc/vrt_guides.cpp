// vrt_guides.cpp -- the guide planes (include/vrt.h vrt_accum_guides, vrt_guide_rays and their device forms): first-hit normal,
// albedo, depth and coverage. For an accumulation: the call-order checks, the guide state (made at the first call, 40 bytes per
// pixel), which samples it still lacks, their launch through the dispatcher -- enqueue() with an AccumStep whose `guides` is set, in
// VRT_MODE_PRIMARY, so the views, the lens selection, the variant and the frame block are those of the accumulation's own primary
// launches -- and the resolve. For ray batches: vrt_shade_rays's arguments and staging, one launch, no state. Neither touches the
// accumulation's sums. Guides past glass (vrt_set_guide_glass): the accumulation's launches take the rule its begin read
// (Accum::guide_glass), ray batches the context's at the call.
#include "vrt_stage.h"
#include "vrt_launch.h"

using namespace vrt_internal;

namespace {

using Accum = vrt_ctx::Accum;

// The guides of the samples the state does not hold yet, on the context's stream (which orders every use of the state)
int catch_up(vrt_ctx *c, const char *what) {
    Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    if (px > ac.guide_pixels) {
        const int r = reserve_synced(c, {{&ac.d_guides, px * vrt::guides::kStateBytes}});
        if (r) return r;
        ac.guide_pixels = px;
        ac.guide_total = 0;
        ac.guide_epoch = 0;   // no epoch: cleared below
    }
    if (ac.guide_epoch != ac.epoch) {   // the sums started again since (or this is the first call): so does the state
        VRT_HIP(c, hipMemsetAsync(ac.d_guides, 0, px * vrt::guides::kStateBytes, c->stream));   // +0.0, no hits
        ac.guide_epoch = ac.epoch;
        ac.guide_total = 0;
    }
    if (ac.guide_total >= ac.total) return VRT_OK;
    // the missing samples are marched with the context's inputs, which must still be those of the samples in the sums (the next
    // vrt_accum_add would restart): a camera, uniforms, tree or lens changed since the last add leaves nothing to march them with
    if (!accum_inputs_current(c))
        return vrt_fail(c, VRT_E_STATE, std::string(what) + ": camera, uniforms, tree or lens changed since the last vrt_accum_add");
    if (c->batch.open) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": a patch batch is open (call vrt_patch_end first)");
    AccumStep step{ac.first + ac.guide_total, ac.total - ac.guide_total, (ac.flags & VRT_ACCUM_JITTER) != 0u, ac.lens[0], ac.lens[1]};
    step.guides = true;
    step.glass = ac.guide_glass;
    const int r = enqueue(c, ac.width, ac.height, 0, ac.height, ac.height, 0, 0, VRT_MODE_PRIMARY, nullptr, nullptr, c->stream, nullptr, 1, &step);
    if (r) {   // what the launch left in the state is unknown
        ac.guide_epoch = 0;
        return r;
    }
    ac.guide_total = ac.total;
    return VRT_OK;
}

int resolve_into(vrt_ctx *c, float *d_normal, float *d_albedo, float *d_depth, float *d_coverage, hipStream_t s) {
    Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    if (!d_normal && !d_albedo && !d_depth && !d_coverage) return VRT_OK;
    const vrt::guides::Resolve q{vrt::guides::state_of(ac.d_guides.get(), px), d_normal, d_albedo, d_depth, d_coverage, ac.total, (uint32_t)px};
    VRT_HIP(c, vrt::launch::guides_resolve(q, s));
    return VRT_OK;
}

int check_rays(vrt_ctx *c, size_t n, const void *origins, int origin_stride, const void *dirs, bool any_out, const char *what) {
    if (!c) return VRT_E_INVALID;
    if (!c->have_scene) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": no octree uploaded (call vrt_upload_octree first)");
    if (c->batch.open) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": a patch batch is open (call vrt_patch_end first)");
    if (origin_stride != 0 && origin_stride != 3) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": origin_stride must be 0 or 3");
    if (n > ((size_t)1 << 30)) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": at most 2^30 rays per call");
    if (!any_out) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": every output is null");
    if (n > 0 && (!origins || !dirs)) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null buffer");
    return VRT_OK;
}

int guide_batch(vrt_ctx *c, size_t n, const float *d_origins, int origin_stride, const float *d_dirs, int width, float *d_normal, float *d_albedo,
                float *d_depth, uint8_t *d_hit, hipStream_t s) {
    const int ra = ensure_analysis(c);
    if (ra) return ra;
    const Variant v = base_variant(c);   // the launch reads its traversal only
    vrt::KArgs a;
    vrt::ViewSet vs;
    fill_ray_batch_args(c, n, width, a, vs);
    vrt::guides::RayArgs q{d_origins, d_dirs, d_normal, d_albedo, d_depth, d_hit, (uint32_t)n, origin_stride, (uint32_t)width, 0u};
    const uint32_t grid = vrt::rays::plan(q.n, q.width, q.tiles_x);
    const hipError_t e = vrt::launch::guide_rays(v, a, vs, q, c->guide_glass, grid, s);
    if (e != hipSuccess) return vrt_fail(c, VRT_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return VRT_OK;
}

// what vrt_guide_frame* check before anything is enqueued
int check_guide_frame(vrt_ctx *c, const char *what, int width, int height, bool any_out) {
    if (!c) return VRT_E_INVALID;
    const int r = check_frame(c, width, height);
    if (r) return r;
    if (!any_out) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": every output is null");
    return VRT_OK;
}

}  // namespace

// One sample per pixel -- sample 0 from the corner, the lens as vrt_accum_add would take it -- through the corner form of guide_kernel
// into the context's own state, then the guide resolve with n = 1: the launches of vrt_accum_begin_ex(PRIMARY, 0, 0), vrt_accum_add(1),
// vrt_accum_guides_device, with no accumulation involved.
int vrt_internal::guide_frame_planes(vrt_ctx *c, const char *what, int width, int height, bool glass, float *d_normal, float *d_albedo,
                                     float *d_depth, float *d_coverage, hipStream_t s) {
    if (!c->have_scene) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": no octree uploaded (call vrt_upload_octree first)");
    if (c->batch.open) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": a patch batch is open (call vrt_patch_end first)");
    if (!c->have_camera) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": no camera set (call vrt_set_camera first)");
    vrt_ctx::GuideFrame &gf = c->guide_frame;
    const size_t px = (size_t)width * (size_t)height;
    if (!gf.marched) VRT_HIP(c, hipEventCreateWithFlags(&gf.marched, hipEventDisableTiming));
    if (!gf.read) VRT_HIP(c, hipEventCreateWithFlags(&gf.read, hipEventDisableTiming));
    if (px * vrt::guides::kStateBytes > gf.d_state.bytes()) {
        const int r = reserve_synced(c, {{&gf.d_state, px * vrt::guides::kStateBytes}});
        if (r) return r;
    }
    VRT_HIP(c, hipMemsetAsync(gf.d_state.get(), 0, px * vrt::guides::kStateBytes, c->stream));   // +0.0, no hits
    AccumStep step{0u, 1u, false, c->lens[0], c->lens[1]};
    step.guides = true;
    step.glass = glass;
    step.guide_state = gf.d_state.get();
    int r = enqueue(c, width, height, 0, height, height, 0, 0, VRT_MODE_PRIMARY, nullptr, nullptr, c->stream, nullptr, 1, &step);
    if (r) return r;
    // the state is the context's, whose every use the context's stream orders: a caller's stream is joined back
    if (s != c->stream) {
        VRT_HIP(c, hipEventRecord(gf.marched, c->stream));
        VRT_HIP(c, hipStreamWaitEvent(s, gf.marched, 0));
    }
    const vrt::guides::Resolve q{vrt::guides::state_of(gf.d_state.get(), px), d_normal, d_albedo, d_depth, d_coverage, 1u, (uint32_t)px};
    VRT_HIP(c, vrt::launch::guides_resolve(q, s));
    if (s != c->stream) {
        VRT_HIP(c, hipEventRecord(gf.read, s));
        VRT_HIP(c, hipStreamWaitEvent(c->stream, gf.read, 0));
    }
    return VRT_OK;
}

extern "C" {

int vrt_guide_frame(vrt_ctx *c, int width, int height, float *out_normal, float *out_albedo, float *out_depth, float *out_coverage) {
    int r = check_guide_frame(c, "vrt_guide_frame", width, height, out_normal || out_albedo || out_depth || out_coverage);
    if (r) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    vrt_stage::Stage st(4);
    const int normal = st.out(px * 12, out_normal), albedo = st.out(px * 16, out_albedo), depth = st.out(px * 4, out_depth);
    const int coverage = st.out(px * 4, out_coverage);
    if ((r = st.reserve_synced(c, c->guide_frame.d_host))) return r;
    r = guide_frame_planes(c, "vrt_guide_frame", width, height, c->guide_glass, st.at<float>(normal), st.at<float>(albedo), st.at<float>(depth),
                           st.at<float>(coverage), c->stream);
    return r ? r : st.download(c, c->stream);
}

int vrt_guide_frame_device(vrt_ctx *c, int width, int height, void *d_normal, void *d_albedo, void *d_depth, void *d_coverage, void *stream) {
    const int r = check_guide_frame(c, "vrt_guide_frame_device", width, height, d_normal || d_albedo || d_depth || d_coverage);
    if (r) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    return guide_frame_planes(c, "vrt_guide_frame_device", width, height, c->guide_glass, static_cast<float *>(d_normal),
                              static_cast<float *>(d_albedo), static_cast<float *>(d_depth), static_cast<float *>(d_coverage),
                              stream ? (hipStream_t)stream : c->stream);
}

int vrt_accum_guides(vrt_ctx *c, float *out_normal, float *out_albedo, float *out_depth, float *out_coverage) {
    int r = accum_state(c, "vrt_accum_guides", false);
    if (r) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    Accum &ac = c->accum;
    const size_t px = (size_t)ac.width * (size_t)ac.height;
    if ((r = catch_up(c, "vrt_accum_guides"))) return r;
    vrt_stage::Stage st(4);
    const int normal = st.out(px * 12, out_normal), albedo = st.out(px * 16, out_albedo), depth = st.out(px * 4, out_depth);
    const int coverage = st.out(px * 4, out_coverage);
    if ((r = st.reserve_synced(c, ac.d_gout))) return r;
    r = resolve_into(c, st.at<float>(normal), st.at<float>(albedo), st.at<float>(depth), st.at<float>(coverage), c->stream);
    return r ? r : st.download(c, c->stream);
}

int vrt_accum_guides_device(vrt_ctx *c, void *d_normal, void *d_albedo, void *d_depth, void *d_coverage, void *stream) {
    int r = accum_state(c, "vrt_accum_guides_device", false);
    if (r) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    if ((r = catch_up(c, "vrt_accum_guides_device"))) return r;
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return accum_joined(c, s, [&] {
        return resolve_into(c, static_cast<float *>(d_normal), static_cast<float *>(d_albedo), static_cast<float *>(d_depth),
                            static_cast<float *>(d_coverage), s);
    });
}

int vrt_set_guide_glass(vrt_ctx *c, int on) {
    if (!c) return VRT_E_INVALID;
    if (on != 0 && on != 1) return vrt_fail(c, VRT_E_INVALID, "vrt_set_guide_glass: on must be 0 or 1");
    c->guide_glass = on == 1;
    return VRT_OK;
}

int vrt_guide_rays(vrt_ctx *c, size_t n, const float *origins, int origin_stride, const float *dirs, int width, float *out_normal,
                   float *out_albedo, float *out_depth, uint8_t *out_hit) {
    int r = check_rays(c, n, origins, origin_stride, dirs, out_normal || out_albedo || out_depth || out_hit, "vrt_guide_rays");
    if (r) return r;
    if (width < 1) return vrt_fail(c, VRT_E_INVALID, "vrt_guide_rays: width must be at least 1");
    if (n == 0) return VRT_OK;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt_stage::Stage st(256);
    const int o = st.in((origin_stride ? n : 1) * 3 * sizeof(float), origins), d = st.in(n * 3 * sizeof(float), dirs);
    const int normal = st.out(out_normal ? n * 12 : 0, out_normal), albedo = st.out(out_albedo ? n * 16 : 0, out_albedo);
    const int depth = st.out(out_depth ? n * 4 : 0, out_depth), hit = st.out(out_hit ? n : 0, out_hit);
    if ((r = st.reserve_staging(c, c->d_rays)) || (r = st.upload(c, c->stream))) return r;
    r = guide_batch(c, n, st.at<float>(o), origin_stride, st.at<float>(d), width, st.at<float>(normal), st.at<float>(albedo), st.at<float>(depth),
                    st.at<uint8_t>(hit), c->stream);
    return r ? r : st.download(c, c->stream);
}

int vrt_guide_rays_device(vrt_ctx *c, size_t n, const void *d_origins, int origin_stride, const void *d_dirs, int width, void *d_normal,
                          void *d_albedo, void *d_depth, void *d_hit, void *stream) {
    const int r = check_rays(c, n, d_origins, origin_stride, d_dirs, d_normal || d_albedo || d_depth || d_hit, "vrt_guide_rays_device");
    if (r) return r;
    if (width < 1) return vrt_fail(c, VRT_E_INVALID, "vrt_guide_rays_device: width must be at least 1");
    if (n == 0) return VRT_OK;
    VRT_HIP(c, hipSetDevice(c->device));
    return guide_batch(c, n, static_cast<const float *>(d_origins), origin_stride, static_cast<const float *>(d_dirs), width,
                       static_cast<float *>(d_normal), static_cast<float *>(d_albedo), static_cast<float *>(d_depth),
                       static_cast<uint8_t *>(d_hit), stream ? (hipStream_t)stream : c->stream);
}

}  // extern "C"
