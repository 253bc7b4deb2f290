// vrt_display.cpp -- the display pass that consumes the two images in the reference's frame loop (the fullscreen quad drawn by
// src/main.cpp:951-967 with shaders/quad.frag:22-83) and the fused frame call. Host code; the kernel is behind vrt_launch.h.
#include "vrt_stage.h"

#include <cmath>
#include <cstdio>
#include <new>

using namespace vrt_internal;
#include "vrt_launch.h"

namespace {

// One launch of the display pass under the trace kernel's feedback scheduling (one tile = one workgroup here), keyed as mode `key`:
// the byte pass is kSchedDenoise, the HDR pass kSchedDenoiseHdr -- a state of its own, so neither pass moves the other's launch
// counter, measured costs or order. launch(group_order, tile_cost, whole_groups) enqueues the kernel.
template <class LAUNCH>
int scheduled_display(vrt_ctx *c, int width, int height, int key, hipStream_t s, const LAUNCH &launch) {
    int tiles_x = 0, n_tiles = 0;
    vrt::launch::denoise_tiling(width, height, tiles_x, n_tiles);
    const long groups = ((long)n_tiles + vrt::kGroupTiles - 1) / vrt::kGroupTiles;
    SchedState *st = nullptr;
    if (c->sched_period > 0 && groups >= kSchedMinDenoiseGroups && groups <= kSchedMaxDenoiseGroups)
        st = sched_state(c, s, width, height, 0, 0, 0, key, (uint32_t)n_tiles, (uint32_t)groups);
    if (!st) {
        VRT_HIP(c, launch(nullptr, nullptr, false));
        return VRT_OK;
    }
    const bool measure = measuring_launch(st->launches, c->sched_period);
    if (measure) VRT_HIP(c, hipMemsetAsync(st->d_cost, 0, (size_t)groups * vrt::kGroupTiles * sizeof(uint32_t), s));
    VRT_HIP(c, launch(st->valid ? st->d_order : nullptr, measure ? st->d_cost : nullptr, true));
    ++st->launches;
    if (measure) {
        const int rr = launch_order_kernel(c, st, s);
        if (rr) return rr;
    }
    return VRT_OK;
}

// vrt_denoise_hdr_host's float images on the device: in and out, 12 bytes per pixel each; grow by ensure_scratch's rule, never shrink
int ensure_hdr_scratch(vrt_ctx *c, size_t px) {
    if (px <= c->hdr_scratch_pixels) return VRT_OK;
    const int r = reserve_synced(c, {{&c->d_hdr_in, px * 12}, {&c->d_hdr_out, px * 12}});
    if (!r) c->hdr_scratch_pixels = px;
    return r;
}

}  // namespace

extern "C" {

int vrt_denoise(vrt_ctx *c, int width, int height, const void *d_rgba8, const void *d_id_dist, void *d_out_rgba8, void *stream) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (!d_rgba8 || !d_id_dist || !d_out_rgba8 || d_rgba8 == d_out_rgba8) return vrt_fail(c, VRT_E_INVALID, "vrt_denoise: null or aliased buffers");
    VRT_HIP(c, hipSetDevice(c->device));
    vrt::launch::Denoise d{d_rgba8, d_id_dist, d_out_rgba8, width, height, nullptr, nullptr};
    d.rows_path = c->denoise_variant;
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return scheduled_display(c, width, height, kSchedDenoise, s, [&](const uint32_t *order, uint32_t *cost, bool whole_groups) {
        d.group_order = order;
        d.tile_cost = cost;
        return vrt::launch::denoise(d, whole_groups, s);
    });
}

int vrt_denoise_hdr(vrt_ctx *c, int width, int height, const void *d_rgb, const void *d_id_dist, const vrt_tonemap *tm, void *d_out_rgb,
                    void *d_out_rgba8, void *stream) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (!d_rgb || !d_id_dist) return vrt_fail(c, VRT_E_INVALID, "vrt_denoise_hdr: null input");
    if (!d_out_rgb && !d_out_rgba8) return vrt_fail(c, VRT_E_INVALID, "vrt_denoise_hdr: both outputs null");
    if (d_out_rgb == d_rgb) return vrt_fail(c, VRT_E_INVALID, "vrt_denoise_hdr: d_out_rgb must not alias d_rgb");
    if ((r = check_tonemap(c, "vrt_denoise_hdr", tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt::launch::DenoiseHdr d{d_rgb, d_id_dist, d_out_rgb, d_out_rgba8, width, height, nullptr, nullptr};
    d.rows_path = c->denoise_variant;
    d.op = tm ? tm->op : VRT_TONEMAP_CLAMP;
    d.exposure = tm ? tm->exposure : 1.0f;
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return scheduled_display(c, width, height, kSchedDenoiseHdr, s, [&](const uint32_t *order, uint32_t *cost, bool whole_groups) {
        d.group_order = order;
        d.tile_cost = cost;
        return vrt::launch::denoise_hdr(d, whole_groups, s);
    });
}

int vrt_denoise_hdr_host(vrt_ctx *c, int width, int height, const float *rgb, const int32_t *id_dist, const vrt_tonemap *tm, float *out_rgb,
                         uint8_t *out_rgba8) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (!rgb || !id_dist) return vrt_fail(c, VRT_E_INVALID, "vrt_denoise_hdr_host: null input");
    if (!out_rgb && !out_rgba8) return vrt_fail(c, VRT_E_INVALID, "vrt_denoise_hdr_host: both outputs null");
    if ((r = check_tonemap(c, "vrt_denoise_hdr_host", tm))) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    if ((r = ensure_scratch(c, px)) || (r = ensure_hdr_scratch(c, px))) return r;
    vrt_stage::Stage st(4);   // the pass's staging depends on its pointers' alignment: the images keep their own buffers
    const int in = st.in(px * 12, rgb, c->d_hdr_in), id = st.in(px * 8, id_dist, c->d_id);
    const int o_rgb = st.out(px * 12, out_rgb, c->d_hdr_out), o_rgba = st.out(px * 4, out_rgba8, c->d_shown);
    if ((r = st.upload(c, c->stream))) return r;
    r = vrt_denoise_hdr(c, width, height, st.at(in), st.at(id), tm, st.at(o_rgb), st.at(o_rgba), nullptr);
    return r ? r : st.download(c, c->stream);
}

int vrt_denoise_host(vrt_ctx *c, int width, int height, const uint8_t *rgba8, const int32_t *id_dist, uint8_t *out_rgba8) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (!rgba8 || !id_dist || !out_rgba8) return vrt_fail(c, VRT_E_INVALID, "vrt_denoise_host: null buffer");
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    r = ensure_scratch(c, px);
    if (r) return r;
    vrt_stage::Stage st(4);
    const int in = st.in(px * 4, rgba8, c->d_rgba), id = st.in(px * 8, id_dist, c->d_id), shown = st.out(px * 4, out_rgba8, c->d_shown);
    if ((r = st.upload(c, c->stream))) return r;
    r = vrt_denoise(c, width, height, st.at(in), st.at(id), st.at(shown), nullptr);
    return r ? r : st.download(c, c->stream);
}

int vrt_dispatch_frame(vrt_ctx *c, int width, int height, int mode, uint8_t *out_shown_rgba8, uint8_t *out_rgba8,
                       int32_t *out_id_dist) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (!out_shown_rgba8) return vrt_fail(c, VRT_E_INVALID, "vrt_dispatch_frame: null output");
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    r = ensure_scratch(c, px);
    if (r) return r;
    r = enqueue(c, width, height, 0, height, height, 0, 0, mode, c->d_rgba, c->d_id, c->stream);
    if (r) return r;
    r = vrt_denoise(c, width, height, c->d_rgba, c->d_id, c->d_shown, nullptr);
    if (r) return r;
    vrt_stage::Stage st(4);
    st.out(px * 4, out_shown_rgba8, c->d_shown);
    st.out(px * 4, out_rgba8, c->d_rgba);
    st.out(px * 8, out_id_dist, c->d_id);
    return st.download(c, c->stream);
}

}  // extern "C"
