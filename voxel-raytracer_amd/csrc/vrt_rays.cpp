// vrt_rays.cpp -- vrt_shade_rays / vrt_shade_rays_device and their HDR forms (include/vrt.h): pathTrace for ray batches of the caller's. Call-order and
// argument checks, the kernel arguments -- the scene and the uniforms as a frame launch carries them, and nothing of a camera: no
// eye lookup, first lookup, ray table, miss mask, tightened root or tile order -- and the device buffers the host form stages
// through. Reads no camera, lens or accumulation state and writes none.
#include "vrt_stage.h"
#include "vrt_launch.h"

#include <cstring>

using namespace vrt_internal;

namespace {

int check(vrt_ctx *c, size_t n, const void *origins, int origin_stride, const void *dirs, int width, int mode, uint32_t n_samples,
          bool any_out, const char *what) {
    if (!c) return VRT_E_INVALID;
    if (!c->have_scene) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": no octree uploaded (call vrt_upload_octree first)");
    if (c->batch.open) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": a patch batch is open (call vrt_patch_end first)");
    if (origin_stride != 0 && origin_stride != 3) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": origin_stride must be 0 or 3");
    if (mode != VRT_MODE_PRIMARY && mode != VRT_MODE_PRIMARY_SHADOW && mode != VRT_MODE_FULL)
        return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": unknown mode");
    if (width < 1) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": width must be at least 1");
    if (n_samples < 1u || n_samples > (1u << 24)) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": 1 to 2^24 samples per call");
    if (n > ((size_t)1 << 30)) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": at most 2^30 rays per call");
    if (!any_out) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": every output is null");
    if (n > 0 && (!origins || !dirs)) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null buffer");
    return VRT_OK;
}

// What the HDR forms add to a launch: the caller's sums and the count they hold, the float output, the tone map
struct Hdr {
    double *d_sums;
    float *d_rgb;
    uint32_t n_prior;
    const vrt_tonemap *tm;
};

// ... and to the checks (any_out: one of the form's outputs, the sums included, is given)
int check_hdr(vrt_ctx *c, size_t n, const void *origins, int origin_stride, const void *dirs, int width, int mode, uint32_t n_samples,
              bool any_out, const void *sums, uint32_t n_prior, const vrt_tonemap *tm, const char *what) {
    const int r = check(c, n, origins, origin_stride, dirs, width, mode, n_samples, any_out, what);
    if (r) return r;
    if (n_prior != 0u && !sums) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": n_prior without sums");
    if ((uint64_t)n_prior + n_samples > ((uint64_t)1 << 24)) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": more than 2^24 samples in all");
    return check_tonemap(c, what, tm);
}

// The launch: the scene and light blocks of KArgs as a frame carries them (vrt_scene.cpp), and nothing derived from an eye
int shade(vrt_ctx *c, size_t n, const float *d_origins, int origin_stride, const float *d_dirs, int width, int mode, uint32_t first_sample,
          uint32_t n_samples, uint32_t *d_rgba, int2 *d_id, hipStream_t s, const Hdr *hdr = nullptr) {
    const int ra = ensure_analysis(c);
    if (ra) return ra;
    const Variant v = base_variant(c);   // the launch reads its traversal only
    vrt::KArgs a;
    vrt::ViewSet vs;
    fill_ray_batch_args(c, n, width, a, vs);
    // the HDR forms hand the float itself out: below 2^-103 div_pi_inrange() may differ from x / PI in the last bit -- a colour term
    // that stores byte 0 either way, but a different float
    if (hdr) a.shade_fast = 0;
    // the kernels of VRT_MODE_FULL by the context's settings as this call finds them, the emitter list made for the current tree
    PathSetup ps{c->path_depth, c->sun_disc, mode == VRT_MODE_FULL && c->emitter_sampling, c->emitter_importance, c->emitter_mis};
    if (ps.sampling) {
        const int re = ensure_emitters(c, "vrt_shade_rays", true);
        if (re) return re;
        ps.list = c->emitters.d_list.get();
        ps.n = (uint32_t)c->emitters.n;
        ps.cdf = c->emitters.d_cdf.get();
        ps.inv_power = emitter_inv_power(c->emitters.wtot);
    }
    vrt::launch::PathFamily fam;
    vrt::launch::PathArgs pa;
    vrt::launch::select_paths(mode, ps, a.light_dir, false, fam, pa);   // no opaque route here: nothing is refused
    if (mode == VRT_MODE_FULL) a.path_depth = (uint32_t)c->path_depth;   // vrt_set_path_depth: every family but the plain one reads it

    vrt::rays::HdrArgs q{};   // Args first in the layout (what late_rays(), vrt_rays.hip.h, relies on), then what the HDR forms add
    q.origins = d_origins;
    q.dirs = d_dirs;
    q.out_rgba = d_rgba;
    q.out_id = d_id;
    q.n = (uint32_t)n;
    q.origin_stride = origin_stride;
    q.width = (uint32_t)width;
    q.first = first_sample;
    // the primary modes draw no random number, every sample is the same: the plain forms trace one, the HDR forms add it n_samples times over
    q.n_samples = (mode == VRT_MODE_FULL || hdr) ? n_samples : 1u;
    if (hdr) {
        q.sums = hdr->d_sums;
        q.out_rgb = hdr->d_rgb;
        q.n_total = hdr->n_prior + n_samples;
        q.op = hdr->tm ? hdr->tm->op : VRT_TONEMAP_CLAMP;
        q.exposure = hdr->tm ? hdr->tm->exposure : 1.0f;
    }
    const uint32_t grid = vrt::rays::plan(q.n, q.width, q.tiles_x);
    const ProfSlot prof = ProfSlot::take(c);
    hipError_t e;
    if (mode == VRT_MODE_FULL) e = vrt::launch::shade_rays_full(hdr != nullptr, fam, pa, v, a, vs, q, grid, s, prof.ev0, prof.ev1);
    else if (hdr) e = vrt::launch::shade_rays_hdr(mode, v, a, vs, q, grid, s, prof.ev0, prof.ev1);
    else e = vrt::launch::shade_rays(mode, v, a, vs, q, grid, s, prof.ev0, prof.ev1);
    if (e != hipSuccess) return vrt_fail(c, VRT_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    prof.commit(c);
    return VRT_OK;
}

}  // namespace

void vrt_internal::fill_ray_batch_args(const vrt_ctx *c, size_t n, int width, vrt::KArgs &a, vrt::ViewSet &vs) {
    std::memset(&a, 0, sizeof a);
    std::memset(&vs, 0, sizeof vs);   // no first lookup (first_valid 0), no ray tables (gen_fast 0), no miss mask
    a.n_views = 1;
    fill_scene_args(c, a);
    fill_light_args(c, a);
    a.width = width;
    a.height = (int)((n + (size_t)width - 1) / (size_t)width);
    a.n_rows = a.height;
    a.tile_rows = a.height;
    a.row_mode = 1;
    // the world is empty outside wide root 0: a property of the tree, applied by find() per ray (never to a first lookup); the
    // tighter root is a property of a view's eye and is not taken
    a.root0_only = (a.n_roots == 1u && c->root0_only_on && vrt::content_only_in_root0(c->host_records, c->wide)) ? 1 : 0;
}

extern "C" {

int vrt_shade_rays(vrt_ctx *c, size_t n, const float *origins, int origin_stride, const float *dirs, int width, int mode,
                   uint32_t first_sample, uint32_t n_samples, uint8_t *out_rgba8, int32_t *out_id_dist) {
    int r = check(c, n, origins, origin_stride, dirs, width, mode, n_samples, out_rgba8 || out_id_dist, "vrt_shade_rays");
    if (r || n == 0) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt_stage::Stage st(256);
    const int o = st.in((origin_stride ? n : 1) * 3 * sizeof(float), origins), d = st.in(n * 3 * sizeof(float), dirs);
    const int rgba = st.out(out_rgba8 ? n * 4 : 0, out_rgba8), id = st.out(out_id_dist ? n * 8 : 0, out_id_dist);
    if ((r = st.reserve_staging(c, c->d_rays)) || (r = st.upload(c, c->stream))) return r;   // kept by the context: grown, never shrunk
    r = shade(c, n, st.at<float>(o), origin_stride, st.at<float>(d), width, mode, first_sample, n_samples, st.at<uint32_t>(rgba), st.at<int2>(id),
              c->stream);
    return r ? r : st.download(c, c->stream);
}

int vrt_shade_rays_device(vrt_ctx *c, size_t n, const void *d_origins, int origin_stride, const void *d_dirs, int width, int mode,
                          uint32_t first_sample, uint32_t n_samples, void *d_rgba8, void *d_id_dist, void *stream) {
    const int r = check(c, n, d_origins, origin_stride, d_dirs, width, mode, n_samples, d_rgba8 || d_id_dist, "vrt_shade_rays_device");
    if (r || n == 0) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    return shade(c, n, static_cast<const float *>(d_origins), origin_stride, static_cast<const float *>(d_dirs), width, mode, first_sample,
                 n_samples, static_cast<uint32_t *>(d_rgba8), static_cast<int2 *>(d_id_dist), stream ? (hipStream_t)stream : c->stream);
}

int vrt_shade_rays_hdr(vrt_ctx *c, size_t n, const float *origins, int origin_stride, const float *dirs, int width, int mode,
                       uint32_t first_sample, uint32_t n_samples, const vrt_tonemap *tm, float *out_rgb, uint8_t *out_rgba8,
                       int32_t *out_id_dist) {
    int r = check_hdr(c, n, origins, origin_stride, dirs, width, mode, n_samples, out_rgb || out_rgba8 || out_id_dist, nullptr, 0u, tm,
                      "vrt_shade_rays_hdr");
    if (r || n == 0) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt_stage::Stage st(256);
    const int o = st.in((origin_stride ? n : 1) * 3 * sizeof(float), origins), d = st.in(n * 3 * sizeof(float), dirs);
    const int rgba = st.out(out_rgba8 ? n * 4 : 0, out_rgba8), id = st.out(out_id_dist ? n * 8 : 0, out_id_dist);
    const int rgb = st.out(out_rgb ? n * 12 : 0, out_rgb);
    if ((r = st.reserve_staging(c, c->d_rays)) || (r = st.upload(c, c->stream))) return r;
    const Hdr hdr{nullptr, st.at<float>(rgb), 0u, tm};
    r = shade(c, n, st.at<float>(o), origin_stride, st.at<float>(d), width, mode, first_sample, n_samples, st.at<uint32_t>(rgba), st.at<int2>(id),
              c->stream, &hdr);
    return r ? r : st.download(c, c->stream);
}

int vrt_shade_rays_hdr_device(vrt_ctx *c, size_t n, const void *d_origins, int origin_stride, const void *d_dirs, int width, int mode,
                              uint32_t first_sample, uint32_t n_samples, uint32_t n_prior, void *d_sums, const vrt_tonemap *tm,
                              void *d_rgb, void *d_rgba8, void *d_id_dist, void *stream) {
    const int r = check_hdr(c, n, d_origins, origin_stride, d_dirs, width, mode, n_samples, d_rgb || d_rgba8 || d_id_dist || d_sums, d_sums,
                            n_prior, tm, "vrt_shade_rays_hdr_device");
    if (r || n == 0) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const Hdr hdr{static_cast<double *>(d_sums), static_cast<float *>(d_rgb), n_prior, tm};
    return shade(c, n, static_cast<const float *>(d_origins), origin_stride, static_cast<const float *>(d_dirs), width, mode, first_sample,
                 n_samples, static_cast<uint32_t *>(d_rgba8), static_cast<int2 *>(d_id_dist), stream ? (hipStream_t)stream : c->stream, &hdr);
}

}  // extern "C"
