// vrt_query.cpp -- the world queries of include/vrt.h (vrt_cast_rays, vrt_cast_rays_device, vrt_find_voxels): call-order
// checks, the scene block of the kernel arguments (fill_scene_args), and the device buffers the host-buffer forms stage through.
#include "vrt_stage.h"
#include "vrt_launch.h"

#include <cstring>

using namespace vrt_internal;

namespace {

int query_state(vrt_ctx *c, const char *what) {
    if (!c) return VRT_E_INVALID;
    if (!c->have_scene) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": no octree uploaded (call vrt_upload_octree first)");
    if (c->batch.open) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": a patch batch is open (call vrt_patch_end first)");
    return VRT_OK;
}

// what the query kernels read of KArgs: the world bounds and the tree in both layouts, wide root 0 as uploaded (no
// tighter root, no root0_only: those are answers the shader may take and octree_ray_cast may not)
int scene_args(vrt_ctx *c, vrt::KArgs &a) {
    const int ra = ensure_analysis(c);
    if (ra) return ra;
    std::memset(&a, 0, sizeof a);
    a.n_views = 1;
    fill_scene_args(c, a);
    a.root0_only = 0;   // never for a query (above)
    return VRT_OK;
}

// ivec3_vec3 (truncation) as the reference's x86-64 build executes it: INT_MIN for NaN and out-of-range values
float box_plane(float v) {
    const int i = (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000u;
    return (float)i;
}

int check_rays(vrt_ctx *c, size_t n, const void *origins, int origin_stride, const void *dirs, const float *box_min,
               const float *box_max, const void *out, const char *what) {
    const int r = query_state(c, what);
    if (r) return r;
    if (origin_stride != 0 && origin_stride != 3) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": origin_stride must be 0 or 3");
    if (n > (size_t)0x7fffffff) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": at most 2^31 rays per call");
    if (n > 0 && (!origins || !dirs || !out)) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null buffer");
    if (n > 0 && (!box_min || !box_max)) return vrt_fail(c, VRT_E_INVALID, std::string(what) + ": null box");
    return VRT_OK;
}

int cast(vrt_ctx *c, size_t n, const float *d_origins, int origin_stride, const float *d_dirs, const float *box_min,
         const float *box_max, vrt::query::RayHit *d_out, hipStream_t s) {
    vrt::KArgs a;
    const int r = scene_args(c, a);
    if (r) return r;
    vrt::query::RayArgs q;
    q.origins = d_origins;
    q.origin_stride = origin_stride;
    q.dirs = d_dirs;
    for (int k = 0; k < 3; ++k) {
        q.box_lo[k] = box_plane(box_min[k]);
        q.box_hi[k] = box_plane(box_max[k]);
    }
    q.out = d_out;
    q.n = (uint32_t)n;
    VRT_HIP(c, vrt::launch::cast_rays(a, q, s));
    return VRT_OK;
}

}  // namespace

extern "C" {

int vrt_cast_rays(vrt_ctx *c, size_t n, const float *origins, int origin_stride, const float *dirs, const float box_min[3],
                  const float box_max[3], vrt_ray_hit *out) {
    int r = check_rays(c, n, origins, origin_stride, dirs, box_min, box_max, out, "vrt_cast_rays");
    if (r || n == 0) return r;
    static_assert(sizeof(vrt_ray_hit) == sizeof(vrt::query::RayHit), "vrt_ray_hit and the kernel's record differ");
    VRT_HIP(c, hipSetDevice(c->device));
    vrt_stage::Stage st(256);
    const int o = st.in((origin_stride ? n : 1) * 3 * sizeof(float), origins), d = st.in(n * 3 * sizeof(float), dirs);
    const int hits = st.out(n * sizeof(vrt_ray_hit), out);
    if ((r = st.reserve_staging(c, c->d_query)) || (r = st.upload(c, c->stream))) return r;   // kept by the context: grown, never shrunk
    r = cast(c, n, st.at<float>(o), origin_stride, st.at<float>(d), box_min, box_max, st.at<vrt::query::RayHit>(hits), c->stream);
    return r ? r : st.download(c, c->stream);
}

int vrt_cast_rays_device(vrt_ctx *c, size_t n, const void *d_origins, int origin_stride, const void *d_dirs,
                         const float box_min[3], const float box_max[3], void *d_out, void *stream) {
    const int r = check_rays(c, n, d_origins, origin_stride, d_dirs, box_min, box_max, d_out, "vrt_cast_rays_device");
    if (r || n == 0) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    return cast(c, n, static_cast<const float *>(d_origins), origin_stride, static_cast<const float *>(d_dirs), box_min, box_max,
                static_cast<vrt::query::RayHit *>(d_out), stream ? (hipStream_t)stream : c->stream);
}

int vrt_find_voxels(vrt_ctx *c, size_t n, const int32_t *coords, uint32_t *out) {
    int r = query_state(c, "vrt_find_voxels");
    if (r) return r;
    if (n > (size_t)0x7fffffff) return vrt_fail(c, VRT_E_INVALID, "vrt_find_voxels: at most 2^31 points per call");
    if (n > 0 && (!coords || !out)) return vrt_fail(c, VRT_E_INVALID, "vrt_find_voxels: null buffer");
    if (n == 0) return VRT_OK;
    VRT_HIP(c, hipSetDevice(c->device));
    vrt::KArgs a;
    r = scene_args(c, a);
    if (r) return r;
    vrt_stage::Stage st(256);
    const int pts = st.in(n * 3 * sizeof(int32_t), coords), found = st.out(n * 3 * sizeof(uint32_t), out);
    st.kept(0);   // the block ends on the alignment, as it always has
    if ((r = st.reserve_staging(c, c->d_query)) || (r = st.upload(c, c->stream))) return r;
    const vrt::query::PointArgs q{st.at<const int32_t>(pts), st.at<uint32_t>(found), (uint32_t)n};
    VRT_HIP(c, vrt::launch::find_voxels(a, q, c->stream));
    return st.download(c, c->stream);
}

}  // extern "C"
