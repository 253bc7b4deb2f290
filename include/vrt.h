/*
 * vrt.h -- C-ABI of the MI355X (gfx950) ray-casting layer: libvrt_hip.so.
 *
 * Drop-in boundary for the compute-shader dispatch of pedroand6/Voxel-Raytracer.
 * Each entry point replaces one piece of the reference's GL plumbing around
 * `glDispatchCompute` (reference paths are relative to the upstream repo root):
 *
 *   vrt_create / vrt_destroy   GL object setup/teardown        src/main.cpp:432-474, 973-983
 *   vrt_upload_octree          updateGPUTexture()/glTexImage3D src/main.cpp:264-311
 *   vrt_set_camera             Camera UBO glBufferSubData      src/main.cpp:643-656, 807-813, 916-917
 *   vrt_set_params             the seven glUniform* calls      src/main.cpp:689-695, 932-938
 *   vrt_dispatch*              glMemoryBarrier+glDispatchCompute src/main.cpp:941-946
 *                              (shader: shaders/raytracing.comp:624-645)
 *
 * Plain pointers and sizes only; no C++/torch types cross this boundary and no
 * exception escapes. Every call returns 0 on success or a negative VRT_E_*;
 * vrt_last_error() gives the text. One context per host thread (thread-
 * compatible, not thread-safe). There is no CPU fallback: without a HIP device
 * vrt_create fails with VRT_E_NO_DEVICE.
 */
#ifndef VRT_H
#define VRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRT_OK 0
#define VRT_E_INVALID (-1)    /* bad argument */
#define VRT_E_NO_DEVICE (-2)  /* no usable HIP device / HIP runtime error at create */
#define VRT_E_HIP (-3)        /* HIP runtime call failed */
#define VRT_E_MALFORMED (-4)  /* texel stream cannot be a flattened octree */
#define VRT_E_STATE (-5)      /* call order (e.g. dispatch before upload) */

/* which subset of pathTrace (raytracing.comp:435-622) a dispatch evaluates */
#define VRT_MODE_PRIMARY 0         /* primary ray, direct term unshadowed */
#define VRT_MODE_PRIMARY_SHADOW 1  /* + notInShadow() ray per opaque hit (comp:333-377, 587) */
#define VRT_MODE_FULL 2            /* the whole shader: glass stack, diffuse bounce, RNG */

typedef struct vrt_ctx vrt_ctx;

/* The shader's scalar uniforms (raytracing.comp:27-39). u_texDim travels with
 * vrt_upload_octree. Defaults = the values src/main.cpp:478-483,638 sets. */
typedef struct vrt_params {
    float voxel_scale;          /* u_voxelScale            (1.0)              */
    int32_t world_min[3];       /* u_worldBoundsMin        (-1023,-1023,-1023) */
    int32_t world_max[3];       /* u_worldBoundsMax        (1024,1024,1024)    */
    float global_light[4];      /* globalLight             (1,1,1,1)           */
    float light_dir[3];         /* lightDir  normalize(.3481553,.870388,.3481553) */
    int32_t highlighted[3];     /* u_highlightedVoxel      (-1,-1,-1)          */
} vrt_params;

typedef struct vrt_scene_info {
    uint32_t tex_dim;           /* u_texDim given at upload */
    uint32_t n_texels;          /* texels in the uploaded stream */
    uint32_t n_records;         /* 8-byte device records (internal + leaf) */
    uint32_t n_internal;        /* internal nodes */
    uint32_t n_leaves;          /* leaf nodes */
    uint32_t max_depth;         /* deepest node below the root */
    uint32_t lds_records;       /* always 0 (no kernel stages records in LDS) */
    uint32_t reserved;
} vrt_scene_info;

int vrt_create(int device_id, vrt_ctx **out);
void vrt_destroy(vrt_ctx *ctx);
/* ctx may be NULL: returns the message of the last failed vrt_create on this thread */
const char *vrt_last_error(const vrt_ctx *ctx);

/* Fills *p with the reference defaults. */
void vrt_default_params(vrt_params *p);
int vrt_set_params(vrt_ctx *ctx, const vrt_params *p);

/* texels: the byte stream octree_texture() returns (4 bytes per texel, root
 * header at texel 0), used_bytes its size, tex_dim = ceil(cbrt(texels)).
 * The library copies and re-lays it out for the device; the caller keeps
 * ownership. texels == NULL / used_bytes == 0 uploads an empty world. */
int vrt_upload_octree(vrt_ctx *ctx, const uint8_t *texels, size_t used_bytes, uint32_t tex_dim);
int vrt_get_scene_info(const vrt_ctx *ctx, vrt_scene_info *info);

/* EXTENSION: edits without re-flattening and re-uploading the tree (the reference does both on every build / destroy
 * click, src/main.cpp:903-914). After the host octree has been edited at voxel (x, y, z):
 *   1. vrt_patch_plan() names the deepest ancestor A of the voxel (depth <= max_depth) whose sub-tree can be replaced
 *      on the device: depth below the root and the child index taken at each level;
 *   2. the host library says whether A is still an internal node (vrth_octree_node_state) -- if not, plan again with
 *      max_depth = depth - 1 -- and emits A's new sub-tree (vrth_octree_path_records: just the nodes that contain the
 *      voxel, or vrth_octree_subtree_records: all of it);
 *   3. vrt_patch_apply() appends those records, rewrites A's record, rebuilds A's part of the wide layout and copies
 *      only what changed to the device (after waiting for dispatches in flight).
 * vrt_patch_plan returns VRT_E_STATE when no ancestor qualifies (use vrt_upload_octree / vrt_upload_records).
 * Replaced sub-trees stay allocated until they outweigh the tree, then vrt_patch_plan compacts the arrays (vrt_compact);
 * vrt_get_scene_info().n_records shows both.
 * Pixels after a patch equal those after a full upload of the edited tree. */
typedef struct vrt_patch {
    int32_t depth;       /* of A below the root, >= 1 */
    uint8_t path[16];    /* child index taken at levels 0 .. depth-1 */
} vrt_patch;
int vrt_patch_plan(vrt_ctx *ctx, int x, int y, int z, int max_depth, vrt_patch *out);
/* The same for an edit that touched a whole BOX of voxels [lo, hi] (inclusive) -- a fill, an explosion: the deepest patchable
 * ancestor whose cube holds the box. The host library then emits ONE sub-tree for it (vrth_octree_box_records: only the nodes
 * that meet the box are walked, the rest are "keep" records) and ONE vrt_patch_apply replaces it: a 16^3 fill is one patch,
 * not 4,096. */
int vrt_patch_plan_box(vrt_ctx *ctx, const int32_t lo[3], const int32_t hi[3], int max_depth, vrt_patch *out);
int vrt_patch_apply(vrt_ctx *ctx, const vrt_patch *patch, const uint32_t *subtree_records, size_t n_records);
/* A batch of edits (a brush stroke, an explosion; src/main.cpp:843-914 re-flattens once per click): between
 * vrt_patch_begin and vrt_patch_end, vrt_patch_plan / vrt_patch_apply work on the library's host copy of the structures
 * only -- each plan sees the patches before it -- and vrt_patch_end sends everything the batch appended or rewrote to the
 * device in one go (one wait for dispatches in flight, one upload). Dispatching with a batch open is an error
 * (VRT_E_STATE). A patch the library refuses (VRT_E_STATE / VRT_E_MALFORMED) changes nothing; a device failure in
 * vrt_patch_end drops the scene (upload again). Outside a batch vrt_patch_apply is begin + apply + end. */
int vrt_patch_begin(vrt_ctx *ctx);
int vrt_patch_end(vrt_ctx *ctx);
/* Reclaims what patches left behind (replaced child blocks and wide nodes): the device arrays are re-laid from the live
 * tree, without a texel stream. vrt_patch_plan does this by itself once the garbage outweighs the tree; pixels do not
 * change. */
int vrt_compact(vrt_ctx *ctx);

/* EXTENSION (not a reference interface): upload the device record array itself -- 2 x uint32 per record,
 * level order, root first; internal: {child_mask | leaf_mask << 8, first child index}, leaf:
 * {R | G<<8 | B<<16 | alpha<<24, refr | illum<<8 | k<<16} -- as vrth_world_records() (vrt_host.h) emits it
 * straight from the pointer octree. It replaces the reference's full re-flatten + re-upload on every edit
 * (src/main.cpp:903-914 -> :264-311) and is not limited to 2^23 texels (src/octree.cpp:556-570).
 * tex_dim must still be ceil(cbrt(_octree_texel_size(tree))): it feeds the voxelID output. */
int vrt_upload_records(vrt_ctx *ctx, const uint32_t *records, size_t n_records, uint32_t tex_dim);

/* EXTENSION: the world questions of the reference's frame loop, answered on the device from the uploaded tree (after
 * patches and compaction, whatever the scene form) instead of a host copy kept in step with it.
 *   vrt_cast_rays     octree_ray_cast (src/octree.cpp:364-485) as src/main.cpp:822-829 picks the voxel under the
 *                     crosshair, plus get_placement_coord (src/main.cpp:315-360), the cell a build click fills (:864)
 *   vrt_find_voxels   octree_find (src/octree.cpp:102-130) as isVoxelSolid / checkCollision ask it (src/main.cpp:100-125)
 * The answers are the reference's functions, bit for bit, on the pointer tree the device tree was made from with ONE
 * difference the device tree cannot express: a leaf whose record words are 0/0 (colour 0, zero material) is empty space
 * there. Such leaves are the phantom voxels of SURVEY F3 (coord.y = MIN_HEIGHT: never hit anyway) and the "ghost" volumes
 * the F1 split makes of them -- a phantom whose lbb has x = z = 0 is split as a volume, its children get coord = their
 * lbb, and the reference's ray cast and octree_find DO hit those (invisible: alpha 0; 38 leaves in dragon.vox, 682 in
 * nature.vox) -- plus any voxel inserted with colour 0 and zero material. The queries answer as the reference does on
 * the tree with those leaves' has_voxel cleared (csrc/vrt_query.hip.h). World bounds of vrt_params must be the tree's
 * root cube (the reference: [-1023, 1024)^3 both, src/main.cpp:478-480). coord is the hit node's minimum corner, which
 * voxel.coord is for every other leaf octree_insert / octree_remove make. Leaf words are the records
 * vrth_world_records() emits, refraction byte 0 under alpha 0 (the layouts keep no other). VRT_E_STATE before any upload and while a patch batch is open; NULL buffers with
 * n > 0 are VRT_E_INVALID; n == 0 does nothing. At most 2^31 rays / points per call. */
typedef struct vrt_ray_hit {
    int32_t hit;        /* 1: octree_ray_cast returned a node, 0: NULL                                              */
    int32_t coord[3];   /* node->voxel.coord of the returned node (src/main.cpp:831); -1,-1,-1 on a miss            */
    int32_t place[3];   /* get_placement_coord(origin, dir, coord) (src/main.cpp:315-360); -1,-1,-1 on a miss       */
    uint32_t leaf[2];   /* the hit leaf's device record words: RGBA, refr | illum << 8 | k << 16; 0 on a miss       */
    int32_t steps;      /* loop iterations begun (<= 512): for tests and tuning                                     */
} vrt_ray_hit;          /* 40 bytes */
/* n rays: origins n x 3 floats (origin_stride 3), or ONE origin shared by all rays (origin_stride 0: config 1, picking);
 * dirs n x 3, used as given (the reference does not normalise them); box_min / box_max = octree_ray_cast's worldMin /
 * worldMax (the reference passes 0..1024), truncated to int as the reference does. The same origin feeds the placement
 * (the reference passes camera.Position there and Position * voxelScale to the cast: equal at its voxelScale 1).
 * HOST buffers, synchronous (copied through device buffers the context keeps). As for frames, page-locked host buffers
 * (vrt_host_alloc) make the copies faster: from pageable memory the runtime stages them, and at 1 M rays the copies
 * are most of the call. */
int vrt_cast_rays(vrt_ctx *ctx, size_t n, const float *origins, int origin_stride, const float *dirs, const float box_min[3],
                  const float box_max[3], vrt_ray_hit *out);
/* The same on DEVICE buffers (d_out: n vrt_ray_hit), enqueued on `stream` (NULL: the context's) -- ordered after the
 * patches and frames enqueued before it on that stream; returns after enqueueing. */
int vrt_cast_rays_device(vrt_ctx *ctx, size_t n, const void *d_origins, int origin_stride, const void *d_dirs,
                         const float box_min[3], const float box_max[3], void *d_out, void *stream);
/* octree_find for n integer points (n x 3 int32): out n x 3 uint32 = {present, leaf word 0, leaf word 1}. present is
 * isVoxelSolid's v.coord.y > MIN_HEIGHT, with octree_find's own equality (vmm's ivec3_equal_vec: x and z equal, both y
 * non-zero -- SURVEY F1): inside a merged volume only the column of its corner, and no point with y == 0, is found; and
 * with octree_find's own child choice at (lbb + rtf) / 2, which differs from the tree's split lo + (hi - lo) / 2 where
 * lo + hi is odd and negative: a voxel on the planes -512, -768, -896, ... of the reference's world is not found.
 * The words are 0 when present is 0. HOST buffers, synchronous. */
int vrt_find_voxels(vrt_ctx *ctx, size_t n, const int32_t *coords, uint32_t *out);

/* EXTENSION: the SHADED answer for rays of the caller's own -- panoramic and fisheye cameras, cube-map faces, light probes, a
 * mirror pass, sparse re-rendering: pathTrace (comp:435-622) for n rays, in `mode` (VRT_MODE_PRIMARY, _PRIMARY_SHADOW, _FULL).
 *   Rays      ray i is pathTrace(origin_i, dir_i) exactly as the shader's main() calls it (comp:641). origin_i is in world units,
 *             the units of camera_pos, before u_voxelScale: gro = origin_i * u_voxelScale, the medium the ray starts in is looked
 *             up at floor(gro) (comp:445-449), and the distance in the medium and the eye vector of the shading come from
 *             origin_i. origin_stride 3: n x 3 floats; 0: ONE origin shared by all rays, as in vrt_cast_rays.
 *   Direction dir_i (n x 3 floats) is used as given; pathTrace normalises it on entry (comp:441) as d * (1 / sqrt(dot(d, d))),
 *             float32, every operation rounded on its own, / and sqrt correctly rounded: any length from 1e-3 to 1e3 and far
 *             beyond gives the ray of the unit vector those operations make of it. A zero, infinite or NaN direction or origin
 *             gives an unspecified result for THAT ray; the call still terminates and no other ray of the batch changes.
 *   State     the uploaded tree (after patches and compaction, either upload form) and vrt_params (bounds, u_texDim for the
 *             voxel ID, the lights, the highlighted voxel). No camera is read (vrt_set_camera is not needed), and no
 *             accumulation, lens, ray table, miss mask or tile order is read or written: frames and accumulations before and
 *             after the call are what they would be without it. Pixels do not depend on vrt_set_variant / vrt_set_option.
 *   width     >= 1: the batch is read as an image of that width FOR THE RANDOM NUMBERS ONLY: ray i of sample k seeds
 *             initRNG(ivec2(i % width, i / width), k) (comp:380-387). A batch that is a frame's rays in row-major order, with the
 *             frame's width, therefore draws the frame's random numbers and gives the frame, byte for byte. A plain list passes
 *             any width. (Batches at least 8 wide and two rows high are also traced in 8 x 8 tiles of that image, the frame
 *             kernels' shape; that is a matter of speed, never of results.)
 *   Samples   the result is the mean of samples first_sample ... first_sample + n_samples - 1 (indices modulo 2^32) by the
 *             accumulation's rule: per channel the integer sum of the unorm8 bytes each sample would store, resolved as
 *             (sum + n_samples / 2) / n_samples, alpha 255; n_samples == 1 is the sample itself. VRT_MODE_PRIMARY and
 *             _PRIMARY_SHADOW draw no random number, so every sample is the same and one is traced. 1 <= n_samples <= 2^24.
 *   Outputs   out_rgba8: n x 4 bytes; out_id_dist: n x 2 int32 = (voxelID, dist) of ray i's primary hit as vrt_dispatch stores
 *             them (0 and the world's x extent on a miss). Either may be NULL, not both.
 *   Errors    VRT_E_STATE before any upload and while a patch batch is open. VRT_E_INVALID: origin_stride not 0 or 3, an unknown
 *             mode, width < 1, n_samples outside [1, 2^24], n > 2^30, both outputs NULL, NULL origins or dirs with n > 0.
 *             n == 0 (with valid arguments otherwise) does nothing and returns VRT_OK.
 * vrt_shade_rays: HOST buffers, synchronous, copied through device buffers the context keeps and grows. */
int vrt_shade_rays(vrt_ctx *ctx, size_t n, const float *origins, int origin_stride, const float *dirs, int width, int mode,
                   uint32_t first_sample, uint32_t n_samples, uint8_t *out_rgba8, int32_t *out_id_dist);
/* The same on DEVICE buffers, enqueued on `stream` (NULL: the context's) -- ordered after the patches and frames enqueued before
 * it on that stream; returns after enqueueing. */
int vrt_shade_rays_device(vrt_ctx *ctx, size_t n, const void *d_origins, int origin_stride, const void *d_dirs, int width,
                          int mode, uint32_t first_sample, uint32_t n_samples, void *d_rgba8, void *d_id_dist, void *stream);

/* Progressive multi-sample accumulation (one per context; vrt_accum_begin_ex below: the other modes, sub-pixel jitter).
 * Sample k is the VRT_MODE_FULL frame rendered with initRNG(pixel, k) (shaders/raytracing.comp:380-387; the shader itself
 * passes 0): camera, uniforms, tree and every other convention unchanged. The accumulation holds the samples first, first + 1,
 * ..., first + n - 1 (sample indices modulo 2^32) as
 * one integer sum per pixel and channel of the unorm8 bytes each sample would store -- exact, whatever chunks they were added
 * in -- and resolves to (sum + n / 2) / n per channel, alpha 255: at n = 1 the sample itself. Averaging clamped bytes is what a
 * display of the successive frames shows (the mean of the unclamped colours: vrt_accum_keep_hdr below). The resolved (voxel ID, dist) image is the frame's: no sample changes it.
 *
 * vrt_accum_begin     (re)starts with zero samples; allocates (grows) the accumulation's device buffers.
 * vrt_accum_add       enqueues n_samples more on the context's stream and stores the new count in *total_out (may be NULL).
 *                     Restart rule: when the camera block's bytes, the vrt_params bytes (highlighted voxel and bounds
 *                     included) or the tree (upload, patch apply / batch end, compaction) differ from what the first sample
 *                     in the sums saw, the sums start again at `first` -- *total_out then shows n_samples. Setting the same
 *                     values again changes nothing, so "add one sample per frame" converges exactly while nothing moves.
 *                     VRT_E_INVALID: n_samples == 0, or more than 2^24 samples in all. VRT_E_STATE: no begin, no scene or
 *                     camera, or a patch batch is open.
 * vrt_accum_resolve   the resolved rgba8 [H][W][4], id_dist [H][W][2] and the display pass of vrt_denoise on them, into host
 *                     buffers (any may be NULL); synchronous. VRT_E_STATE: no begin, or no sample yet.
 * vrt_accum_resolve_device  the same into device buffers, enqueued on `stream` (NULL: the context's), ordered after the adds
 *                     before it and before the adds after it; d_shown_rgba8 needs d_rgba8. */
int vrt_accum_begin(vrt_ctx *ctx, int width, int height, uint32_t first_sample);

/* Anti-aliased progressive frames, and accumulations of the other two modes. vrt_accum_begin_ex (re)starts an accumulation of
 * `mode` (VRT_MODE_PRIMARY, _PRIMARY_SHADOW or _FULL); vrt_accum_begin(ctx, w, h, first) is exactly
 * vrt_accum_begin_ex(ctx, w, h, VRT_MODE_FULL, first, 0). The mode and flags belong to the accumulation: add, resolve,
 * resolve_device, the 2^24 cap and the restart rule are the ones above. VRT_E_INVALID: an unknown mode or flag.
 *
 * Without VRT_ACCUM_JITTER sample k is the frame of `mode` (VRT_MODE_FULL: with initRNG(pixel, k), as above; the other two modes
 * draw no random number, so every sample is their frame and the resolve is that frame byte for byte).
 *
 * VRT_ACCUM_JITTER: sample k also moves the pixel's ray inside the pixel. The shader's ray generation
 * u = (float(px) / float(W)) * 2 - 1 (comp:631-638, and v with py and H) measures from the pixel's corner; jittered sample k uses
 * float(px) + jx(k) and float(py) + jy(k) instead of float(px) and float(py) -- one float32 addition each, rounded to nearest,
 * not contracted into the divide or multiply-add that follows. Everything after that -- the projection, the normalisations, the
 * traversal, the shading, the unorm8 store -- is unchanged, and in VRT_MODE_FULL the sample also seeds initRNG(pixel, k).
 * The offsets are a 2-D (0,2)-sequence, every value exact in float32:
 *     jx(k) = (float)(bitreverse32(k) >> 8) * 0x1p-24f                      van der Corput, base 2
 *     jy(k) = (float)(sobol2(k) >> 8) * 0x1p-24f                            Sobol's second dimension:
 *             sobol2(k): y = 0; v = 1u << 31; for (i = k; i; i >>= 1, v ^= v >> 1) if (i & 1) y ^= v;
 * so jx, jy lie in [0, 1), (jx, jy)(0) = (0, 0) -- sample 0 is the frame -- and the first 2^m samples of any aligned block of
 * 2^m fall one into each elementary interval. The first eight: (0, 0), (1/2, 1/2), (1/4, 3/4), (3/4, 1/4), (1/8, 5/8),
 * (5/8, 1/8), (3/8, 3/8), (7/8, 7/8).
 * The resolved id_dist is the unjittered frame's: what vrt_dispatch stores in that mode. The display pass runs on the resolved
 * mean with that image. */
#define VRT_ACCUM_JITTER 1u
int vrt_accum_begin_ex(vrt_ctx *ctx, int width, int height, int mode, uint32_t first_sample, uint32_t flags);
int vrt_accum_add(vrt_ctx *ctx, uint32_t n_samples, uint32_t *total_out);
int vrt_accum_resolve(vrt_ctx *ctx, uint8_t *out_rgba8, int32_t *out_id_dist, uint8_t *out_shown_rgba8);
int vrt_accum_resolve_device(vrt_ctx *ctx, void *d_rgba8, void *d_id_dist, void *d_shown_rgba8, void *stream);

/* Thin lens for the progressive accumulation. aperture: lens radius; focus_distance: distance of the plane of focus
 * along the view axis. Both are in world units, the units of camera_pos (before u_voxelScale). Default (0, 1): a pinhole.
 * VRT_E_INVALID unless aperture is finite and >= 0 and focus_distance is finite and > 0. The lens is context state, like the
 * camera, and applies to every accumulation mode, with or without VRT_ACCUM_JITTER; its bytes join the restart rule (a change
 * restarts the sums at `first`, the same values set again change nothing). Frames, views, shards and vrt_multi stay pinhole.
 *
 * Sample k with a lens, all arithmetic float32, every operation rounded on its own (no contraction):
 *  1. d: the pixel's ray direction as the shader's prologue hands it to pathTrace (comp:640-641), with the jittered pixel
 *     position under VRT_ACCUM_JITTER and the corner without; e = camera_pos.xyz.
 *  2. Lens point (lu, lv) in [0,1)^2: two digital sequences over x^3+x+1 (m = 1,1,5) and x^3+x^2+1 (m = 1,3,1), 24 bits,
 *     top bit flipped (a digital shift by 1/2, so that sample 0 is the lens centre):
 *        direction numbers v[i] = m[i] << (31 - i) for i < 3, then v[i] = v[i-3] ^ (v[i-3] >> 3) ^ (x^2 term: v[i-1]) ^
 *        (x term: v[i-2]); g(D, k) = XOR of D[i] over the set bits i of k;
 *        lu(k) = (float)((g(U, k) >> 8) ^ 0x800000) * 0x1p-24f, lv(k) likewise with V.
 *     The first eight: (1/2,1/2), (0,0), (3/4,1/4), (1/4,3/4), (1/8,5/8), (5/8,1/8), (3/8,3/8), (7/8,7/8).
 *  3. Concentric map to the unit disc (Shirley-Chiu): a = 2*lu - 1, b = 2*lv - 1; a == b == 0: (lx, ly) = (0, 0); else if
 *     |a| > |b|: r = a, phi = 0.785398163f * (b / a); else r = b, phi = 1.57079633f - 0.785398163f * (a / b);
 *     lx = r * cos(phi), ly = r * sin(phi) with the conventions' Cephes sin/cos (det_sincos).
 *  4. R = inv_view[0..2], U = inv_view[4..6], Z = inv_view[8..10] (column-major, as given);
 *     cosd = -((d.x*Z.x + d.y*Z.y) + d.z*Z.z).
 *  5. aperture == 0, or lx == ly == 0, or !(cosd > 0): the pinhole ray (e, d) bit for bit. Otherwise sx = aperture*lx,
 *     sy = aperture*ly, o_i = (e_i + sx*R_i) + sy*U_i, t = focus_distance / cosd, p_i = e_i + t*d_i, dir = normalize(p - o),
 *     and the sample is pathTrace from o along dir, which normalises dir again on entry as it does any ray (comp:441;
 *     VRT_MODE_FULL: with initRNG(pixel, k)). Everything the shader derives
 *     from the ray origin comes from o: gro = o * u_voxelScale, the medium looked up at floor(gro), the distance in the medium
 *     and the eye vector of the shading.
 *  6. The resolved id_dist stays the unjittered pinhole frame's.
 * Sample 0 is therefore the frame, and aperture 0 reproduces the lens-free accumulations byte for byte. */
int vrt_set_lens(vrt_ctx *ctx, float aperture, float focus_distance);

/* Path depth: multi-bounce diffuse paths. The shader declares BOUNCES (comp:8) but a ray of depth >= 1 that hits an opaque
 * surface adds the ambient term and ends (comp:590-594): its light transport is one cosine-weighted bounce whatever the constant
 * says. vrt_set_path_depth sets the depth D of the samples of VRT_MODE_FULL, an integer in 1..VRT_MAX_PATH_DEPTH, default 1;
 * VRT_E_INVALID outside that range (the previous depth still holds). It is context state, like the uniforms.
 *
 * The rule. Inside pathTrace's loop only the opaque, non-emissive branch (comp:584-616) changes. A ray of depth d at such a hit:
 *   d == 0       unchanged: the direct term through notInShadow, then the bounce ray of depth 1.
 *   1 <= d < D   an inner vertex. It takes the depth-0 operations verbatim, in this order:
 *                  lit = notInShadow(hitPoint + normal * 2e-3, lightDir);
 *                  finalColor += globalLight.rgb * lit * ndotl * surfaceColor.rgb * transmittedColor.rgb * weight / PI;
 *                  two rand() draws; cosineSampleHemisphere(normal, r);
 *                  a new ray from hitPoint + normal * 1e-1 with rayIOF n1, the same weight, tint transmittedColor * surfaceColor,
 *                  distanceInMedium 0, the last voxel as its medium, depth d + 1.
 *                It adds no ambient term.
 *   d == D       the shader's terminal branch: the ambient term max(1 - exp(-distanceInMedium / 512), 0.01), then `continue`.
 * Nothing else moves: a miss at depth > 0 adds sky * sunIntensity / PI; an emissive hit at depth > 0 adds emission / PI and ends
 * the path; translucent surfaces are glass only at depth <= 0 and diffuse below it, so a bounce chain is linear and never pushes;
 * (voxel ID, dist) come from depth 0 only; the random numbers come from the pixel's one initRNG stream, in the order the LIFO
 * stack pops the rays. At D == 1 the middle case is empty and the rule is the shader.
 *
 * Who honours it: the samples of VRT_MODE_FULL in the progressive accumulation (vrt_accum_add in every form: corner, jitter, lens,
 * adaptive, HDR) and in ray batches (vrt_shade_rays, _device, _hdr, _hdr_device). The depth is one of the inputs of an accumulation
 * of VRT_MODE_FULL: a change restarts the sums at `first`, the same value set again changes nothing. The primary modes ignore it,
 * their accumulations included (no restart). vrt_dispatch*
 * frames (views, shards and vrt_multi included) stay the reference's shader at any setting -- so at D > 1 sample 0 of an
 * unjittered accumulation is no longer the frame. */
#define VRT_MAX_PATH_DEPTH 8
int vrt_set_path_depth(vrt_ctx *ctx, int depth);

/* Sun disc: soft shadows. The shader's sun is a point at infinity: every shadow ray runs along lightDir, and a shadow edge is the same
 * hard staircase at any number of samples. vrt_set_sun_disc gives the sun an angular size: tan_radius is the tangent of its angular
 * radius (the real sun: about 0.00465), default 0. It is context state, like the path depth. VRT_E_INVALID unless tan_radius is finite
 * and 0 <= tan_radius <= 1 (the previous value still holds).
 *
 * Who honours it: whoever honours the path depth, at every depth D in 1..8 -- the samples of VRT_MODE_FULL in the progressive
 * accumulation (vrt_accum_add in every form: corner, jitter, lens, adaptive, HDR) and in ray batches (vrt_shade_rays, _device, _hdr,
 * _hdr_device). vrt_dispatch* frames (views, shards and vrt_multi included) stay the reference's shader at any setting;
 * VRT_MODE_PRIMARY and VRT_MODE_PRIMARY_SHADOW ignore it, their accumulations included: they draw no random number. The value is one
 * of the inputs of an accumulation of VRT_MODE_FULL: a change restarts the sums at `first`, the same value set again changes
 * nothing; accumulations of the primary modes do not restart.
 *
 * At tan_radius == 0 nothing changes: no extra random number is drawn, the same kernels are launched, every byte is the same.
 * At tan_radius > 0 (all arithmetic float32, every operation rounded on its own, no contraction):
 *   1. The basis, once per launch, with the operations of normalize3 / len3 / cross3: with L = vrt_params.light_dir as given,
 *      ll = len3(L), Ln = normalize3(L), up = fabsf(Ln.z) < 0.999f ? (0,0,1) : (1,0,0) (cosineSampleHemisphere's choice),
 *      T = normalize3(cross3(up, Ln)), B = cross3(Ln, T). A zero or non-finite light_dir gives unspecified shading for the
 *      shadowed terms; the call still terminates.
 *   2. The rule applies inside pathTrace's loop, only at a vertex that casts a shadow ray: the opaque, non-emissive branch
 *      (comp:584-616) of a ray of depth d < D (at D = 1: d = 0).
 *   3. That vertex, in this order:
 *        u1 = rand(), then u2 = rand(), from the pixel's one initRNG stream, immediately before notInShadow -- hence before the
 *          two draws of the bounce direction;
 *        (dx, dy) = the concentric map of vrt_set_lens step 3 with lu = u1, lv = u2;
 *        s = tan_radius; v_i = (Ln_i + (s * dx) * T_i) + (s * dy) * B_i; L' = normalize3(v) * ll -- the length of lightDir keeps
 *          the meaning it has in the shader;
 *        lit = notInShadow(hitPoint + normal * 2e-3, L'), the shadow ray's set-up (comp:335-345) computed from L';
 *        ndotl' = max(dot(normal, L'), 0);
 *        the shader's direct term with lit and ndotl'; then the two bounce draws and everything after them, unchanged.
 *   4. What does not move: the translucent branch's unshadowed direct term (comp:547-572) keeps ndotl from L; sky, emission, the
 *      ambient term, (voxel ID, dist), the glass stack and the order in which the LIFO stack pops rays.
 *   5. Consequence: a pixel's stream carries four draws per shadowing vertex instead of two, so sample k is not sample k of the
 *      hard-shadow accumulation with a softened term: it is a different, equally valid sample. */
int vrt_set_sun_disc(vrt_ctx *ctx, float tan_radius);

/* Emitter sampling: next-event estimation towards emissive voxels. A voxel with a non-zero illumination byte lights a surface only
 * when a cosine-distributed bounce ray happens to hit it (the shader's `emission > 0 && depth > 0` branch, comp:575-581): indoors the
 * slowest-converging term of the image. vrt_set_emitter_sampling(ctx, 1) makes every vertex that casts a shadow ray also connect to a
 * random point on a random emitter, and in exchange drops what bounce rays find by accident. enable is 0 (default) or 1; anything
 * else is VRT_E_INVALID (the previous value still holds). It is context state, like the path depth and the sun disc.
 *
 * The emitter list. An emitter is a leaf of the current tree whose record has alpha byte > 0 and illumination byte > 0: exactly the
 * leaves for which the shader's `emission` is positive. An entry is the leaf's cube in tree (grid) coordinates, four int32
 * {lo.x, lo.y, lo.z, size}: its minimum corner and its edge length under the world bounds of vrt_params, split as the shader splits
 * them; a merged volume is one entry with size > 1. (A merged leaf whose box is no cube -- possible only where the bounds are no power
 * of two -- is listed as its unit cells; a box that holds no cell is not listed.) The order is ascending by (lo.x, lo.y, lo.z) and
 * does not depend on record order: a patched or compacted tree gives the list of a fresh upload of the same world. The list is made
 * lazily, by the first vrt_emitters call and by the first add or batch that honours sampling, after any change of the tree (upload,
 * patch, batch end, compaction) or of the bounds.
 *   vrt_emitters returns N and writes the first min(N, cap) entries to out (out may be NULL where cap is 0), whether or not sampling
 * is enabled; for N > VRT_MAX_EMITTERS it writes none. VRT_E_STATE before any upload and while a patch batch is open.
 *   With sampling on and N > VRT_MAX_EMITTERS every call that would honour sampling returns VRT_E_STATE with a message.
 *
 * Who honours it: exactly who honours the path depth and the sun disc -- the samples of VRT_MODE_FULL in vrt_accum_add in every form
 * (corner, jitter, lens, adaptive, HDR) and vrt_shade_rays, _device, _hdr, _hdr_device, at every D in 1..8, with any sun radius.
 * vrt_dispatch* frames, views, shards, vrt_multi and the two primary modes ignore it. The flag is one of the inputs of an accumulation
 * of VRT_MODE_FULL: a change restarts the sums at `first`, the same value set again changes nothing; accumulations of the primary
 * modes do not restart.
 *
 * Off, or N == 0: nothing changes -- no extra random number is drawn, the same kernels are launched, every byte is the same.
 * On with N > 0 (all arithmetic float32, every operation rounded on its own, no contraction). At every vertex that casts a shadow
 * ray -- the opaque, non-emissive branch (comp:584-616) of a ray of depth d < D -- after the sun's direct term (which follows the
 * sun's own two draws, if any) and before the two draws of the bounce direction:
 *   1. Four draws from the pixel's stream, in this order: u0 = rand(), uf = rand(), ua = rand(), ub = rand().
 *   2. The emitter: j = min((int)(u0 * (float)N), N - 1), with corner lo and sz = (float)size.
 *      The face: f = min((int)(uf * 6.0f), 5), ax = f >> 1, side = f & 1, a1 = (ax + 1) % 3, a2 = (ax + 2) % 3.
 *      The point q on it: q[ax] = (float)lo[ax] + (side ? sz : 0.0f), q[a1] = (float)lo[a1] + ua * sz, q[a2] = (float)lo[a2] + ub * sz.
 *   3. The connection: x = hitPoint + normal * 1e-1 (the bounce ray's origin, in grid units); w = q - x; r2 = dot3(w, w); if
 *      !(r2 > 0) nothing more happens; dir = w * (1 / sqrt(r2)); cs = dot3(normal, dir); cl = side ? -dir[ax] : dir[ax]; if
 *      !(cs > 0 && cl > 0) nothing is marched or added -- the four draws stay spent.
 *   4. The connection ray is the ray the bounce would make (make_ray, comp:604-615) with dir in place of the hemisphere direction:
 *      origin x, rayIOF n1, the same weight, tint = transmittedColor * surfaceColor, distanceInMedium 0, the last voxel as its
 *      medium, depth d + 1.
 *   5. It is marched with the shader's own hitMarching (the first hit). It contributes only if it hits and the hit cell lies in
 *      emitter j's cube: per axis lo <= hitMapPos < lo + size.
 *   6. Then the hit is evaluated as the shader evaluates any hit of a ray of depth >= 1, up to the emissive test: the distance in the
 *      medium (comp:499-501), the absorption (comp:512-516), the highlighted-voxel inversion, emission = props[1] * 10. If
 *      emission > 0:
 *        E_k  = tc'[k] * sc'[k] * emission * weight / PI    (the shader's own depth > 0 emissive term, comp:579)
 *        area = ((float)N * 6.0f) * (sz * sz)
 *        g    = ((cs * cl) * area) / (PI * r2)
 *        fc[k] = fc[k] + E_k * g
 *   7. In exchange a ray of depth >= 1 that hits an emissive voxel adds nothing and ends: the light would be counted twice.
 * What does not move: the depth-0 emissive term, the sky and ambient terms, the translucent branch, (voxel ID, dist), the order in
 * which the LIFO stack pops rays.
 * Consequences: the expectation of a sample equals that of the same sample with sampling off -- the two estimators integrate the same
 * quantity, one over direction, one over emitter area (the choice is uniform over emitters and over the six faces: unbiased, but
 * wasteful where emitter sizes differ much -- vrt_set_emitter_importance below). Sample k itself is a different, equally valid sample: the stream carries four more draws
 * per shadowing vertex. */
#define VRT_MAX_EMITTERS (1u << 20)
int vrt_set_emitter_sampling(vrt_ctx *ctx, int enable);
long vrt_emitters(vrt_ctx *ctx, int32_t *out, size_t cap);

/* Emitter importance: how a vertex picks from the emitter list. vrt_set_emitter_importance(ctx, VRT_EMIT_POWER) replaces the uniform
 * choice of steps 1-2 above -- one of N emitters, one of six faces -- by one that picks the emitter in proportion to its power and the
 * face among those turned towards the vertex. mode is VRT_EMIT_UNIFORM (default) or VRT_EMIT_POWER; anything else is VRT_E_INVALID
 * (the previous value still holds). It is context state, like the flag, and vrt_set_emitter_sampling keeps its 0 / 1 contract. The
 * mode is read only where sampling is on and the list is not empty: otherwise the same kernels run and the same bytes come out at
 * either mode. Exactly the callers that honour the flag honour the mode (see "Who honours it" above, at every D and any sun radius),
 * and it is one of the inputs of an accumulation of VRT_MODE_FULL exactly as the flag is: a change restarts the sums at `first`, the
 * same value set again changes nothing; accumulations of the primary modes do not restart. With VRT_EMIT_UNIFORM every launch and
 * every byte is that of the rule above.
 *
 * Weights. Entry j of the list with the record words (w0, w1) of its leaf, as the shader's decoder reads them, has the integer weight
 *     W_j = size^2 * illum * (R + G + B),   illum = (w1 >> 8) & 0xff,   R, G, B the low three bytes of w0;
 * a unit cell of a merged leaf that is no cube takes that leaf's record. With C_j the inclusive prefix sum and Wtot = C_{N-1} the
 * thresholds are, in exact integers,
 *     Wtot > 0:   T_j = (j + 1) + floor(C_j * (2^24 - N) / Wtot)
 *     Wtot == 0:  T_j = floor((j + 1) * 2^24 / N)
 * so that T is strictly increasing, T_{N-1} = 2^24 and every emitter holds at least one of the 2^24 ticks: a black or highlighted
 * emitter is never given probability zero, and the estimator stays unbiased. The table is made and uploaded with the list, by the same
 * lazy rule.
 *   vrt_emitter_cdf behaves as vrt_emitters does: it returns N and writes the first min(N, cap) thresholds T_j to out, in the list's
 * order (out may be NULL where cap is 0), whatever the flag and the mode; for N > VRT_MAX_EMITTERS it writes none. VRT_E_STATE before
 * any upload and while a patch batch is open. With sampling on, VRT_EMIT_POWER set and N > VRT_MAX_EMITTERS the calls that honour
 * sampling return the same VRT_E_STATE as with VRT_EMIT_UNIFORM.
 *
 * Per vertex (all arithmetic float32, every operation rounded on its own, no contraction), at every vertex that casts a shadow ray, at
 * the position the uniform rule occupies; the four draws u0, uf, ua, ub are taken in the same order:
 *   1. The emitter: t = min((uint32)(u0 * 16777216.0f), 16777215) (rand() can return exactly 1.0f: the clamp is for that case);
 *      j = the smallest index with T_j > t; ticks = T_j - T_{j-1} with T_{-1} = 0; p = (float)ticks * 0x1p-24f. Corner lo and
 *      sz = (float)size as before.
 *   2. The faces: x = hitPoint + normal * 1e-1. Per axis k in the order 0, 1, 2 the low face is visible if x[k] < (float)lo[k], the
 *      high face if x[k] > (float)lo[k] + sz, otherwise neither. m = the number of visible faces, 0 to 3. m == 0 (x inside the cube's
 *      slab on every axis): nothing more happens, the four draws stay spent. Otherwise i = min((int)(uf * (float)m), m - 1), and the
 *      i-th visible face in axis order gives ax and side; a1, a2 and the point q on the face are those of step 2 above.
 *   3. Steps 3 to 6 above, word for word: w, r2, dir, cs, cl, the !(cs > 0 && cl > 0) test, the connection ray, the march, the in-cube
 *      test, the hit's evaluation, E_k -- with the weight
 *        g = ((cs * cl) * ((float)m * (sz * sz))) / ((PI * r2) * p)
 *   4. Step 7 above is unchanged: a ray of depth >= 1 that hits an emissive voxel adds nothing and ends.
 * Consequences: the same expectation as VRT_EMIT_UNIFORM and as sampling off; a bright emitter is reached in proportion to its
 * share of the list's power instead of once in N vertices, and no connection is drawn towards a face turned away. The threshold
 * search is a lower bound of ceil(log2 N) steps on a global table of at most 4 MB. Multiple importance sampling with the bounce:
 * vrt_set_emitter_mis below. Not done: faces by projected solid angle, the stack-free opaque routes, vrt_multi. */
#define VRT_EMIT_UNIFORM 0
#define VRT_EMIT_POWER   1
int vrt_set_emitter_importance(vrt_ctx *ctx, int mode);
long vrt_emitter_cdf(vrt_ctx *ctx, uint32_t *out, size_t cap);

/* Emitter MIS: weigh the emitter connection against the bounce ray. With VRT_EMIT_POWER alone a bounce ray that finds an emitter adds
 * nothing and all emitted light arrives through the connection, whose weight g = cs * cl * (m * size^2) / (PI * r2 * p) nothing bounds:
 * at a vertex 0.1 off a surface that an emitter touches r2 is a few hundredths and g runs into the tens -- fireflies that never average
 * out, just where the dropped bounce ray was the good estimator. vrt_set_emitter_mis(ctx, 1) keeps both samples and weighs each by the
 * balance heuristic, the same function of (vertex, direction) on both sides; the two weights sum to one. enable is 0 (default) or 1;
 * anything else is VRT_E_INVALID (the previous value still holds). It is context state, and vrt_set_emitter_importance keeps its 0 / 1
 * contract. The flag is read only where vrt_set_emitter_sampling is on, the emitter list is not empty and the mode is VRT_EMIT_POWER:
 * in every other case the same kernels launch and the same bytes come out at either value. Exactly the callers that honour the emitter
 * flag and the mode honour this flag (vrt_accum_add of VRT_MODE_FULL in every form, vrt_shade_rays and its three siblings, at every D
 * and any sun radius); frames, views, shards and vrt_multi ignore it. Where it is read it is one of the inputs of an accumulation of
 * VRT_MODE_FULL: a change restarts the sums at `first`, the same value set again changes nothing. Where it is not read a change does
 * not restart, and accumulations of the primary modes never do.
 *
 * Per launch: inv_power = Wtot > 0 ? (float)(1.0 / (double)Wtot) : 0.0f, with Wtot the sum of the list's integer weights W_j, kept when
 * the table of thresholds is made.
 *
 * The densities (all arithmetic float32, every operation rounded on its own, no contraction). emit_mis_density(x, dir, cs, hit), for a
 * ray from x in the direction dir whose march ended in `hit` (point, axis, cell `map`, leaf words w0, w1), cs the cosine at x:
 *     v = hit.point - x;  r2 = dot3(v, v);  cl = fabsf(dir[hit.axis])
 *     axis k is visible if x[k] < (float)map[k] || x[k] > (float)map[k] + 1.0f;  m = the number of visible axes
 *     w = illum * (R + G + B), of the hit voxel's words exactly as W_j reads them
 *     pl = (m == 0 || !(cl > 0)) ? 0 : ((((float)w * inv_power) * r2) / ((float)m * cl))
 *     pb = (cs > 0 ? cs : 0) / PI
 * pl is the power rule's solid-angle density computed from the hit alone -- the bounce side knows its hit, not the list entry -- with
 * two stated simplifications. The emitter's probability is w / Wtot (the size^2 of W_j cancels against the face's area) and ignores
 * the table's one-tick floor: by the formula for T_j the true p is at least (W_j / Wtot) * (1 - N * 2^-24). And m is that of the hit
 * cell, not of the list's cube; it can only be larger. So the function is exact for single voxels and under-trusts connections to a
 * merged emitter by at most m_cell / m_cube <= 3. The weights need only be the same function on both sides and sum to one.
 *
 * The connection: VRT_EMIT_POWER's steps 1 to 3, word for word, up to and including emission > 0 and g. Then pl and pb of the
 * connection's own hit, its x, its dir and its cs. !(pl > 0): nothing is added. Otherwise wn = pl / (pl + pb) and
 *     fc[k] = fc[k] + (E_k * g) * wn.
 * The four draws and their order are unchanged.
 * The bounce: when the bounce ray is made, cb = dot3(normal, bd) is kept. Where that ray (depth >= 1) hits a voxel with emission > 0:
 * pl and pb of x = the ray's origin, dir = its direction, cs = cb and this hit; wb = !(pl > 0) ? 1 : pb / (pl + pb);
 *     fc[k] = fc[k] + (tc[k] * sc[k] * emission * weight / PI) * wb
 * and the path ends there, as it does with the flag off.
 * Consequences: the expectation is that of VRT_EMIT_POWER, VRT_EMIT_UNIFORM and sampling off. With g = pb / pl the connection's term is
 * E * pb / (pl + pb), at most E (up to the two simplifications: at most 1 / (1 - N * 2^-24) times that, and the float32 difference
 * between the sampled point and the marched hit). A black emitter (w == 0) is carried by the bounce alone, at weight 1. Sample k at
 * flag 1 draws the same numbers as at flag 0. One case is not exactly unbiased: a vertex whose x lies inside an emitter's own list cube
 * but outside the hit cell -- the connection cannot be drawn there (m of the cube is 0), yet the bounce is weighted below 1; it arises
 * only for rays started inside solids. Not done: MIS under VRT_EMIT_UNIFORM (its density needs the cube's size at the hit), a
 * hit-to-list lookup that would make m and the ticks exact, the power heuristic, the stack-free opaque routes, vrt_multi. */
int vrt_set_emitter_mis(vrt_ctx *ctx, int enable);

/* Adaptive accumulation: stop sampling pixels whose mean has converged. vrt_accum_begin_adaptive is vrt_accum_begin_ex (same
 * modes, VRT_ACCUM_JITTER, the lens as context state) plus a stopping rule, which belongs to the accumulation. VRT_E_INVALID
 * unless 2 <= min_samples <= max_samples <= 2^24 and tolerance <= 65535, or for what vrt_accum_begin_ex refuses.
 *
 * The rule. Pixel p holds n samples; for each, L_i = R_i + G_i + B_i (its three unorm8 bytes); S = sum L_i, Q = sum L_i^2.
 * The pixel is active -- it takes the next round's sample -- iff
 *     n < min_samples  ||  (n < max_samples  &&  256 * (n*Q - S^2) > tolerance^2 * n^2 * (n - 1))
 * in exact integer arithmetic: sampling goes on while the standard error of the mean of L exceeds tolerance / 16 units of L.
 * tolerance 0 stops a pixel once all its samples are identical, after at least min_samples.
 *
 * Rounds. vrt_accum_add(ctx, n, &total) runs n rounds: in round r (counted from the first round in the sums) every pixel
 * active at the start of the round adds sample first + r, exactly the sample a plain accumulation of the same mode, flags and
 * lens would add at that index. A stopped pixel never takes another sample, so pixels only drop out, and each pixel's fate
 * depends on its own samples alone: 3 + 5 rounds equal 8 rounds equal 8 x 1 round, and min_samples == max_samples == N is the
 * plain accumulation of N samples byte for byte. `total` and the 2^24 cap count rounds. The restart rule is unchanged; a
 * restart makes every pixel active again with zero samples.
 *
 * vrt_accum_resolve / _resolve_device give each pixel (sum + n_p / 2) / n_p with its own count n_p; the id_dist image and the
 * display pass are as above.
 * vrt_accum_counts: synchronous; writes the per-pixel counts [H][W] to out_counts (may be NULL) and returns the number of active
 * pixels (>= 0), or VRT_E_STATE before any begin or on a non-adaptive accumulation. Before the first round every pixel is active
 * with zero samples; a restart that the next add will make is not yet seen. */
int vrt_accum_begin_adaptive(vrt_ctx *ctx, int width, int height, int mode, uint32_t first_sample, uint32_t flags,
                             uint32_t min_samples, uint32_t max_samples, uint32_t tolerance);
int vrt_accum_counts(vrt_ctx *ctx, uint32_t *out_counts);

/* HDR accumulation: float64 sums of the samples' unclamped colours, a float resolve and a tone map. The accumulations above
 * average the unorm8 bytes, so every sample brighter than 1 -- an emitter (comp:575-581: colour * light * 10), the sky behind a
 * bounce (comp:493: sky * 3 / PI) -- is clamped before it enters the mean: mean(min(c, 1)), where a still wants min(mean(c), 1).
 *
 * vrt_accum_keep_hdr(ctx, 1) makes the accumulations begun after it keep HDR sums too. It is context state, like the lens, read
 * by the next vrt_accum_begin / _begin_ex / _begin_adaptive; it is not part of the restart rule, and changing it leaves a running
 * accumulation as it was begun. Default 0. VRT_E_INVALID unless enable is 0 or 1.
 *
 * All arithmetic below: every operation rounded on its own, no contraction.
 *  1. The HDR sample. Sample k's HDR value is the three floats c the sample's unorm8 store receives (the shader's finalColor.rgb,
 *     comp:645), each mapped by h(c) = min(max(0, c), 65504.0f) with min(a, b) = b < a ? b : a and max(a, b) = a < b ? b : a --
 *     the conventions of the unorm8 store, the zero first, so that NaN goes to +0 (0 < NaN is false). unorm8(h(c)) == unorm8(c)
 *     for every float c (a NaN stores byte 0). The same in all three modes and for the corner, jittered and thin-lens samples.
 *  2. The sums. An accumulation begun with HDR on keeps everything it keeps otherwise -- the integer sums, and when adaptive the
 *     counts and Q; the adaptive rule stays on the bytes -- and three float64 sums per pixel, which start at +0.0 and take
 *     sum = sum + (double)h(c) once per sample the pixel takes, in sample-index order. They continue across vrt_accum_add calls
 *     (3 + 5 samples equal 8 bit for bit); a restart zeroes them. float64: a float32 sum stalls long before the 2^24-sample cap,
 *     and m * c is exact in a double for a float c and m <= 2^24, so a pixel whose every sample is the same float adds
 *     (double)c * k for k samples at once and gets the k sequential adds' result.
 *  3. The resolve. mean = (float)(sum / (double)n_p) per channel, n_p the pixel's own count (the accumulation's when not adaptive).
 *  4. The tone map, per channel on the float mean x with exposure e:
 *        VRT_TONEMAP_CLAMP     y = e * x
 *        VRT_TONEMAP_REINHARD  x' = e * x;  y = x' / (1.0f + x')
 *     and the bytes are unorm8(y), alpha 255. tm == NULL: VRT_TONEMAP_CLAMP with exposure 1.
 *
 * vrt_accum_resolve_hdr   the float means [H][W][3], the tone-mapped rgba8 [H][W][4] and the display pass of vrt_denoise on those
 *                         bytes with the accumulation's id_dist image (as vrt_accum_resolve runs it), into host buffers (any may
 *                         be NULL); synchronous.
 * vrt_accum_resolve_hdr_device  the same into device buffers, enqueued on `stream` (NULL: the context's), ordered against the adds
 *                         as vrt_accum_resolve_device is; d_shown_rgba8 needs d_rgba8.
 * VRT_E_STATE: no begin, no sample yet, or the accumulation was begun without HDR. VRT_E_INVALID: an unknown op, an exposure that
 * is not finite or not > 0, d_shown_rgba8 without d_rgba8.
 * With HDR off nothing changes: behaviour, buffers and kernels are those of the accumulations above. With HDR on,
 * vrt_accum_resolve, _resolve_device and vrt_accum_counts return exactly what the same accumulation without HDR returns; the
 * accumulation takes 36 bytes per pixel more (the sums, and the frame's float colour for the pixels whose samples all equal it).
 * Frames, views, shards and vrt_multi have no float output; a ray batch's float mean comes from vrt_shade_rays_hdr / _hdr_device (below). */
int vrt_accum_keep_hdr(vrt_ctx *ctx, int enable);
#define VRT_TONEMAP_CLAMP 0
#define VRT_TONEMAP_REINHARD 1
typedef struct vrt_tonemap { int32_t op; float exposure; } vrt_tonemap;
int vrt_accum_resolve_hdr(vrt_ctx *ctx, float *out_rgb, const vrt_tonemap *tm, uint8_t *out_rgba8, uint8_t *out_shown_rgba8);
int vrt_accum_resolve_hdr_device(vrt_ctx *ctx, void *d_rgb, const vrt_tonemap *tm, void *d_rgba8, void *d_shown_rgba8, void *stream);

/* Ray batches in HDR: vrt_shade_rays with the mean of the samples' unclamped colours -- what a light probe, an environment map or
 * a mirror pass of an emitter wants, where vrt_shade_rays averages clamped bytes. Rays, Direction, width (for the random numbers
 * only), State -- no camera, accumulation, lens, ray table, miss mask or tile order is read or written -- and the stream ordering
 * are those of vrt_shade_rays / vrt_shade_rays_device. vrt_accum_keep_hdr has no bearing on these calls.
 *
 * All arithmetic below: every operation rounded on its own, no contraction.
 *  1. The HDR sample. Sample k of ray i is the three floats c its unorm8 store receives, each through
 *     h(c) = min(max(0, c), 65504.0f): point 1 of vrt_accum_keep_hdr above, unchanged (NaN goes to +0).
 *  2. The sums. Three float64 sums per ray. They start at +0.0, or -- device form, d_sums not NULL -- at the three doubles of ray i
 *     in d_sums (n x 3 float64, the caller's, read and written). VRT_MODE_FULL: sum = sum + (double)h(c) once per sample, in the
 *     order first_sample, first_sample + 1, ... (indices modulo 2^32). VRT_MODE_PRIMARY and _PRIMARY_SHADOW draw no random number,
 *     so one sample is traced and sum = sum + (double)h(c) * (double)n_samples, one multiply and one add: m * h(c) is exact in a
 *     double for m <= 2^24, so from a sum that holds m * h(c) with m + n_samples <= 2^24 this is the n_samples sequential adds'
 *     result exactly. The sums are written back to d_sums when it is given.
 *  3. The mean. out_rgb[i] = (float)(sum / (double)(n_prior + n_samples)) per channel, n x 3 floats. n_prior is the number of
 *     samples the caller says d_sums already holds; the host form has no sums, so its n_prior is 0.
 *  4. The tone map. out_rgba8 (n x 4 bytes) is the mean through the tone map of vrt_accum_resolve_hdr: the same vrt_tonemap, the
 *     same two operators, unorm8 of the result, alpha 255; tm == NULL: VRT_TONEMAP_CLAMP with exposure 1. With n_samples == 1,
 *     n_prior == 0 and tm == NULL these are vrt_shade_rays's bytes.
 *  5. out_id_dist: exactly what vrt_shade_rays stores.
 * Progressive use: the library keeps no state between calls. Call k + 1 passes first_sample + (samples so far) and
 * n_prior = (samples so far) with the same d_sums, zeroed before the first call: 3 + 5 samples equal 8 in one call bit for bit,
 * in the sums and in the mean.
 * Errors: everything vrt_shade_rays refuses (for "both outputs NULL": all of out_rgb, out_rgba8 and out_id_dist NULL in the host
 * form; all of d_rgb, d_rgba8, d_id_dist and d_sums NULL in the device form -- d_sums alone is an output), and VRT_E_INVALID for
 * n_prior != 0 with d_sums == NULL, n_prior + n_samples > 2^24, an unknown tm->op, an exposure that is not finite or not > 0.
 * n == 0 (with valid arguments otherwise) does nothing and returns VRT_OK.
 * vrt_shade_rays_hdr: HOST buffers, synchronous, staged through the device buffers vrt_shade_rays keeps (n x 12 bytes more for
 * out_rgb; they grow by the same rule and never shrink). vrt_shade_rays_hdr_device: DEVICE buffers, enqueued on `stream`. */
int vrt_shade_rays_hdr(vrt_ctx *ctx, size_t n, const float *origins, int origin_stride, const float *dirs, int width, int mode,
                       uint32_t first_sample, uint32_t n_samples, const vrt_tonemap *tm,
                       float *out_rgb, uint8_t *out_rgba8, int32_t *out_id_dist);
int vrt_shade_rays_hdr_device(vrt_ctx *ctx, size_t n, const void *d_origins, int origin_stride, const void *d_dirs, int width, int mode,
                              uint32_t first_sample, uint32_t n_samples, uint32_t n_prior, void *d_sums, const vrt_tonemap *tm,
                              void *d_rgb, void *d_rgba8, void *d_id_dist, void *stream);

/* Column-major mat4 x2 + vec4, exactly the std140 Camera block (comp:17-21). */
int vrt_set_camera(vrt_ctx *ctx, const float inv_projection[16], const float inv_view[16],
                   const float camera_pos[4]);

/* Synchronous whole-frame dispatch into HOST buffers:
 *   out_rgba8   width*height*4 bytes  (image binding 0, rgba8; row 0 = bottom, v = -1)
 *   out_id_dist width*height*2 int32  (image binding 3, rg32i = voxelID, dist)
 * Either pointer may be NULL. Any width/height >= 1 is accepted. */
int vrt_dispatch(vrt_ctx *ctx, int width, int height, int mode, uint8_t *out_rgba8, int32_t *out_id_dist);

/* The same, asynchronous and double-buffered: the call enqueues the trace and the two copies to the host on one of two
 * internal lanes (a stream and a pair of device images each) and returns a ticket (0 or 1); vrt_dispatch_wait(ticket)
 * blocks until that frame's host buffers are complete. While frame i crosses PCIe, frame i+1 is traced: a loop that
 * keeps two frames in flight runs at the copy's rate (12 B/pixel over PCIe: 24.9 MB, >= 0.40 ms at the link's 63 GB/s
 * for a 1080p frame -- no arrangement of copies brings both images of that frame to the host faster) instead of trace +
 * copy. The host buffers should be pinned (vrt_host_alloc): into pageable memory the runtime stages the copy and the
 * call blocks for most of it. At most two frames in flight: a third call waits for the older ticket itself. */
int vrt_dispatch_async(vrt_ctx *ctx, int width, int height, int mode, uint8_t *out_rgba8, int32_t *out_id_dist, int *ticket);
int vrt_dispatch_wait(vrt_ctx *ctx, int ticket);
/* page-locked host memory for those buffers (hipHostMalloc / hipHostFree) */
int vrt_host_alloc(vrt_ctx *ctx, size_t bytes, void **host_ptr);
int vrt_host_free(vrt_ctx *ctx, void *host_ptr);

/* Stream-ordered dispatch into DEVICE buffers laid out as full frames; only
 * rows [row_begin, row_end) are traced and written (row sharding across GPUs).
 * stream: a hipStream_t, or NULL for the context's own stream. Returns after
 * enqueueing. */
int vrt_dispatch_rows(vrt_ctx *ctx, int width, int height, int row_begin, int row_end, int mode,
                      void *d_rgba8, void *d_id_dist, void *stream);

/* Interleaved row-tile sharding: the frame is cut into tiles of tile_rows rows;
 * shard s of n_shards owns tiles t with t % n_shards == s. Output buffers are
 * COMPACT: the shard's tiles back to back in tile order (each W*tile_rows
 * pixels, the last one possibly shorter). */
int vrt_dispatch_shard(vrt_ctx *ctx, int width, int height, int tile_rows, int shard, int n_shards, int mode,
                       void *d_rgba8, void *d_id_dist, void *stream);
/* rows (and pixels = rows*width) a shard owns under that scheme */
int vrt_shard_rows(int height, int tile_rows, int shard, int n_shards);
/* The same tiles written at their place in a FULL frame (width*height pixels) instead of a compact buffer: the frame
 * may live on this device, on a peer device whose memory this one can reach (hipDeviceEnablePeerAccess, or an
 * allocation opened with vrt_ipc_open in another process) -- the shards of one frame then land in ONE framebuffer
 * with no gather step: the kernels' own stores cross xGMI. */
int vrt_dispatch_tiles(vrt_ctx *ctx, int width, int height, int tile_rows, int shard, int n_shards, int mode,
                       void *d_frame_rgba8, void *d_frame_id_dist, void *stream);

/* Device memory that other processes of the node can map (one process per GPU: the frame lives on one rank, the
 * others store into it). vrt_device_alloc is hipMalloc on the context's device (zero-filled); vrt_ipc_export fills a
 * 64-byte handle another process passes to vrt_ipc_open, which returns the address of the same memory in ITS address
 * space (on its context's device: peer access over xGMI); vrt_ipc_close unmaps it. Needs
 * HSA_ENABLE_IPC_MODE_LEGACY=0 (dmabuf handles) in both processes. */
#define VRT_IPC_HANDLE_BYTES 64
int vrt_device_alloc(vrt_ctx *ctx, size_t bytes, void **d_ptr);
int vrt_device_free(vrt_ctx *ctx, void *d_ptr);
/* synchronous copies between such memory and the host, after the work enqueued on `stream` (NULL: the context's) */
int vrt_device_read(vrt_ctx *ctx, const void *d_ptr, void *host, size_t bytes, void *stream);
int vrt_device_write(vrt_ctx *ctx, void *d_ptr, const void *host, size_t bytes, void *stream);
/* Device-to-device copy ordered on `stream` (NULL: the context's), asynchronous. Either pointer may be a mapping of another
 * rank's memory (vrt_ipc_open) or another device's (vrt_multi): how a rank hands a finished block of rows -- e.g. its band
 * of the DISPLAYED image after vrt_denoise -- to the rank that shows it. */
int vrt_device_copy(vrt_ctx *ctx, void *d_dst, const void *d_src, size_t bytes, void *stream);
int vrt_ipc_export(vrt_ctx *ctx, void *d_ptr, uint8_t handle[VRT_IPC_HANDLE_BYTES]);
int vrt_ipc_open(vrt_ctx *ctx, const uint8_t handle[VRT_IPC_HANDLE_BYTES], void **d_ptr);
int vrt_ipc_close(vrt_ctx *ctx, void *d_ptr);
/* Stream-ordered flags in device memory (a uint32 per flag): vrt_stream_write_flag makes `stream` store `value`
 * once everything enqueued before it has finished; vrt_stream_wait_flag makes `stream` wait until *d_flag >= value.
 * With the flag in an IPC-mapped allocation this is how a producer rank tells the consumer rank "my tiles of frame i
 * have landed" (and the consumer tells it "buffer k is free again") without the host or a collective in the loop. */
int vrt_stream_write_flag(vrt_ctx *ctx, void *d_flag, uint32_t value, void *stream);
int vrt_stream_wait_flag(vrt_ctx *ctx, void *d_flag, uint32_t value, void *stream);

/* ---- several GPUs behind one handle (reference: one GL context, src/main.cpp:432-474) -------------------------------
 * vrt_create_multi(n, device_ids) makes one context per device in THIS process (no Python, no launcher) and enables
 * peer access from every device to device_ids[0]. Scene, camera and uniforms are replicated by the vrt_multi_* setters.
 * vrt_multi_dispatch traces one frame, the devices sharing it by interleaved tile_rows-row tiles, into full-frame DEVICE
 * buffers on device_ids[0] (vrt_multi_frame_alloc): delivery VRT_DELIVER_PEER_STORE lets every device's kernel store its
 * tiles straight into those buffers (peer mappings over xGMI, no gather); VRT_DELIVER_GATHER traces into per-device
 * compact shard buffers and lets device 0 pull and un-interleave them with one copy kernel per image (reads over xGMI).
 * Returns after enqueueing; vrt_multi_synchronize waits for all devices. The frame is complete on device_ids[0] once
 * the call's work on stream vrt_multi_stream(m) has finished. */
typedef struct vrt_multi vrt_multi;
#define VRT_DELIVER_PEER_STORE 0
#define VRT_DELIVER_GATHER 1
int vrt_create_multi(int n_devices, const int *device_ids, vrt_multi **out);
void vrt_destroy_multi(vrt_multi *m);
const char *vrt_multi_last_error(const vrt_multi *m);   /* m may be NULL: the last failed vrt_create_multi on this thread */
int vrt_multi_devices(const vrt_multi *m);
vrt_ctx *vrt_multi_context(vrt_multi *m, int i);        /* the i-th device's context (for per-device calls) */
int vrt_multi_upload_octree(vrt_multi *m, const uint8_t *texels, size_t used_bytes, uint32_t tex_dim);
int vrt_multi_set_camera(vrt_multi *m, const float inv_projection[16], const float inv_view[16], const float camera_pos[4]);
int vrt_multi_set_params(vrt_multi *m, const vrt_params *p);
int vrt_multi_frame_alloc(vrt_multi *m, int width, int height, void **d_rgba8, void **d_id_dist);   /* on device_ids[0] */
int vrt_multi_frame_free(vrt_multi *m, void *d_rgba8, void *d_id_dist);
int vrt_multi_dispatch(vrt_multi *m, int width, int height, int tile_rows, int mode, int delivery, void *d_rgba8,
                       void *d_id_dist);
/* The frame the reference SHOWS -- dispatch (src/main.cpp:946) then the display pass (:951-967, shaders/quad.frag) -- over the
 * devices of m: the frame is cut into one band of rows per device (multiples of 8), every device traces its band plus a
 * 20-row halo on either side (the display pass reads up to 20 rows away), filters that sub-image and copies the band's
 * displayed rows into d_shown_rgba8 (W*H packed rgba8 on device_ids[0], e.g. from vrt_multi_frame_alloc). Only the displayed
 * image crosses devices. Returns after enqueueing; the frame is complete once vrt_multi_stream(m)'s work has finished. */
int vrt_multi_dispatch_frame(vrt_multi *m, int width, int height, int mode, void *d_shown_rgba8);
int vrt_multi_synchronize(vrt_multi *m);
void *vrt_multi_stream(vrt_multi *m);                    /* device_ids[0]'s stream: consumers of the frame order themselves after it */

/* EXTENSION: up to 4 views of the uploaded scene in ONE launch -- frames that are known together (a stereo pair,
 * the next frames of a camera path, the views of a rig). Each view brings its own camera block (what
 * vrt_set_camera takes) and its own compact shard buffers (what vrt_dispatch_shard takes); scene, uniforms and the
 * row sharding are shared. Pixels are those of n_views separate vrt_dispatch_shard calls; the launch is shorter
 * than their sum because one view's last waves no longer drain an otherwise idle chip. DEVICE pointers,
 * stream-ordered, returns after enqueueing. */
typedef struct vrt_view {
    float inv_projection[16];
    float inv_view[16];
    float camera_pos[4];
    void *d_rgba8;      /* rows_of_shard * width packed rgba8, or NULL */
    void *d_id_dist;    /* rows_of_shard * width int2 (voxelID, dist), or NULL */
} vrt_view;
int vrt_dispatch_views(vrt_ctx *ctx, int width, int height, int tile_rows, int shard, int n_shards, int mode,
                       const vrt_view *views, int n_views, void *stream);

/* Repeats vrt_dispatch_rows `iters` times on `stream` with a hipEvent pair
 * around every launch and returns each launch's duration (ms) in ms_out[iters].
 * Blocks until done. */
int vrt_dispatch_timed(vrt_ctx *ctx, int width, int height, int row_begin, int row_end, int mode,
                       void *d_rgba8, void *d_id_dist, void *stream, int iters, float *ms_out);

/* The display pass that consumes the two images in the reference's frame loop (the fullscreen
 * quad drawn by src/main.cpp:951-967 with shaders/quad.frag:22-83): ID-aware box blur, radius
 * clamp(int(200/sqrt(max(1,dist))), 1, 20), only pixels with the centre's voxelID contribute.
 * DEVICE pointers, full frames (W*H packed rgba8 / W*H int2), stream-ordered; out must not alias in. */
int vrt_denoise(vrt_ctx *ctx, int width, int height, const void *d_rgba8, const void *d_id_dist, void *d_out_rgba8,
                void *stream);
/* the same through HOST buffers, synchronous */
int vrt_denoise_host(vrt_ctx *ctx, int width, int height, const uint8_t *rgba8, const int32_t *id_dist,
                     uint8_t *out_rgba8);

/* The display pass in HDR: the same ID-aware blur on a FLOAT image, then the tone map. vrt_denoise reads rgba8, so the shown image
 * of an HDR accumulation (vrt_accum_resolve_hdr's out_shown_rgba8) is tone map, quantise, then blur: an emitter sample of 10.0 is
 * clamped to 1.0 before its face's neighbours average it, and blur(tonemap(x)) != tonemap(blur(x)). These calls filter the floats
 * and map the filtered estimate; they also hand out the filtered floats themselves, to save or to grade.
 *
 * All arithmetic below is float32: every operation rounded on its own, no contraction.
 *  1. The input value. Every float read from the input image [H][W][3] goes through h(c) = min(max(0, c), 65504.0f), with the min /
 *     max conventions of vrt_accum_keep_hdr point 1: NaN -> +0, a negative value (and -0) -> +0, +Inf -> 65504; subnormals are
 *     kept. The centre pixel, every tap, and the pixels that pass through alike.
 *  2. The filter, quad.frag:22-83 with screenTexture that float image. A pixel whose voxel ID is 0 yields h(c) per channel.
 *     Otherwise R = clamp(int(200.0f / sqrtf((float)max(1, dist))), 1, 20); sum_ch = 0 and count = 0; then, over the taps of the
 *     (2R+1)^2 window that lie inside the image and whose voxel ID equals the centre's, y outer, x inner:
 *     sum_ch = sum_ch + h(c_ch), count = count + 1.0f; and f_ch = sum_ch / max(count, 1.0f).
 *  3. The outputs; either may be NULL, not both. out_rgb [H][W][3] receives f. out_rgba8 [H][W][4] receives unorm8(tonemap(f)),
 *     alpha 255, with the vrt_tonemap of vrt_accum_resolve_hdr: the same two operators, the same validation, tm == NULL means
 *     VRT_TONEMAP_CLAMP with exposure 1.
 *  4. Identity with the byte pass. Where every input float is byte / 255.0f of an rgba8 image whose alpha is 255 (what every image
 *     this library writes) and tm == NULL, out_rgba8 equals vrt_denoise's output on that image byte for byte: the staged floats
 *     are the same, 1.0f * x is exact, and unorm8(byte / 255.0f) is the byte. (vrt_denoise copies a pass-through pixel's alpha;
 *     this pass always writes 255.)
 * The sums cannot overflow: at most 1681 taps of at most 65504. Options, tile scheduling and VRT_OPT_DISPLAY_KERNEL act on this
 * pass as on vrt_denoise, from scheduling state of its own: neither pass changes the other's measurements or tile order. (The
 * states of all launch shapes share one pool of 16 per context; once a context has used more shapes than that, a new shape of
 * either pass recycles the least recently used state of any, which only costs that shape its measured order.)
 *
 * vrt_denoise_hdr       DEVICE pointers, full frames (W*H x 3 floats / W*H int2 / W*H x 3 floats / W*H packed rgba8), stream-ordered.
 *                       VRT_E_INVALID: d_rgb or d_id_dist NULL, both outputs NULL, d_out_rgb == d_rgb, an unknown tm->op, an exposure
 *                       that is not finite or not > 0, a frame size vrt_denoise refuses.
 * vrt_denoise_hdr_host  the same through HOST buffers, synchronous; staged through device buffers the context keeps (24 bytes per
 *                       pixel for the two float images; like the other host forms' they grow and never shrink).
 * vrt_accum_resolve_hdr_shown  the filter on an HDR accumulation: the input is its float mean -- exactly what vrt_accum_resolve_hdr
 *                       writes to out_rgb -- with the accumulation's id_dist image. HOST buffers (either may be NULL, not both),
 *                       synchronous. Errors: those of vrt_accum_resolve_hdr (VRT_E_STATE: no begin, no sample yet, begun without
 *                       HDR; VRT_E_INVALID: the tone map), VRT_E_INVALID for both outputs NULL.
 * vrt_accum_resolve_hdr_shown_device  the same into DEVICE buffers, enqueued on `stream` (NULL: the context's), ordered against the
 *                       adds as vrt_accum_resolve_hdr_device is.
 * The mean passes through 12 bytes per pixel of device memory that belong to the accumulation and are allocated by the first of
 * these two calls: an HDR accumulation that never makes one takes what it took. vrt_accum_resolve_hdr's three outputs are not
 * changed by them. Frames, views and vrt_multi have no float output, so vrt_dispatch_frame's display pass stays the byte pass. */
int vrt_denoise_hdr(vrt_ctx *ctx, int width, int height, const void *d_rgb, const void *d_id_dist, const vrt_tonemap *tm,
                    void *d_out_rgb, void *d_out_rgba8, void *stream);
int vrt_denoise_hdr_host(vrt_ctx *ctx, int width, int height, const float *rgb, const int32_t *id_dist, const vrt_tonemap *tm,
                         float *out_rgb, uint8_t *out_rgba8);
int vrt_accum_resolve_hdr_shown(vrt_ctx *ctx, const vrt_tonemap *tm, float *out_shown_rgb, uint8_t *out_shown_rgba8);
int vrt_accum_resolve_hdr_shown_device(vrt_ctx *ctx, const vrt_tonemap *tm, void *d_shown_rgb, void *d_shown_rgba8, void *stream);

/* EXTENSION: guide planes -- per pixel of an accumulation (or per ray of a batch) the first hit's normal, albedo, depth and coverage,
 * averaged over the samples: the feature buffers a denoiser or a compositor asks for beside the colour. Features, not radiance: no
 * shading, no shadow ray, no random number.
 *
 * The guide of one sample of one pixel is taken from the depth-0 march of that sample's own ray: the ray sample k of the
 * accumulation starts from -- the pixel's corner, the jittered ray of VRT_ACCUM_JITTER or the thin-lens ray of vrt_set_lens, origin
 * and medium at the origin included -- marched as every frame marches it. The guide hit is therefore the hit the sample's
 * (voxel ID, dist) describes.
 *   hit      the march returned a hit. A miss adds nothing to any sum below.
 *   normal   +1 or -1 on one axis: hitNormal, or (0, 1, 0) where its length is not above 0 (comp:497), before the flip towards the
 *            ray of comp:524. Three signed integer sums.
 *   albedo   the four bytes of surfaceColor (comp:505-507): the hit leaf's R, G, B, A, or the previous voxel's where the hit leaf's
 *            alpha is 0; where the hit cell is the highlighted voxel (vrt_params) R, G, B become 255 - byte and A 255. Four
 *            unsigned integer sums. Alpha below 1 shows glass: by default the guide through glass is the glass surface and no
 *            refraction is followed; vrt_set_guide_glass (below) follows it.
 *   depth    the float32 distance from the sample's ray origin to the hit point in world units: with p = hitPoint, each component
 *            divided by u_voxelScale only when the scale is not 1, and o the ray's origin, d = sqrtf((dx*dx + dy*dy) + dz*dz) of
 *            p - o, every operation rounded on its own; then h(d) = min(max(0, d), 65504.0f) as in vrt_accum_keep_hdr point 1,
 *            added as a double, one add per sample in sample order, to one float64 sum.
 *   hits     one unsigned count.
 * The state is 40 bytes per pixel (uint32[4], int32[3], uint32, double), the accumulation's own, allocated by the first guide call:
 * an accumulation that never asks takes what it took. The planes of n samples, every division in float64 and one rounding to
 * float32:
 *   normal[3] = (float)(nsum / n)    albedo[4] = (float)(asum / (255.0 * n))    coverage = (float)(hits / n)
 *   depth = hits ? (float)(dsum / hits) : 0
 * Integer sums do not depend on how the samples were split over calls, and the depth sum is sequential per pixel: the planes are
 * the same bits after any sequence of vrt_accum_add and guide calls that leads to the same samples.
 *
 * vrt_accum_guides         HOST buffers [H][W][3], [H][W][4], [H][W], [H][W] (any may be NULL), synchronous. Needs an accumulation of
 *                          any mode and form (corner, jitter, lens, adaptive, plain or HDR) that holds samples: VRT_E_STATE before
 *                          vrt_accum_begin* and before the first vrt_accum_add. The first call adds the guides of samples
 *                          first_sample .. first_sample + total - 1, a later call those of the samples added since the last one,
 *                          then the planes are resolved over `total`. Whatever restarts the accumulation's sums -- a begin, or a
 *                          vrt_accum_add after a change of camera, uniforms, tree or lens -- clears the guide state with them. The
 *                          missing samples are marched with the context's current inputs: where those changed since the last
 *                          vrt_accum_add (which would restart) and samples are missing, the call returns VRT_E_STATE; add first.
 *                          Path depth, sun disc and the emitter settings are no inputs of a guide.
 * vrt_accum_guides_device  the same into DEVICE buffers; the resolve is enqueued on `stream` (NULL: the context's), ordered against
 *                          the adds as vrt_accum_resolve_device is.
 * Adaptive accumulations: `total` is the number of rounds, and every pixel's guide takes every round's sample index whatever its
 * active mask says -- a pixel that stopped early still has n = total guide samples, so its planes stay comparable with its
 * neighbours'. These calls read and write no byte of the accumulation's own sums: vrt_accum_resolve* return the same bytes with and
 * without them. They take no profiling slot.
 *
 * Ray batches, stateless, beside vrt_shade_rays: one march per ray, no sample index (a caller's ray has no jitter); the planes are
 * those of n = 1 -- normal [n][3] (zeros on a miss), albedo [n][4] = (float)(byte / 255.0), depth [n] = h(d) (0 on a miss) -- and
 * out_hit one byte per ray, 1 or 0. Rays, origin_stride and width as in vrt_shade_rays (width >= 1 only chooses how rays map to
 * lanes: a batch at least 8 wide and two rows high is traced in 8 x 8 tiles); origins in glass, in a solid or outside the world and
 * un-normalised or axis-parallel directions behave as there. Any output may be NULL, not all. Errors: those of vrt_shade_rays.
 * vrt_guide_rays: HOST buffers, synchronous; vrt_guide_rays_device: DEVICE buffers, enqueued on `stream` (NULL: the context's).
 * Unlike vrt_shade_rays they take no profiling slot (vrt_set_profiling) and do not count towards its stride.
 *
 * Guides past glass: vrt_set_guide_glass(ctx, 1) makes a guide sample follow the refracted ray through translucent surfaces to the
 * first opaque one, at most VRT_GUIDE_MAX_SURFACES surfaces in all. `on` is 0 (the default: everything above) or 1, VRT_E_INVALID
 * otherwise. It is context state: an accumulation reads it at vrt_accum_begin*, as vrt_accum_keep_hdr is read, and every call that
 * brings that accumulation's guide state up to date -- vrt_accum_guides*, vrt_accum_resolve_hdr_filtered*, ..._filtered_var*,
 * ..._temporal*, ..._temporal_mom* -- uses the rule as begun, so one guide state never mixes the two rules; a change takes effect at
 * the next begin and is no part of the restart rule. vrt_guide_rays and vrt_guide_rays_device read it at the call. Frames, views,
 * shards and vrt_multi ignore it. One sample's guide, every float operation float32 with no contraction:
 *   G0  Segment 0 is the sample's own ray exactly as above: the origin, the start medium read from the leaf at the origin, the
 *       normalised direction. S = 0, L = 0.0f.
 *   G1  March the segment with the frame's own march. A miss on any segment makes the sample a miss: it adds nothing to any sum,
 *       whatever glass it passed -- sky seen through glass has coverage 0, as sky seen directly has.
 *   G2  On a hit take the normal (comp:497, before the flip), the four surfaceColor bytes b (comp:505-507) and the highlighted
 *       voxel's inversion, all exactly as above. d_j = sqrtf((dx*dx + dy*dy) + dz*dz) of p - o in world units: p the hit point, each
 *       component divided by u_voxelScale only when the scale is not 1; o the segment's origin, the ray's own for segment 0 and for
 *       later segments the grid-space origin of G5 divided in the same way. L = L + d_j. If S == 0, A0 = the alpha byte of b.
 *       S = S + 1.
 *   G3  If the alpha byte of b is 255 the chain ends here, on an opaque surface.
 *   G4  Otherwise, if S == VRT_GUIDE_MAX_SURFACES, the chain ends here, on glass.
 *   G5  Otherwise comp:547-572 as VRT_MODE_FULL has it: the alpha-0 rules for the hit and the previous voxel's properties (the
 *       latter with this segment's medium), n1 and n2, the normal flipped and n1, n2 swapped when dot(inc, normal) > 0, refr_dir =
 *       refract(inc, normal, n1 / n2), R0 = (n1 - n2) / (n1 + n2) * (n1 - n2) / (n1 + n2), fres = clamp(R0 + (1 - R0) *
 *       pow(1 - max(0, dot(-inc, normal)), 5), 0, 1) with the shader's deterministic pow, has_tir = length(refr_dir) < 0.001f,
 *       reflect_i = fres, refract_i = has_tir ? 0 : 1 - fres. Where reflect_i <= 0.001f or refract_i <= 0.001f the shader shades
 *       this surface and spawns nothing: the chain ends here, on glass. (The shader's full-stack test is no part of the rule: a guide
 *       has no stack.) Otherwise the next segment starts at hitPoint - normal * 1e-4f (grid units) along refr_dir, as given, in
 *       medium n2, whose byte is rint(n2 * 85); go to G1.
 *   G6  The sample is a hit: the normal, R, G and B are the final surface's, A = A0, the first surface's alpha byte, and the depth
 *       is h(L), the length of the bent path. A is 255 where the pixel sees its surface directly and the glass's alpha where it sees
 *       it through glass, so an albedo distance still separates "through the pane" from "beside the pane", whose radiance differs
 *       by the pane's tint, while R, G, B, the normal and the depth separate the objects behind it.
 * The sums, the 40-byte state, the resolve and the hit count are those above. With the setting off, or where no segment-0 hit is
 * translucent, G0-G6 give the guide above bit for bit. For vrt_temporal_hdr* the depth plane then places a pixel's point at
 * origin + dir * L, the unfolded path: exact where nothing refracts, approximate behind a pane.
 * Not provided: following reflections, a per-surface tint plane, exact reprojection through refraction, motion vectors, frames,
 * views, shards, vrt_multi. */
#define VRT_GUIDE_MAX_SURFACES 8
int vrt_set_guide_glass(vrt_ctx *ctx, int on);
int vrt_accum_guides(vrt_ctx *ctx, float *out_normal, float *out_albedo, float *out_depth, float *out_coverage);
int vrt_accum_guides_device(vrt_ctx *ctx, void *d_normal, void *d_albedo, void *d_depth, void *d_coverage, void *stream);
int vrt_guide_rays(vrt_ctx *ctx, size_t n, const float *origins, int origin_stride, const float *dirs, int width, float *out_normal,
                   float *out_albedo, float *out_depth, uint8_t *out_hit);
int vrt_guide_rays_device(vrt_ctx *ctx, size_t n, const void *d_origins, int origin_stride, const void *d_dirs, int width, void *d_normal,
                          void *d_albedo, void *d_depth, void *d_hit, void *stream);

/* EXTENSION: the guided filter -- an edge-avoiding a-trous wavelet filter on FLOAT radiance whose edge weights come from the guide
 * planes above. vrt_denoise_hdr averages inside one voxel ID, so where a voxel is a pixel wide it filters nothing; this filter
 * averages across voxels that lie on one surface (same normal, same albedo, depth on the centre's own slope) and stops at the edges
 * the planes show. Input: any [H][W][3] float image -- an HDR accumulation's mean, a ray batch's -- and the four planes in the shapes
 * vrt_accum_guides_device writes: normal [H][W][3], albedo [H][W][4], depth [H][W], coverage [H][W].
 *
 * All arithmetic below is float32: every operation rounded on its own, no contraction. h(c) = min(max(0, c), 65504.0f) with the
 * min / max conventions of vrt_accum_keep_hdr point 1 (NaN -> +0). p is a pixel, q a tap, s a level's step.
 *  1. Inputs. Every colour float goes through h. Every guide float goes through g(v): NaN -> 0, anything else clamped to
 *     [-65504, 65504]. A pixel is LIVE when g(coverage) > 0. A pixel that is not live yields h(c) per channel, at every `levels`, and
 *     is never a tap: sky is never mixed into surfaces, nor surfaces into sky.
 *  2. Modulation. With VRT_FILTER_DEMODULATE m_ch = max(albedo_ch + (1.0f - coverage), 1.0f / 255.0f) for ch in R, G, B (the albedo
 *     plane is coverage-weighted, so the part of the pixel that saw sky counts as albedo 1); otherwise m_ch = 1. Level 0 reads
 *     u = h(c) / m.
 *  3. Depth slopes of the centre. gx = the smaller of |Z(x-1, y) - Z(x, y)| and |Z(x+1, y) - Z(x, y)| over those of the two
 *     neighbours that are inside the image and live, 0 if there is none; gy likewise over (x, y-1) and (x, y+1). The one-sided
 *     minimum keeps the slope of the surface the pixel lies on at a depth edge.
 *  4. Level i = 0 .. levels-1, s = 1 << i. For a live p: sumw = 0, sum_ch = 0; then over oy = -2..2 (outer), ox = -2..2 (inner),
 *     q = p + s * (ox, oy), skipped when outside the image or not live:
 *       dn2 = (dx*dx + dy*dy) + dz*dz                   of the three normal differences q - p
 *       da2 = (a0*a0 + a1*a1) + (a2*a2 + a3*a3)         of the four albedo differences (alpha separates glass from the opaque)
 *       dzq = |Z_q - Z_p|
 *       den = sigma_depth * ((gx * (float)(|ox|*s) + gy * (float)(|oy|*s)) + Z_p * (1.0f / 256.0f)) + 0x1p-20f
 *       e   = (dn2 * kn + da2 * ka) + dzq / den
 *       w   = (B[|oy|] * B[|ox|]) * det_expf(-e)        B = {3/8, 1/4, 1/16}; det_expf: the kernels' exp (Cephes-style, plain mul/add)
 *       sumw = sumw + w;  sum_ch = sum_ch + w * u_q[ch]
 *     and u'_p[ch] = sum_ch / sumw. kn = 1.0f / (sigma_normal * sigma_normal), ka = 1.0f / (sigma_albedo * sigma_albedo), computed
 *     once on the host. The centre tap has e = +0 and w = 9/64 exactly, so sumw > 0. Levels ping-pong between two images: a level
 *     never reads what it writes, and the sum order is the loop order above, whatever the launch shape.
 *  5. Output. f = h(u * m); with levels == 0 that is h(h(c) / m * m), h(c) bit for bit without demodulation. out_rgb [H][W][3]
 *     receives f, out_rgba8 [H][W][4] unorm8(tonemap(f)), alpha 255, with vrt_accum_resolve_hdr's two operators (tm == NULL:
 *     VRT_TONEMAP_CLAMP, exposure 1). Either output may be NULL, not both.
 * There is no colour or luminance term here: without a per-pixel variance its width would be a guess (vrt_filter_hdr_var below has
 * both). Depth is meant to be >= 0 (the guide
 * planes' is); a negative depth is taken as it is and may make den <= 0, whose outcome the rules above still define (h ends it).
 *
 * vrt_filter_default    levels 1, VRT_FILTER_DEMODULATE, sigma_normal 1.0, sigma_albedo 0.05, sigma_depth 2.0: the best row
 *                       of the quality sweep in profiles/filter_quality.txt (DESIGN.md section 3 "Guided filter").
 * vrt_filter_hdr        DEVICE pointers, stream-ordered, stateless. f == NULL: vrt_filter_default. VRT_E_INVALID: a NULL input, both
 *                       outputs NULL, d_out_rgb equal to any input, levels outside 0..VRT_FILTER_MAX_LEVELS, unknown flag bits, a
 *                       sigma that is not finite or not > 0 (or so small that 1 / sigma^2 is not finite), a tone map
 *                       vrt_accum_resolve_hdr refuses, a frame size vrt_denoise refuses. Scratch is the context's: 48 bytes per pixel
 *                       of packed guides (levels >= 1) and 16 per pixel for each of the two level images (levels >= 2, >= 3),
 *                       allocated by the first call that needs them, grown and never shrunk; a call that grows them waits for the
 *                       device. Calls on different streams are ordered against each other, since they share the scratch.
 * vrt_filter_hdr_host   the same through HOST buffers, synchronous, staged through 64 more bytes per pixel the context keeps.
 * vrt_accum_resolve_hdr_filtered  the filter on an HDR accumulation: the input is its float mean -- exactly vrt_accum_resolve_hdr's
 *                       out_rgb -- with the accumulation's own guide planes, which the call first brings up to date exactly as a
 *                       vrt_accum_guides call would. HOST buffers (either may be NULL, not both), synchronous. Errors: VRT_E_STATE
 *                       where vrt_accum_guides or vrt_accum_resolve_hdr return it (no begin, no sample, begun without HDR, inputs
 *                       changed since the last add while guide samples are missing); VRT_E_INVALID as above. Mean, planes and outputs
 *                       pass through 64 bytes per pixel that belong to the accumulation, allocated by the first such call.
 * vrt_accum_resolve_hdr_filtered_device  the same into DEVICE buffers, enqueued on `stream` (NULL: the context's), ordered against the
 *                       adds as vrt_accum_resolve_hdr_device is.
 * The accumulation forms read and write no byte of the accumulation's sums: vrt_accum_resolve*, vrt_accum_resolve_hdr* and
 * vrt_accum_guides* return the same bits with and without them. None of these calls takes a profiling slot or counts towards the
 * stride. Per-sample second moments of the HDR sums: vrt_accum_keep_moments below, whose plane vrt_filter_hdr_var's variance input
 * takes. Not provided: motion vectors of moving geometry, frames, views, shards and vrt_multi, and a filtered form of vrt_shade_rays_hdr
 * (an image-shaped batch can call vrt_filter_hdr with vrt_guide_rays_device's planes and a coverage plane made of its hit bytes). */
#define VRT_FILTER_MAX_LEVELS 8
#define VRT_FILTER_DEMODULATE 1u
typedef struct vrt_filter { int32_t levels; uint32_t flags; float sigma_normal, sigma_albedo, sigma_depth; } vrt_filter;
void vrt_filter_default(vrt_filter *f);
int vrt_filter_hdr(vrt_ctx *ctx, int width, int height, const void *d_rgb, const void *d_normal, const void *d_albedo,
                   const void *d_depth, const void *d_coverage, const vrt_filter *f, const vrt_tonemap *tm, void *d_out_rgb,
                   void *d_out_rgba8, void *stream);
int vrt_filter_hdr_host(vrt_ctx *ctx, int width, int height, const float *rgb, const float *normal, const float *albedo,
                        const float *depth, const float *coverage, const vrt_filter *f, const vrt_tonemap *tm, float *out_rgb,
                        uint8_t *out_rgba8);
int vrt_accum_resolve_hdr_filtered(vrt_ctx *ctx, const vrt_filter *f, const vrt_tonemap *tm, float *out_rgb, uint8_t *out_rgba8);
int vrt_accum_resolve_hdr_filtered_device(vrt_ctx *ctx, const vrt_filter *f, const vrt_tonemap *tm, void *d_rgb, void *d_rgba8,
                                          void *stream);
/* EXTENSION: the variance-guided filter -- the guided filter above with an edge-stopping LUMINANCE term whose width is the pixel's own
 * variance, and that variance carried through the levels (SVGF's rule). Shadow edges, penumbrae and the falloff around emitters lie on
 * one surface -- one normal, one albedo, a smooth depth -- so no guide sees them and every level of vrt_filter_hdr past the first
 * blurs them; here a tap whose luminance differs from the centre's by many standard deviations counts for little. The variance is
 * the caller's plane d_variance [H][W] -- the variance of Y (V1) of the INPUT image at that pixel: of the mean, not of one sample --
 * or, with d_variance == NULL, a spatial estimate from the image itself (SVGF's rule for pixels with a short history).
 *
 * All arithmetic is float32, every operation rounded on its own, nothing contracted. Points 1-3 of vrt_filter_hdr (inputs,
 * modulation, depth slopes) hold unchanged; u is level 0's h(c) / m.
 *  V1. Luminance. Y(u) = (0.2126f * u.x + 0.7152f * u.y) + 0.0722f * u.z.
 *  V2. Initial variance v0_p of a live pixel. hv(x): NaN, -0 and everything negative -> +0, otherwise at most 65504.0f * 65504.0f.
 *      Ym = Y(m) with point 2's m; without VRT_FILTER_DEMODULATE Ym is 1.0f and is not computed.
 *      With a caller's plane: v0 = hv(var_p) / (Ym * Ym).
 *      With d_variance == NULL: sw = s1 = s2 = 0, then over oy = -3..3 (outer), ox = -3..3 (inner), q = p + (ox, oy), skipped when
 *      outside the image or not live:
 *        e  = point 4's e with s = 1, that is den = sigma_depth * ((gx * (float)|ox| + gy * (float)|oy|) + Z_p * (1.0f / 256.0f)) + 0x1p-20f
 *        w  = det_expf(-e)                               no B factor
 *        l  = Y(u_q)
 *        sw = sw + w;  s1 = s1 + w * l;  s2 = s2 + w * (l * l)
 *      and m1 = s1 / sw, m2 = s2 / sw, v0 = max(0, m2 - m1 * m1) (NaN -> +0). The centre has w = 1, so sw > 0.
 *  V3. Level i = 0 .. levels-1, s = 1 << i, live p. First the centre's smoothed variance: gs = gv = 0, then over oy = -1..1 (outer),
 *      ox = -1..1 (inner), q = p + s * (ox, oy), skipped when outside the image or not live: G = 1/4 for the centre, 1/8 for the four
 *      edges, 1/16 for the four corners; gs = gs + G; gv = gv + G * v_q. vbar = gv / gs and
 *        sl = sigma_lum * sqrtf(vbar) + 0x1p-20f         the IEEE correctly rounded square root
 *      The 3 x 3 runs on the level's own lattice, spacing s (SVGF's has spacing 1): that is what a level has at hand.
 *      Then point 4's 25 taps in point 4's order, with
 *        dl   = |Y(u_q) - Y(u_p)|
 *        e    = ((dn2 * kn + da2 * ka) + dzq / den) + dl / sl
 *        w    = (B[|oy|] * B[|ox|]) * det_expf(-e)
 *        sumw = sumw + w;  sum_ch = sum_ch + w * u_q[ch];  sumv = sumv + (w * w) * v_q
 *      and u'_p[ch] = sum_ch / sumw, v'_p = sumv / (sumw * sumw). The centre tap has e = +0 and w = 9/64.
 *  V4. Output. The colours as in point 5. out_variance [H][W] receives hv(v * (Ym * Ym)) for a live pixel, v the variance after the last
 *      level (v0 with levels == 0), and +0 for a pixel that is not live: it is the variance of Y of the OUTPUT image, a plane a
 *      further call can take. (hv ends what a negative depth may make of v, as h ends the colours.)
 * Two identities follow. On an image whose live pixels all carry one colour, without demodulation, dl = 0 at every tap of level 0,
 * and of a later level where the levels before returned that colour exactly -- they do where every channel is 0 or a power of two
 * (each w * c is exact, sum_ch is c times sumw, the quotient c). The colour outputs are then vrt_filter_hdr's bit for bit: up to one
 * level for any colour, at every level count for such a colour. With levels == 0 the colour outputs are vrt_filter_hdr's at levels == 0.
 *
 * vrt_filter_var_default  levels 3, VRT_FILTER_DEMODULATE, sigma_normal 0.5, sigma_albedo 0.05, sigma_depth 2.0, sigma_lum 4.0: the best
 *                       row of the quality sweep with the spatial estimate (profiles/filter_var_quality.txt, DESIGN.md section 3
 *                       "Variance-guided filter").
 * vrt_filter_hdr_var    DEVICE pointers, stream-ordered, stateless. f == NULL: vrt_filter_var_default. levels, flags, the guide sigmas,
 *                       the tone map, the frame size, the stream ordering, and the scratch with its ownership and growth are
 *                       vrt_filter_hdr's (levels == 0 with d_out_variance takes the packed guides too); sigma_lum must be finite
 *                       and > 0. d_variance may be NULL (the spatial estimate). d_out_variance is an output only and may be NULL;
 *                       one of the two colour outputs must not be. VRT_E_INVALID also where d_out_rgb or d_out_variance equals
 *                       any input, d_variance included.
 * vrt_filter_hdr_var_host  the same through HOST buffers, synchronous, staged through 72 bytes per pixel the context keeps.
 * vrt_accum_resolve_hdr_filtered_var, _device  vrt_accum_resolve_hdr_filtered{,_device} with this filter: the same input, the same
 *                       VRT_E_STATE rule, the guide state brought up to date as a vrt_accum_guides call would, 72 bytes per pixel
 *                       that belong to the accumulation. The variance: on an accumulation that keeps moments
 *                       (vrt_accum_keep_moments below) and holds two samples or more, vrt_accum_variance_device's plane (M3) as
 *                       d_variance, through four more bytes per pixel that belong to the accumulation, made at the first such call
 *                       (an adaptive accumulation has min_samples >= 2, so every pixel then holds two samples); on every other
 *                       accumulation, and with one sample, the spatial estimate (d_variance == NULL).
 * These calls read and write no byte of the accumulation's sums, take no profiling slot and do not count towards the stride. */
typedef struct vrt_filter_var { int32_t levels; uint32_t flags; float sigma_normal, sigma_albedo, sigma_depth, sigma_lum; } vrt_filter_var;
void vrt_filter_var_default(vrt_filter_var *f);
int vrt_filter_hdr_var(vrt_ctx *ctx, int width, int height, const void *d_rgb, const void *d_normal, const void *d_albedo,
                       const void *d_depth, const void *d_coverage, const void *d_variance, const vrt_filter_var *f, const vrt_tonemap *tm,
                       void *d_out_rgb, void *d_out_rgba8, void *d_out_variance, void *stream);
int vrt_filter_hdr_var_host(vrt_ctx *ctx, int width, int height, const float *rgb, const float *normal, const float *albedo,
                            const float *depth, const float *coverage, const float *variance, const vrt_filter_var *f,
                            const vrt_tonemap *tm, float *out_rgb, uint8_t *out_rgba8, float *out_variance);
int vrt_accum_resolve_hdr_filtered_var(vrt_ctx *ctx, const vrt_filter_var *f, const vrt_tonemap *tm, float *out_rgb, uint8_t *out_rgba8,
                                       float *out_variance);
int vrt_accum_resolve_hdr_filtered_var_device(vrt_ctx *ctx, const vrt_filter_var *f, const vrt_tonemap *tm, void *d_rgb, void *d_rgba8,
                                              void *d_variance_out, void *stream);
/* EXTENSION: luminance moments of an HDR accumulation -- a MEASURED variance for the filter above. A sample's luminance exists only
 * inside the sample kernels, so the sums are kept there.
 *
 * vrt_accum_keep_moments(ctx, 1) makes the HDR accumulations begun after it keep two more float64 sums per pixel. It is context state,
 * read by the next vrt_accum_begin / _begin_ex / _begin_adaptive exactly as vrt_accum_keep_hdr is; it is not part of the restart
 * rule, and changing it leaves a running accumulation as it was begun. It takes effect only in an accumulation begun with HDR on and
 * is ignored otherwise. Default 0. VRT_E_INVALID unless enable is 0 or 1.
 *
 * All float32 operations below are rounded on their own; nothing is contracted.
 *  M1. A sample's luminance and its square. y = Y(h(c)) with V1's Y (float32, V1's association) on the sample's three h(c) values of
 *      vrt_accum_keep_hdr point 1; q = y * y, a FLOAT32 product (q <= 65504^2: no overflow).
 *  M2. The sums. Two float64 sums per pixel start at +0.0: S1 = S1 + (double)y and S2 = S2 + (double)q, one add each per sample the
 *      pixel takes, in sample-index order, exactly where and when the three colour sums take theirs. They continue across
 *      vrt_accum_add calls (3 + 5 samples equal 8 bit for bit); whatever zeroes the colour sums zeroes them. A pixel whose every
 *      sample is one float colour adds (double)y * k and (double)q * k for k samples at once: both exact for k <= 2^24, y and q being
 *      floats, so the result is the k sequential adds'.
 *  M3. The resolve, n the pixel's own count (the accumulation's when not adaptive). n < 2: the variance is 65504.0f * 65504.0f,
 *      "unknown", the value the temporal pass gives a pixel without history. Otherwise
 *        m1 = S1 / (double)n;  m2 = S2 / (double)n;  m1f = (float)m1;  sq = m1f * m1f (float32);  d = m2 - (double)sq
 *        var = hv((float)(max(0, d) / (double)(n - 1)))      max with the zero first: NaN -> +0; hv of V2
 *      the variance of the MEAN's luminance, what vrt_filter_hdr_var's d_variance asks for. The square of the mean is a float32
 *      product on purpose, as q is: a pixel whose samples are all equal has m1 = y, sq = q, m2 = q and a variance of exactly +0 at
 *      any count -- sky, the primary modes from the corner and pixels without a bounce are not handed rounding noise as a width. The
 *      price: on a nearly constant pixel the rounding of m1 to float32 leaves a floor of about 2^-22 * m1^2 / (n - 1) (|d| below that
 *      is not resolved, and may come out as +0 or as the floor).
 *
 * vrt_accum_variance    the M3 plane [H][W] into a HOST buffer, synchronous.
 * vrt_accum_variance_device  the same into a DEVICE buffer, enqueued on `stream` (NULL: the context's), ordered against the adds as
 *                       vrt_accum_resolve_hdr_device is.
 * Both: VRT_E_STATE with no begin, no sample yet, an accumulation begun without HDR or begun without moments; VRT_E_INVALID for a NULL
 * output. Neither takes a profiling slot or counts towards the stride.
 * With moments off nothing changes: the same kernels, the same bytes, the same footprint. With moments on the accumulation takes 16
 * bytes per pixel more, allocated at the begin; every resolve, vrt_accum_counts and the guide calls return the bits they return
 * without -- the colour sums are the same bits -- and only vrt_accum_resolve_hdr_filtered_var{,_device} change, as said there.
 * Not provided: moments of ray batches (vrt_shade_rays_hdr_device's d_sums are the caller's), per-channel variance, a per-pixel mix of the spatial and the measured variance, frames, views,
 * shards and vrt_multi. */
int vrt_accum_keep_moments(vrt_ctx *ctx, int enable);
int vrt_accum_variance(vrt_ctx *ctx, float *out_variance);
int vrt_accum_variance_device(vrt_ctx *ctx, void *d_variance, void *stream);
/* EXTENSION: temporal accumulation -- last frame's integrated colour and luminance moments reprojected into this frame through the
 * guide planes, each tap tested against them, blended with this frame's image, and a TEMPORAL variance handed to the filter above
 * (SVGF's rules). An accumulation restarts on every change of the camera block, so a moving camera never holds more than one frame's
 * samples per pixel; this pass carries them across the move, and gives vrt_filter_hdr_var the variance input the accumulation forms
 * above estimate spatially. Input: a float image [H][W][3] and the normal [H][W][3], depth [H][W] and coverage [H][W] planes that
 * vrt_accum_guides_device writes, with the camera block they were made with, in vrt_set_camera's shapes; no albedo.
 *
 * The history is the caller's memory, as d_sums is for vrt_shade_rays_hdr_device: 48 bytes per pixel as three row-major planes of
 * 16-byte words, plane k at byte k * W * H * 16, 16-byte aligned:
 *   plane 0  {r, g, b, N}           the integrated colour and the history length, a float
 *   plane 1  {m1, m2, Z, coverage}  the first and second moment of luminance, the depth and coverage of the frame that wrote it
 *   plane 2  {nx, ny, nz, +0}       the normal of the frame that wrote it
 * history_in == NULL marks the first frame: no pixel has a history and the previous camera is not read. history_out must differ from
 * history_in and from every input, since a pass reads its neighbours; a caller ping-pongs two histories.
 *
 * All arithmetic is float32, every operation rounded on its own, nothing contracted; h, g and hv as in vrt_filter_hdr_var, min and
 * max with vrt_accum_keep_hdr's conventions. The inputs go through h (colour) and g (normal, depth, coverage); every value read from
 * the history goes through h (colour, m1), hv (m2) or g (the rest), and N then into [0, (float)max_history]. A pixel is LIVE when
 * g(coverage) > 0. A pixel that is not live writes {h(c), 0}, {0, 0, 0, 0}, {0, 0, 0, 0} to the history, h(c) to out_rgb and +0 to
 * out_variance, and is never a tap. For a live pixel p = (px, py) with depth Z_p and normal n_p:
 *  T1. World point. d = shader_ray_dir() (the ray generation of comp:624-641, one operation at a time) at
 *      ((float)px + offset_x, (float)py + offset_y), scaled by 1.0f / sqrtf(dot(d, d)) as primary_ray_dir()'s general form does;
 *      P_i = e_i + Z_p * d_i with e = camera_pos. The planes' depth is the distance from the RAY'S origin: with a thin lens
 *      (vrt_set_lens) that origin is not e and P is approximate.
 *  T2. Previous position. clip = mat_vec(prev_view_proj, P, 1) in mat_vec's order, (m0*x + m1*y) + (m2*z + m3*w). No history unless
 *      clip.w > 1e-6f. fx = (((clip.x / clip.w) + 1.0f) * 0.5f) * (float)W - offset_x, the inverse of the shader's u; fy likewise with
 *      clip.y, H and offset_y. No history unless fx > -1 && fx < W && fy > -1 && fy < H (NaN: false). x0 = floorf(fx), tx = fx - x0,
 *      the same in y. Zexp = sqrtf((dx*dx + dy*dy) + dz*dz) of P - prev_camera_pos: the depth the previous frame saw P at.
 *  T3. Taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), in that order, with the weights (1.0f - tx) * (1.0f - ty),
 *      tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty. A tap q COUNTS when it is inside the image, its stored coverage is > 0 and its
 *      N >= 1, (nq.x*np.x + nq.y*np.y) + nq.z*np.z >= normal_min, and |Zq - Zexp| <= depth_tol * Zexp + 0x1p-20f. sw = the sum of
 *      the counted taps' weights, from 0 in tap order; there is a history iff sw > 0, and every previous quantity X -- the colour,
 *      N, m1, m2 -- is (the sum of w * Xq, from 0 in tap order) / sw. Without a history every previous quantity is +0.
 *  T4. N' = min(Nprev + 1.0f, (float)max_history), a = max(1.0f / N', alpha_min), am = max(1.0f / N', alpha_moments_min).
 *  T5. c' = cp + a * (h(c) - cp) per channel; Y = V1's luminance of h(c); m1' = m1p + am * (Y - m1p); m2' = m2p + am * (Y * Y - m2p).
 *      A pixel without a history therefore returns h(c), Y and Y * Y exactly, with N' = 1.
 *  T6. The history receives {c', N'}, {m1', m2', Z_p, coverage_p}, {n_p, +0}; out_rgb [H][W][3] receives c'; out_variance [H][W]
 *      receives hv(max(0, m2' - m1' * m1') / (N' - 1.0f)) where N' >= 2 -- the variance of the MEAN, exact while a = 1 / N' and an
 *      approximation once alpha_min or max_history binds -- and 65504.0f * 65504.0f where N' < 2: the luminance term of
 *      vrt_filter_hdr_var vanishes there and the guides alone filter a pixel that has no history.
 *
 * vrt_temporal_default  max_history 8, alpha_min 0.4, alpha_moments_min 0.6, normal_min 0.0, depth_tol 0.4, offsets 0: the best row of
 *                       the quality sweep in profiles/temporal_quality.txt (DESIGN.md section 3 "Temporal accumulation"); the two
 *                       previous-camera fields zeroed, the caller fills them.
 *                       prev_view_proj is the previous frame's FORWARD projection * view, column-major: what main.cpp:808-809
 *                       multiplies, the inverse of that frame's inv_view * inv_projection.
 * vrt_temporal_hdr      DEVICE pointers, stream-ordered (NULL: the context's), stateless: it reads no context state, keeps no scratch
 *                       and takes no profiling slot. d_out_rgb and d_out_variance may be NULL. VRT_E_INVALID: a NULL input, t or
 *                       d_history_out; d_history_out equal to d_history_in or to an input, or an output equal to an input or to
 *                       another output; a history that is not 16-byte aligned; max_history outside 1..32768, an alpha outside
 *                       [0, 1], normal_min outside [-1, 1], depth_tol not finite or not > 0, an offset outside [0, 1]; a matrix or
 *                       camera position entry that is not finite (the previous camera's only where d_history_in is given); a
 *                       frame size vrt_denoise refuses.
 * vrt_temporal_hdr_host the same through HOST buffers, synchronous, staged through 144 bytes per pixel the context keeps.
 * vrt_accum_resolve_hdr_temporal  the pass on an HDR accumulation, chained with vrt_filter_hdr_var: the input is its float mean
 *                       (vrt_accum_resolve_hdr's out_rgb) with its own planes, brought up to date as a vrt_accum_guides call would,
 *                       and the context's CURRENT camera block; offset_x / offset_y of t are replaced by 0.5 for VRT_ACCUM_JITTER
 *                       and 0 otherwise. T1-T6, then vrt_filter_hdr_var on the integrated colour with T6's variance as its
 *                       plane (f == NULL: vrt_filter_var_default). out_integrated [H][W][3] (may be NULL) is the UNFILTERED
 *                       integrated colour, which is also what the history stores; out_rgb, out_rgba8, out_variance are the
 *                       filter's (one of the first two must not be NULL). HOST buffers, the histories too (history_in may be
 *                       NULL), synchronous. Errors: VRT_E_STATE as vrt_accum_resolve_hdr_filtered_var, VRT_E_INVALID as the two
 *                       stateless calls. The accumulation's filter stage serves it, grown to 84 bytes per pixel (12 for the
 *                       integrated image), and by 96 more for the two histories of this host form.
 * vrt_accum_resolve_hdr_temporal_device  the same with DEVICE histories and outputs, enqueued on `stream` (NULL: the context's),
 *                       ordered against the adds as vrt_accum_resolve_hdr_device is.
 * These calls read and write no byte of the accumulation's sums: every resolve and guide call returns the same bits with and without
 * them. None takes a profiling slot or counts towards the stride. The measured variance of an accumulation that keeps moments as
 * an input, and a 3 x 3 search where all four bilinear taps fail, are vrt_temporal_hdr_mom's, below. Not provided: the filter's
 * first level fed back into the history, an albedo or voxel-ID test, moving geometry (a voxel edit between frames is
 * seen only through the depth and normal tests), lens-exact reprojection, frames, views, shards and vrt_multi. */
typedef struct vrt_temporal {
    float prev_view_proj[16];   /* previous frame's FORWARD projection * view, column-major */
    float prev_camera_pos[4];   /* previous frame's camera_pos */
    float offset_x, offset_y;   /* where in the pixel the planes' ray passes: 0 corner, 0.5 jittered; finite, in [0, 1] */
    int32_t max_history;        /* 1 .. 32768 */
    float alpha_min, alpha_moments_min;   /* in [0, 1] */
    float normal_min;           /* finite, in [-1, 1] */
    float depth_tol;            /* finite, > 0 */
} vrt_temporal;
void vrt_temporal_default(vrt_temporal *t);
int vrt_temporal_hdr(vrt_ctx *ctx, int width, int height, const float inv_projection[16], const float inv_view[16],
                     const float camera_pos[4], const void *d_rgb, const void *d_normal, const void *d_depth, const void *d_coverage,
                     const void *d_history_in, const vrt_temporal *t, void *d_history_out, void *d_out_rgb, void *d_out_variance,
                     void *stream);
int vrt_temporal_hdr_host(vrt_ctx *ctx, int width, int height, const float inv_projection[16], const float inv_view[16],
                          const float camera_pos[4], const float *rgb, const float *normal, const float *depth, const float *coverage,
                          const void *history_in, const vrt_temporal *t, void *history_out, float *out_rgb, float *out_variance);
int vrt_accum_resolve_hdr_temporal(vrt_ctx *ctx, const vrt_temporal *t, const vrt_filter_var *f, const vrt_tonemap *tm,
                                   const void *history_in, void *history_out, float *out_integrated, float *out_rgb, uint8_t *out_rgba8,
                                   float *out_variance);
int vrt_accum_resolve_hdr_temporal_device(vrt_ctx *ctx, const vrt_temporal *t, const vrt_filter_var *f, const vrt_tonemap *tm,
                                          const void *d_history_in, void *d_history_out, void *d_integrated, void *d_rgb, void *d_rgba8,
                                          void *d_variance_out, void *stream);
/* EXTENSION: the temporal pass with MEASURED frame variances and a 3 x 3 search -- vrt_temporal_hdr above hands a pixel without a
 * history 65504^2, which the variance-guided filter then carries to its neighbours level by level; and a pixel loses its history
 * whenever all four bilinear taps fail. These calls take this frame's measured variance of the mean (vrt_accum_variance_device's
 * plane, M3) as one more input, integrate it as the colour is integrated, and hand it out while the history is short; and they can
 * look for a history in the 3 x 3 neighbourhood of the reprojected position where the bilinear taps found none (SVGF's fallback).
 * New entry points beside the old ones: every existing call keeps its bits.
 *
 * All arithmetic is float32, every operation rounded on its own, nothing contracted; h, g, hv as in vrt_temporal_hdr. The history
 * has vrt_temporal_hdr's layout except plane 2, which is {nx, ny, nz, V}: V the variance of the integrated mean's luminance by T7.
 * Inputs, liveness, the pixel that is not live (it stores +0 in V's place too) and T1, T2, T4, T5 are vrt_temporal_hdr's, unchanged.
 * T3 is unchanged, and V is one more previous quantity: Vq = hv(plane 2's fourth float of tap q), weighted as every other.
 *  T3s. The search. Only where search == 1, a history is given, T2 produced a position (clip.w > 1e-6f and fx, fy inside T2's
 *      window), and T3 ended with sw == 0. xc = (int)floorf(fx + 0.5f), yc = (int)floorf(fy + 0.5f). The nine taps (xc + dx, yc + dy),
 *      dy outer from -1 to 1, dx inner from -1 to 1. A tap COUNTS by T3's own tests, unchanged: inside the image, stored coverage > 0,
 *      N >= 1, the normal test, the depth test against the same Zexp and tolerance. Every counted tap has weight 1.0f; sw is their
 *      sum, from 0 in that order; there is a history iff sw > 0, and every previous quantity X -- the colour, N, m1, m2, V -- is
 *      (the sum of Xq, from 0 in that order) / sw. With search == 0 the step does not exist.
 *  T7. The variance of the integrated mean, from measured frame variances. v = hv(variance_in[p]), or 65504.0f * 65504.0f where
 *      d_variance_in is NULL. Vp is the previous quantity V (+0 without a history). om = 1.0f - a with T4's a;
 *      V' = hv((om * om) * Vp + (a * a) * v). The integrated colour is a weighted sum of independent frame means, so this is its
 *      variance with whatever weights T4 chose, exponential ones included; T6's estimate is exact only while a = 1 / N'. Without a
 *      history a = 1 and V' = v exactly.
 *  T6m. Outputs. The history is T6's with plane 2 = {n_p, V'}. out_rgb is T6's. out_variance = N' < (float)measured_below ? V' :
 *      T6's value (which is 65504.0f * 65504.0f at N' < 2).
 * A history written by vrt_temporal_hdr carries +0 in V's place: handed to these calls it reads as "exactly known" and is
 * under-trusted only until the (1 - a)^2 decay has worn that off; vrt_temporal_hdr ignores the slot, so a history of these calls can
 * go back to it. measured_below = 1, search = 0 is vrt_temporal_hdr on every output, and on the history except that one float. A
 * frame of one sample has v = "unknown" (M3 at n < 2) and behaves as today at a disocclusion.
 *
 * vrt_temporal_mom_default  vrt_temporal_default's fields, then measured_below and search: the best row of the quality sweep in
 *                       profiles/temporal_mom_quality.txt at vrt_temporal_default's tap tests (DESIGN.md section 3 "Temporal
 *                       pass with measured variances").
 * vrt_temporal_hdr_mom  DEVICE pointers, stream-ordered, stateless, no profiling slot: every rule of vrt_temporal_hdr. d_variance_in
 *                       [H][W] may be NULL; it counts among the inputs for the aliasing rules. VRT_E_INVALID also for
 *                       measured_below outside 1..32769 (32769: always the measured variance, max_history being at most 32768)
 *                       and search other than 0 or 1.
 * vrt_temporal_hdr_mom_host  the same through HOST buffers, synchronous, staged through 148 bytes per pixel the context keeps.
 * vrt_accum_resolve_hdr_temporal_mom, _device  the chain of vrt_accum_resolve_hdr_temporal{,_device} with this pass: the same
 *                       input, camera, offsets, filter, outputs, staging and VRT_E_STATE rule. d_variance_in is the accumulation's
 *                       own M3 plane where it was begun with moments (vrt_accum_keep_moments) -- exactly what
 *                       vrt_accum_variance_device returns, through the accumulation's own four bytes per pixel -- and NULL where
 *                       it was not.
 * These calls read and write no byte of the accumulation's sums: every resolve, vrt_accum_counts, vrt_accum_variance and the guide
 * calls return the same bits with and without them. None takes a profiling slot or counts towards the stride. Not provided (out of
 * scope here): the filter's first level fed back into the history, an albedo or voxel-ID test, moving geometry, lens-exact
 * reprojection, per-channel variance, frames, views, shards and vrt_multi; vrt_temporal_default is what it was. */
typedef struct vrt_temporal_mom {
    float prev_view_proj[16];   /* vrt_temporal's fields in their order ... */
    float prev_camera_pos[4];
    float offset_x, offset_y;
    int32_t max_history;
    float alpha_min, alpha_moments_min;
    float normal_min;
    float depth_tol;
    int32_t measured_below;     /* ... then: out_variance is T7's V' while N' < measured_below; 1 .. 32769 */
    int32_t search;             /* T3s: 0 or 1 */
} vrt_temporal_mom;
void vrt_temporal_mom_default(vrt_temporal_mom *t);
int vrt_temporal_hdr_mom(vrt_ctx *ctx, int width, int height, const float inv_projection[16], const float inv_view[16],
                         const float camera_pos[4], const void *d_rgb, const void *d_normal, const void *d_depth, const void *d_coverage,
                         const void *d_variance_in, const void *d_history_in, const vrt_temporal_mom *t, void *d_history_out,
                         void *d_out_rgb, void *d_out_variance, void *stream);
int vrt_temporal_hdr_mom_host(vrt_ctx *ctx, int width, int height, const float inv_projection[16], const float inv_view[16],
                              const float camera_pos[4], const float *rgb, const float *normal, const float *depth, const float *coverage,
                              const float *variance_in, const void *history_in, const vrt_temporal_mom *t, void *history_out,
                              float *out_rgb, float *out_variance);
int vrt_accum_resolve_hdr_temporal_mom(vrt_ctx *ctx, const vrt_temporal_mom *t, const vrt_filter_var *f, const vrt_tonemap *tm,
                                       const void *history_in, void *history_out, float *out_integrated, float *out_rgb,
                                       uint8_t *out_rgba8, float *out_variance);
int vrt_accum_resolve_hdr_temporal_mom_device(vrt_ctx *ctx, const vrt_temporal_mom *t, const vrt_filter_var *f, const vrt_tonemap *tm,
                                              const void *d_history_in, void *d_history_out, void *d_integrated, void *d_rgb,
                                              void *d_rgba8, void *d_variance_out, void *stream);
/* EXTENSION: guided upsampling -- radiance traced at 1 / r of the resolution (r = 1 .. VRT_UPSAMPLE_MAX_FACTOR in each direction)
 * and rebuilt at full size by a joint bilateral upsample that FULL-resolution guide planes steer. A march is about a hundred times
 * cheaper than a shaded sample, so the full-size planes cost little; the pass runs on the albedo-divided image, so per-voxel colour
 * comes back at full sharpness; and the caller gets a mask of the pixels that could not be rebuilt, which vrt_shade_rays_hdr can
 * shade exactly. Three families of calls: the guide planes of a frame (vrt_guide_frame*), the pass (vrt_upsample_hdr*), and the pass
 * on an HDR accumulation (vrt_accum_resolve_hdr_upsampled*).
 *
 * vrt_guide_frame         the guide planes of ONE sample per pixel through the pixel's corner ray (the frame's own ray, offset 0) of a
 *                         width x height frame, from the context's current camera, uniforms and tree, in the shapes
 *                         vrt_accum_guides* writes; vrt_set_guide_glass is read at the call, as vrt_guide_rays reads it. By
 *                         definition the planes are bit for bit those of vrt_accum_begin_ex(ctx, W, H, VRT_MODE_PRIMARY, 0, 0),
 *                         vrt_accum_add(ctx, 1, ..), vrt_accum_guides_device(..). HOST buffers, synchronous. Any output may be NULL,
 *                         not all of them (VRT_E_INVALID); the frame size rule is vrt_denoise's; VRT_E_STATE before an upload or a
 *                         camera has been set and while a patch batch is open. The call reads and writes no accumulation state: it
 *                         may be made in the middle of an accumulation of any size, whose resolves, counts, variance and guides
 *                         return the same bits afterwards. It takes no profiling slot. The march runs on 40 bytes per pixel of
 *                         guide state that belong to the context, grown and never shrunk; every call is ordered on it.
 * vrt_guide_frame_device  the same into DEVICE buffers; the resolve is enqueued on `stream` (NULL: the context's), after the march on
 *                         the context's stream.
 *
 * The pass. LOW is the w x h image with its planes, HIGH the W x H = r w x r h planes. All arithmetic is float32, every operation
 * rounded on its own, nothing contracted; h, g, det_expf and the tone map are vrt_filter_hdr's. p = (x, y) is a high pixel, q a low one.
 *  U1. Inputs. Colours go through h, guide floats of both sizes through g. A pixel of either size is LIVE when g(coverage) > 0.
 *  U2. Modulation. With VRT_UPSAMPLE_DEMODULATE m of a live pixel is vrt_filter_hdr's point 2 from its OWN albedo and coverage: low
 *      pixels use the low planes, high pixels the high planes. m = 1 for a pixel that is not live, and for every pixel without the
 *      flag. u_q = h(c_q) / m_q for a low pixel q.
 *  U3. Position of p in the low image. fx = ((float)x + offset_hi_x) / (float)r - offset_lo_x, x0 = floorf(fx), tx = fx - x0; the
 *      same in y. (The two frames show the same view: the shader's u = px / W * 2 - 1 gives the same bits for X / w and r X / (r w).)
 *  U4. Taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), in that order, with the bilinear weights b of T3: (1-tx)(1-ty),
 *      tx(1-ty), (1-tx)ty, tx ty. A tap is skipped when it lies outside the low image or when its liveness differs from p's: sky is
 *      never mixed into surfaces, nor surfaces into sky. For a live p and the tap q = (X, Y):
 *        dn2, da2 as in point 4 of the filter, between the tap's LOW guides and p's HIGH guides (q - p)
 *        dzq = |Z_q - Z_p|
 *        gx, gy   point 3's one-sided slopes of p on the HIGH depth plane (neighbours inside the high image and live)
 *        ddx = fabsf((float)X - fx) * (float)r, ddy = fabsf((float)Y - fy) * (float)r      the tap's distance in high pixels
 *        den = sigma_depth * ((gx * ddx + gy * ddy) + Z_p * (1.0f / 256.0f)) + 0x1p-20f
 *        e   = (dn2 * kn + da2 * ka) + dzq / den                    kn, ka as in the filter, computed once on the host
 *        w   = b * det_expf(-e)
 *      and for a p that is not live w = b. sumw = sumw + w; sum_ch = sum_ch + w * u_q[ch], from 0 in tap order.
 *  U5. Resolve. Where sumw > min_weight: u_p[ch] = sum_ch / sumw, unresolved = 0. Otherwise (a NaN sumw included) the nearest low
 *      pixel N = (clamp((int)floorf(fx + 0.5f), 0, w-1), clamp((int)floorf(fy + 0.5f), 0, h-1)) is taken whatever its liveness:
 *      u_p = u_N, unresolved = 1.
 *  U6. Output. f = h(u_p * m_p) with the HIGH pixel's m. out_rgb [H][W][3] receives f, out_rgba8 [H][W][4] the tone-mapped bytes as
 *      in point 5 of the filter, out_unresolved [H][W] one byte per pixel. Any output may be NULL, not both colour outputs.
 * Identities: with r = 1, equal offsets and the same planes on both sides every pixel has one tap of weight 1 and three of weight 0,
 * and the colour outputs are vrt_filter_hdr's at levels = 0 bit for bit. Where every guide of a region agrees, e = +0 and the pass
 * is the float32 bilinear interpolation of u.
 *
 * vrt_upsample_default    factor 2, VRT_UPSAMPLE_DEMODULATE, sigma_normal 0.5, sigma_albedo 0.05, sigma_depth 0.5, min_weight 0, offsets 0:
 *                         the best row of the quality sweep in profiles/upsample_quality.txt (DESIGN.md section 3 "Guided
 *                         upsampling", which also says where upsampling loses to the full-size image of the same cost).
 * vrt_upsample_hdr        DEVICE pointers, stream-ordered (NULL: the context's), stateless: it reads no context state, keeps no scratch
 *                         and takes no profiling slot. width, height: the LOW size. u == NULL: vrt_upsample_default. VRT_E_INVALID: a NULL
 *                         input, both colour outputs NULL, an output equal to an input or to another output, a factor outside
 *                         1..VRT_UPSAMPLE_MAX_FACTOR, unknown flag bits, a sigma that is not finite or not > 0 (or so small that
 *                         1 / sigma^2 is not finite), a min_weight outside [0, 1), an offset outside [0, 1], a tone map
 *                         vrt_accum_resolve_hdr refuses, a low or a high frame size vrt_denoise refuses.
 * vrt_upsample_hdr_host   the same through HOST buffers, synchronous, staged through 48 bytes per low and 53 per high pixel the
 *                         context keeps.
 * vrt_accum_resolve_hdr_upsampled  the pass on an HDR accumulation, which is the LOW image: the input is its float mean with its own
 *                         guide planes, brought up to date as a vrt_accum_guides call would; the high planes are vrt_guide_frame's at
 *                         r w x r h with the context's current inputs and the guide-glass rule AS BEGUN, so the two sides never mix
 *                         rules. The low offsets are replaced by 0.5 for VRT_ACCUM_JITTER and 0 otherwise, the high offsets by 0.
 *                         u == NULL: the default. HOST buffers, synchronous. VRT_E_STATE where vrt_accum_resolve_hdr_filtered returns
 *                         it, and where the context's camera, uniforms, tree or lens changed since the last vrt_accum_add: the high
 *                         planes would show another view. Mean and planes pass through the accumulation's own stage. The sums are
 *                         never touched: every resolve, vrt_accum_counts, vrt_accum_variance and the guide calls return the same bits
 *                         with and without these calls. No profiling slot is taken.
 * vrt_accum_resolve_hdr_upsampled_device  the same into DEVICE buffers of the HIGH size, enqueued on `stream` (NULL: the context's),
 *                         ordered against the adds as vrt_accum_resolve_hdr_device is.
 * Not provided: a built-in repair of unresolved pixels; a luminance or variance term; upsampling of variance or moment planes;
 * the filters chained inside the accumulation form (chain vrt_filter_hdr* on the outputs with vrt_guide_frame_device's planes); the
 * lens's origin shift; frames, views, shards and vrt_multi. */
#define VRT_UPSAMPLE_MAX_FACTOR 4
#define VRT_UPSAMPLE_DEMODULATE 1u
struct vrt_upsample {
    int32_t factor;                      /* r: 1 .. VRT_UPSAMPLE_MAX_FACTOR; W = r * w, H = r * h */
    uint32_t flags;
    float sigma_normal, sigma_albedo, sigma_depth;   /* finite, > 0, as vrt_filter's */
    float min_weight;                    /* finite, in [0, 1) */
    float offset_lo_x, offset_lo_y;      /* where in the pixel the LOW planes' ray passes: 0 corner, 0.5 jittered; in [0, 1] */
    float offset_hi_x, offset_hi_y;      /* the same for the HIGH planes */
};
typedef struct vrt_upsample vrt_upsample;
void vrt_upsample_default(vrt_upsample *u);
int vrt_guide_frame(vrt_ctx *ctx, int width, int height, float *out_normal, float *out_albedo, float *out_depth, float *out_coverage);
int vrt_guide_frame_device(vrt_ctx *ctx, int width, int height, void *d_normal, void *d_albedo, void *d_depth, void *d_coverage,
                           void *stream);
int vrt_upsample_hdr(vrt_ctx *ctx, int width, int height, const void *d_rgb, const void *d_normal, const void *d_albedo,
                     const void *d_depth, const void *d_coverage, const void *d_hi_normal, const void *d_hi_albedo,
                     const void *d_hi_depth, const void *d_hi_coverage, const vrt_upsample *u, const vrt_tonemap *tm, void *d_out_rgb,
                     void *d_out_rgba8, void *d_out_unresolved, void *stream);
int vrt_upsample_hdr_host(vrt_ctx *ctx, int width, int height, const float *rgb, const float *normal, const float *albedo,
                          const float *depth, const float *coverage, const float *hi_normal, const float *hi_albedo,
                          const float *hi_depth, const float *hi_coverage, const vrt_upsample *u, const vrt_tonemap *tm,
                          float *out_rgb, uint8_t *out_rgba8, uint8_t *out_unresolved);
int vrt_accum_resolve_hdr_upsampled(vrt_ctx *ctx, const vrt_upsample *u, const vrt_tonemap *tm, float *out_rgb, uint8_t *out_rgba8,
                                    uint8_t *out_unresolved);
int vrt_accum_resolve_hdr_upsampled_device(vrt_ctx *ctx, const vrt_upsample *u, const vrt_tonemap *tm, void *d_rgb, void *d_rgba8,
                                           void *d_unresolved, void *stream);
/* EXTENSION: auto-exposure -- light metering on the device. Every HDR route ends in vrt_tonemap { op, exposure }, and the exposure is
 * a number the caller has to know: the room seen from inside and the dragon against the sky want different ones. These calls take a
 * luminance histogram of a float image on the device (vrt_meter_hdr), turn it into an exposure with eye adaptation from frame to frame
 * (the record, a vrt_exposure that the CALLER carries), and tone map by a record that lies in device memory (vrt_tonemap_hdr), so that
 * a stream of frames never waits for the host. With the binning rule below everything but two float operations is integer arithmetic,
 * and the whole rule is the same bits on the device, on the host (vrt_meter_resolve) and in the scalar checker (tests/oracle_meter.c).
 *
 * The rule. float32 where it is float, every operation rounded on its own, nothing contracted; h is h(c) of vrt_accum_keep_hdr point
 * 1, min and max follow the conventions of the unorm8 store stated there (min(a, b) = b < a ? b : a, max(a, b) = a < b ? b : a).
 *  E1. Luminance. Y = (0.2126f * h(r) + 0.7152f * h(g)) + 0.0722f * h(b): M1's luminance (vrt_accum_keep_moments), V1's Y of the
 *      clamped channels. Y is finite, at least +0 and below 2^16: a NaN, an infinity or a negative channel has gone through h.
 *  E2. Bin. k = max((int)(bits(Y) >> 20) - 888, 0), bits the float's 32 bits as an unsigned integer: the exponent and the top three
 *      mantissa bits, counted from 2^-16 (exponent field 111, 111 * 8 = 888) -- eight bins per octave, 32 octaves. The largest
 *      possible Y, Y(65504, 65504, 65504) = 65504 in float32, lands in bin 255. Bin 0 holds everything below 2^-16 * 1.125, +0
 *      included, and counts as BLACK. No logarithm is evaluated anywhere.
 *  E3. Histogram. VRT_METER_BINS uint32 counts of the pixels of the metered rectangle; N is their number. The frame-size rule is
 *      vrt_denoise's, so N <= 2^30 and no count can wrap.
 *  E4. Window. a = (uint64)N * low_permille / 1000, b = (uint64)N * high_permille / 1000, integer divisions. Pixels are ranked by
 *      bin: bin k holds the ranks [cum_{k-1}, cum_k), cum_k the number of pixels in bins 0..k. n_k is the size of the overlap of
 *      [cum_{k-1}, cum_k) with [a, b).
 *  E5. Sums. Over k = 1..255 only: M = sum n_k and S = sum n_k * k, both uint64. Black pixels occupy ranks but never enter the sums.
 *  E6. Metered luminance. If M = 0, metered = +0.0f. Otherwise t = (S << 20) / M as a uint64 integer division,
 *      bits = (888u << 20) + (uint32)t + (1u << 19), Ym = float_from_bits(bits). This is the mean of the bins' pseudo-logarithms
 *      taken at the bins' centres, in exact integer arithmetic; when every windowed pixel lies in one bin, Ym is that bin's centre.
 *      The pseudo-logarithm is Mitchell's piecewise-linear one -- the float's bits read as a fixed-point number, exact at powers of
 *      two and linear between them -- so Ym is a geometric mean to within 0.086 octave (the largest gap between log2(1 + f) and f),
 *      not exactly.
 *  E7. Target. e* = min(max(key / Ym, min_exposure), max_exposure), one float division. If M = 0, e* = io->exposure when
 *      io->frames > 0, otherwise min(max(1.0f, min_exposure), max_exposure).
 *  E8. Adaptation. When adapt == 1.0f, or io->frames == 0, or M = 0: exposure = e*. Otherwise exposure = prev + adapt * (e* - prev)
 *      with prev = io->exposure. The record then holds exposure, metered (Ym, or +0.0f), window = M, and frames incremented,
 *      saturating at 2^32 - 1. For adapt < 1 the step never overshoots: adapt * d is not beyond d.
 *  E9. Tone map by a record. e = min(tm->exposure * E, 3.402823466e38f) with E the record's exposure; with no record e = tm->exposure.
 *      The bytes are unorm8(tone_map(x, op, e)) per channel with the tone map of vrt_accum_resolve_hdr point 4, alpha 255. With no
 *      record these are the rgba8 bytes vrt_accum_resolve_hdr gives for the same mean and tm.
 * Exact scaling: an image scaled by 2^j shifts every bin by 8 j, makes Ym exactly 2^j times larger and e* exactly 2^-j times,
 * wherever no clamp of h, bin 0 or the exposure range is met (E2 and E6).
 *
 * vrt_meter_default       key 0.18, low_permille 500, high_permille 950, min_exposure 2^-10, max_exposure 2^10, adapt 1, rectangle 0
 *                         (the whole frame).
 * vrt_meter_resolve       E4-E8 on the HOST from a histogram of VRT_METER_BINS counts: needs no context and no device. m == NULL: the
 *                         default. io: the record, read and written. Returns VRT_OK, or VRT_E_INVALID for a NULL histogram or io, a
 *                         parameter outside the ranges below, or counts that sum to more than 2^30. The device's finishing step
 *                         evaluates the same text (csrc/vrt_meter.h).
 * vrt_meter_hdr           DEVICE pointers, stream-ordered (NULL: the context's), stateless: it reads no context state, keeps no scratch
 *                         and takes no profiling slot. d_rgb: width x height pixels of 3 floats. d_histogram: VRT_METER_BINS uint32,
 *                         required -- the call's workspace and an output; the call zeroes it itself, in stream order. d_exposure: one
 *                         vrt_exposure, read and written on the device (zero it before the first frame); the host never sees it.
 *                         m == NULL: the default. VRT_E_INVALID: a NULL pointer; a pointer that is no multiple of 4; outputs that alias
 *                         the input or each other (equal pointers); a frame size vrt_denoise refuses; a rectangle that is not all
 *                         zeros and not 0 <= x0 < x1 <= width, 0 <= y0 < y1 <= height; key not finite or not > 0; not
 *                         0 <= low_permille < high_permille <= 1000; min_exposure, max_exposure not finite or not
 *                         0 < min_exposure <= max_exposure; adapt outside (0, 1].
 * vrt_meter_hdr_host      the same through HOST buffers, synchronous, on the context's stream: rgb in, the record io read and written,
 *                         out_histogram (may be NULL) the counts.
 * vrt_tonemap_hdr         E9 on n pixels (1 <= n <= 2^30): DEVICE pointers, stream-ordered, stateless as above. d_rgb: n x 3 floats;
 *                         d_out_rgba8: n x 4 bytes; d_exposure: the record, or NULL for none. tm as in vrt_accum_resolve_hdr (NULL:
 *                         VRT_TONEMAP_CLAMP, exposure 1). VRT_E_INVALID: a NULL d_rgb or d_out_rgba8, a pointer that is no multiple of
 *                         4, an output equal to an input, n outside its range, a tone map vrt_accum_resolve_hdr refuses.
 * vrt_tonemap_hdr_host    the same through HOST buffers, synchronous; e: the record, or NULL.
 * vrt_accum_resolve_hdr_metered  an HDR accumulation resolved as vrt_accum_resolve_hdr_device resolves it, into the accumulation's
 *                         own stage; the mean metered over E1-E8 (the rectangle is of the accumulation's frame) into the record;
 *                         tone mapped by the fresh record over E9. HOST buffers, synchronous: io is read and written, out_rgb
 *                         [H][W][3], out_rgba8 [H][W][4] and out_histogram [VRT_METER_BINS] may each be NULL. State errors and
 *                         ordering are vrt_accum_resolve_hdr's (VRT_E_STATE: no begin, no sample yet, begun without HDR);
 *                         VRT_E_INVALID: a NULL io, the parameters as above, a tone map vrt_accum_resolve_hdr refuses. The sums are
 *                         never touched: every other resolve, vrt_accum_counts, vrt_accum_variance and the guide calls return the same
 *                         bits with and without these calls. No profiling slot is taken.
 * vrt_accum_resolve_hdr_metered_device  the same with the record (required), the histogram, the mean and the bytes in the caller's
 *                         DEVICE memory (the last three may each be NULL; pointers multiples of 4, no two equal), enqueued on
 *                         `stream` (NULL: the context's), ordered against the adds as vrt_accum_resolve_hdr_device is.
 * Not provided: a device-side exposure inside the tone maps of the filter, temporal, upsample and display passes (ask them for the
 * float output and finish with vrt_tonemap_hdr); weighting by coverage, or centre weighting; more tone-map operators; frames, views,
 * shards and vrt_multi. */
#define VRT_METER_BINS 256
struct vrt_meter {
    float key;                            /* the luminance the metered value is mapped to; finite, > 0; default 0.18 */
    int32_t low_permille, high_permille;  /* the rank window, 0 <= low < high <= 1000; default 500, 950 */
    float min_exposure, max_exposure;     /* finite, 0 < min <= max; default 2^-10, 2^10 */
    float adapt;                          /* in (0, 1]; 1 = no adaptation; default 1 */
    int32_t x0, y0, x1, y1;               /* metered rectangle [x0,x1) x [y0,y1); all four 0 = the whole frame */
};
typedef struct vrt_meter vrt_meter;
struct vrt_exposure {     /* the caller's, carried from frame to frame; zero it before the first */
    float exposure;       /* E8 */
    float metered;        /* Ym of E6, +0.0f when nothing was metered */
    uint32_t window;      /* M of E5 */
    uint32_t frames;      /* meterings chained into this record, saturating */
};
typedef struct vrt_exposure vrt_exposure;
void vrt_meter_default(vrt_meter *m);
int vrt_meter_resolve(const uint32_t *histogram, const vrt_meter *m, vrt_exposure *io);
int vrt_meter_hdr(vrt_ctx *ctx, int width, int height, const void *d_rgb, const vrt_meter *m, void *d_histogram, void *d_exposure,
                  void *stream);
int vrt_meter_hdr_host(vrt_ctx *ctx, int width, int height, const float *rgb, const vrt_meter *m, uint32_t *out_histogram,
                       vrt_exposure *io);
int vrt_tonemap_hdr(vrt_ctx *ctx, size_t n, const void *d_rgb, const vrt_tonemap *tm, const void *d_exposure, void *d_out_rgba8,
                    void *stream);
int vrt_tonemap_hdr_host(vrt_ctx *ctx, size_t n, const float *rgb, const vrt_tonemap *tm, const vrt_exposure *e, uint8_t *out_rgba8);
int vrt_accum_resolve_hdr_metered(vrt_ctx *ctx, const vrt_meter *m, const vrt_tonemap *tm, vrt_exposure *io, float *out_rgb,
                                  uint8_t *out_rgba8, uint32_t *out_histogram);
int vrt_accum_resolve_hdr_metered_device(vrt_ctx *ctx, const vrt_meter *m, const vrt_tonemap *tm, void *d_exposure, void *d_histogram,
                                         void *d_rgb, void *d_rgba8, void *stream);
/* EXTENSION: bloom -- the glare of an HDR frame, on the device, between metering and the tone map. Every HDR route ends in
 * unorm8(tone_map(x, op, e)): a lamp of radiance 40 and one of radiance 4 both store 255 with a razor edge. These calls spread what
 * lies above a threshold over the neighbours before the tone map clips it: a bright pass, a down-sampled pyramid of L levels, an
 * up-sampling chain that adds the levels up again, and a composite fused with the tone map, which reads the exposure record
 * vrt_meter_hdr left on the device. 2 L kernel launches, no host round trip, no context state.
 *
 * The rule. float32 wherever a value is a float, every operation rounded on its own, nothing contracted; h(c), min and max are those
 * of vrt_accum_keep_hdr point 1 and vrt_meter_hdr; / is the correctly rounded division. A pyramid pixel is four floats (r, g, b, w).
 *  B0. Sizes. Level 0 is the W x H input; level l = 1..L is w_l = (w_{l-1} + 1) >> 1 by h_l = (h_{l-1} + 1) >> 1. A level may be
 *      1 x 1, and the levels after it stay 1 x 1. 1 <= L <= VRT_BLOOM_MAX_LEVELS.
 *  B1. Exposure of the bright pass. eb = min(tm->exposure * E, 3.402823466e38f) with E the device record's exposure: E9's e. With no
 *      record eb = tm->exposure; with a NULL tm, tm->exposure is 1. With a record the threshold is therefore in display units: 1.0 is
 *      what the tone map is about to clip.
 *  B2. Bright pass, per input pixel c: x_ch = h(c_ch); Y = E1's luminance of x; Ye = min(Y * eb, 3.402823466e38f);
 *      d = Ye - threshold. If knee > 0: s = min(max(d + knee, 0), knee + knee) and soft = (s * s) / (4.0f * knee); otherwise soft = 0.
 *      a = max(max(soft, d), 0); g = min(a / max(Ye, 0x1p-16f), 1.0f); b_ch = x_ch * g; w = 1.
 *  B3. Firefly weights (VRT_BLOOM_KARIS): w = 1.0f / (1.0f + Y(b)) with E1's luminance of b, then b_ch = b_ch * w. The weight
 *      travels as the fourth component through level 1 only.
 *  B4. Down-sample. Destination (X, Y) of level l reads the 4 x 4 block of level l - 1 whose columns are
 *      clamp(2X + o, 0, w_{l-1} - 1) for o = -1, 0, 1, 2, the rows likewise. The weights are [1 3 3 1] (x) [1 3 3 1] / 64, evaluated
 *      with additions only: T(a0, a1, a2, a3) is p0 = a0 + a1, p1 = a1 + a2, p2 = a2 + a3, T = (p0 + p1) + (p1 + p2). r_j = T of
 *      row j's four columns in ascending order, for the four rows in ascending order; v = T(r_0, r_1, r_2, r_3) * 0.015625f, per
 *      component. Level 1 reads B2 / B3's pixels. Level 1 with KARIS stores D_1.ch = v.ch / v.w and w = 1; every other level stores v.
 *  B5. Up-sample up(S, w, h) of an image S of w' x h' to w x h. For destination column x: nx = x >> 1 and
 *      fx = clamp(nx + ((x & 1) ? 1 : -1), 0, w' - 1); rows likewise. lerp(far, near) = ((far + near) + (near + near)) * 0.25f;
 *      t(row) = lerp(S[row][fx], S[row][nx]); up = lerp(t(fy), t(ny)).
 *  B6. Chain. U_L = D_L; for l = L-1 .. 1: U_l = D_l + up(U_{l+1}, w_l, h_l).
 *  B7. Composite. B = up(U_1, W, H) * invL with invL = 1.0f / (float)L; f_ch = h(x_ch + intensity * B_ch).
 *  B8. Outputs. out_rgb is f; out_rgba8 is unorm8(tone_map(f_ch, op, e)) with E9's e, alpha 255.
 * What follows from the weights: with threshold = knee = 0, no KARIS and eb = 1 a constant image (k, k, k), k dyadic, gives every D_l
 * and B exactly k. Scaling the image, the threshold and the knee by 2^j scales B and f exactly wherever no clamp of h and not the
 * 2^-16 floor is met. One pixel of value v in a black frame, away from the border, gives 4^l * sum(D_l) == v exactly.
 *
 * vrt_bloom_default          levels 5, VRT_BLOOM_KARIS, threshold 1, knee 0.5, intensity 0.2.
 * vrt_bloom_workspace_bytes  the bytes of d_workspace for a width x height frame and `levels`: 16 per pyramid pixel of the levels
 *                            1..L, each level rounded up to 256 bytes. 0 for arguments vrt_bloom_hdr would refuse. Needs no context.
 * vrt_bloom_hdr              DEVICE pointers, stream-ordered (NULL: the context's), stateless as vrt_meter_hdr is: it reads no context
 *                            state, keeps no scratch and takes no profiling slot. d_rgb: width x height pixels of 3 floats.
 *                            b == NULL: the default. tm as in vrt_tonemap_hdr. d_exposure: the record, or NULL for none; it is only
 *                            read. d_workspace: vrt_bloom_workspace_bytes bytes of the caller's, a multiple of 16; it needs no
 *                            initialising, the call never reads a word of it that it has not written, and its contents afterwards
 *                            mean nothing. d_out_rgb (3 floats per pixel) and d_out_rgba8 (4 bytes per pixel): either may be NULL,
 *                            not both. VRT_E_INVALID: a NULL d_rgb or d_workspace, or both outputs NULL; a workspace that is no
 *                            multiple of 16, another pointer that is no multiple of 4; an output equal to d_rgb, d_exposure, the
 *                            workspace or the other output; a frame size vrt_denoise refuses; levels outside
 *                            1..VRT_BLOOM_MAX_LEVELS; unknown flags; not 0 <= knee <= threshold <= 65504; intensity not finite or
 *                            outside [0, 65504]; a tone map vrt_accum_resolve_hdr refuses.
 * vrt_bloom_hdr_host         the same through HOST buffers, synchronous, on the context's stream; e: the record, or NULL.
 * vrt_accum_resolve_hdr_bloomed  an HDR accumulation resolved as vrt_accum_resolve_hdr_device resolves it, into the accumulation's own
 *                            stage; metered as vrt_accum_resolve_hdr_metered meters it into the record io; bloomed and tone mapped by
 *                            the fresh record. io == NULL skips the metering and there is no record (eb = e = tm->exposure). HOST
 *                            buffers, synchronous; out_rgb [H][W][3] (f) and out_rgba8 [H][W][4]: either may be NULL, not both. State
 *                            errors, ordering and the parameter checks of m are vrt_accum_resolve_hdr_metered's; those of b and tm are
 *                            vrt_bloom_hdr's. The sums are never touched. No profiling slot is taken.
 * vrt_accum_resolve_hdr_bloomed_device  the same with the record (NULL: no metering), f and the bytes in the caller's DEVICE memory
 *                            (pointers multiples of 4, no two equal), enqueued on `stream` (NULL: the context's).
 * Not provided: lens dirt, streaks, anamorphic shapes; bloom inside the filter, temporal, upsample and display passes (take their
 * float output and call vrt_bloom_hdr); frames, views, shards and vrt_multi. */
#define VRT_BLOOM_MAX_LEVELS 8
#define VRT_BLOOM_KARIS 1u
struct vrt_bloom {
    int32_t levels;      /* L, 1..VRT_BLOOM_MAX_LEVELS; default 5 */
    uint32_t flags;      /* VRT_BLOOM_KARIS or 0; default VRT_BLOOM_KARIS */
    float threshold, knee, intensity;   /* 0 <= knee <= threshold <= 65504, 0 <= intensity <= 65504; default 1, 0.5, 0.2 */
};
typedef struct vrt_bloom vrt_bloom;
void vrt_bloom_default(vrt_bloom *b);
size_t vrt_bloom_workspace_bytes(int width, int height, int levels);
int vrt_bloom_hdr(vrt_ctx *ctx, int width, int height, const void *d_rgb, const vrt_bloom *b, const vrt_tonemap *tm,
                  const void *d_exposure, void *d_workspace, void *d_out_rgb, void *d_out_rgba8, void *stream);
int vrt_bloom_hdr_host(vrt_ctx *ctx, int width, int height, const float *rgb, const vrt_bloom *b, const vrt_tonemap *tm,
                       const vrt_exposure *e, float *out_rgb, uint8_t *out_rgba8);
int vrt_accum_resolve_hdr_bloomed(vrt_ctx *ctx, const vrt_meter *m, const vrt_bloom *b, const vrt_tonemap *tm, vrt_exposure *io,
                                  float *out_rgb, uint8_t *out_rgba8);
int vrt_accum_resolve_hdr_bloomed_device(vrt_ctx *ctx, const vrt_meter *m, const vrt_bloom *b, const vrt_tonemap *tm, void *d_exposure,
                                         void *d_rgb, void *d_rgba8, void *stream);
/* EXTENSION: one whole frame of the reference's loop -- dispatch (src/main.cpp:946) then the display pass
 * (:951-967) -- with both intermediate images kept on the device; only what the caller asks for comes back.
 * HOST pointers, synchronous. out_shown_rgba8 receives what the reference puts on screen; out_rgba8 and
 * out_id_dist (either may be NULL) the two images the dispatch wrote. */
int vrt_dispatch_frame(vrt_ctx *ctx, int width, int height, int mode, uint8_t *out_shown_rgba8, uint8_t *out_rgba8,
                       int32_t *out_id_dist);

/* Per-launch timing of the dispatches that follow: a hipEvent pair is attached
 * to the kernel's dispatch packet (hipExtLaunchKernel), so it reads the kernel's
 * own begin-to-end time on the stream it runs on, for up to max_launches
 * launches (0 switches it off). vrt_profile_read waits for the recorded
 * launches, writes their durations (ms) and returns how many.
 *
 * What takes a slot: one per accepted call of vrt_dispatch, vrt_dispatch_rows, vrt_dispatch_shard, vrt_dispatch_tiles,
 * vrt_dispatch_views (its up to four views are one launch and one slot), vrt_dispatch_async, vrt_dispatch_frame (the frame; its
 * display pass takes none), vrt_shade_rays, vrt_shade_rays_device, vrt_shade_rays_hdr, vrt_shade_rays_hdr_device (the host forms
 * shade a batch in one launch), and one per iteration of vrt_dispatch_timed -- in every mode, on every variant and traversal the
 * dispatcher may take. What takes none, and does not count towards the stride either: vrt_accum_add (the frame it may launch for
 * itself included), the resolves, vrt_denoise, vrt_denoise_hdr and their host forms, vrt_cast_rays, vrt_find_voxels, and every
 * call that is refused (bad argument, open patch batch, no camera, no scene).
 * The span of a slot is the trace kernel's dispatch packet. VRT_MODE_FULL as two kernels (VRT_OPT_FULL_OPAQUE 1) is ONE slot from
 * the first kernel's begin to the second one's end. The kernels and memsets a launch may put around its trace kernel lie outside
 * the span and take no slot: the miss-mask build of VRT_OPT_MISS_TILES (a memset and a kernel before it), the feedback
 * scheduler's order kernel after a measuring launch, the memset of the tile times before a measuring launch with part-tile waves.
 * Every vrt_set_profiling call starts a new record of at most max_launches slots and restarts the stride's count; the stride
 * itself persists. tests/test_gpu_profiling.py pins all of this against event pairs of the caller's own. */
int vrt_set_profiling(vrt_ctx *ctx, int max_launches);
/* time only every `every`-th launch (launches 0, every, 2 * every, ... since vrt_set_profiling; default 1): timing every launch
 * costs a few percent of the frame rate. every < 1: VRT_E_INVALID. */
int vrt_set_profiling_stride(vrt_ctx *ctx, int every);
/* Returns the number of entries written: min(recorded launches, cap), oldest first. The read EMPTIES the record: recorded launches
 * beyond cap are dropped, and a second read returns 0 until more launches are recorded. ms_out == NULL or cap < 0: VRT_E_INVALID. */
int vrt_profile_read(vrt_ctx *ctx, float *ms_out, int cap);

int vrt_synchronize(vrt_ctx *ctx);
/* the context's own stream (hipStream_t) and device ordinal */
void *vrt_stream(vrt_ctx *ctx);
int vrt_device(const vrt_ctx *ctx);

/* kernel variant selection (0 = default). The library holds the default and the fallbacks its dispatcher may take
 * (variants 0, 1, 4, 20, 22): vrt_variant_available() says which, vrt_set_variant() returns VRT_E_INVALID for the others. */
int vrt_set_variant(vrt_ctx *ctx, int variant);
int vrt_variant_available(int variant);

/* Feedback scheduling of the tracing kernel and the display pass (on by default, period 16). Frames that repeat a
 * launch shape on a stream -- the reference's loop dispatches the same W x H every frame (main.cpp:946) -- start
 * their tiles heaviest first, using the tile times measured on the shape's second launch (the first may be cold) and
 * on every `period`-th one after it (period 1: on all of them); this shortens the tail of a launch (1080p dragon:
 * primary rays -10 %, full shader -13 %, display pass -17 %); a jump of the camera triggers a fresh measurement at
 * once. Pixels do not depend on it. period = 0 switches it off: tiles then start in row-major order. Applies to
 * one-view launches of the default variant in all three modes and to vrt_denoise / vrt_dispatch_frame. */
int vrt_set_tile_scheduling(vrt_ctx *ctx, int period);

/* Switches of the dispatcher. Pixels never depend on them: both settings of each are held to the same oracle frames by the parity
 * suite, which is what they exist for (and for A/B timing).
 *   VRT_OPT_RAY_TABLES     1 (default): views whose inverse projection has the shape of a perspective or orthographic matrix read the
 *                          per-column / per-row part of ray generation (raytracing.comp:626-634) from tables made once per projection;
 *                          0: every launch runs the shader's own prologue.
 *   VRT_OPT_EMPTY_OCTANTS  1 (default): when the tree is empty outside one aligned cube (every scene loaded at the origin of the
 *                          reference's [-1023,1024)^3 world), rays that leave it end there and the deepest node that still holds
 *                          everything stands in for the root; 2: the same without the tighter root; 0: off (rays walk the empty octants).
 *   VRT_OPT_DISPLAY_KERNEL 0 (default): the display pass sums two pixels per lane and every wave takes the cheaper of two walks over its
 *                          staged window: the rows and column segments any of its 64 lanes needs, the same for all lanes (faces that fill
 *                          the window: close-ups), or every pixel the box its own voxel face occupies (faces small against the window:
 *                          1080p dragon frame 0.186 -> 0.123 ms with the staging changes that came with it); 2 / 3: always the first / the second walk (A/B, tests);
 *                          any other value: VRT_E_INVALID.
 *   VRT_OPT_FULL_OPAQUE    VRT_MODE_FULL where pathTrace cannot branch: in a scene without translucent voxels seen from empty space it is
 *                          the primary ray, a shadow ray and ONE diffuse bounce ray that spawns nothing (comp:573-616), so the 8-deep ray
 *                          stack is never used. 6 (default): such launches run a kernel that holds no stack -- primary + shadow stage, then
 *                          the bounce stage in the same wave, 80 registers instead of 96 + 560 B of scratch: 0.137 against 0.172 ms on the
 *                          1080p dragon frame; 5, 7: the same built for five / seven waves per SIMD; 1: the two stages as two kernels with
 *                          a 20-byte seed per pixel between them (0.158 ms: the experiment the one-kernel form came from); 0: always the
 *                          general kernel. Scenes with a translucent voxel and eyes inside a medium take the general kernel whatever the
 *                          setting.
 *   VRT_OPT_HEAVY_TILES    1 (default): the general VRT_MODE_FULL kernel, on launches the feedback scheduler has an order for, traces the
 *                          few heaviest groups of tiles (those above 3/4 of the heaviest one's time, at most 64, when the heaviest tile outlasts 3/4 of its even share of the frame) as eight
 *                          waves per 8x8 tile instead of one. A frame of a translucent scene is as long as its longest wave -- dozens of
 *                          rays one after the other, each round as long as the longest of the wave's marches; with 8 pixels per wave that
 *                          is the longest of 8 instead of 64 (profiles/r03_room_critical_path.txt). 0: every tile is one wave.
 *   VRT_OPT_MISS_TILES     1 (default): primary and primary + shadow launches of the default kernel from an eye in empty space, for views
 *                          with ray tables, skip the march of every pixel whose ray provably hits nothing: the dispatcher keeps a list of
 *                          boxes covering every voxel that can stop such a ray (made for a tree and bounds that stood unchanged) and, per
 *                          view, a mask of the 8x8 tiles no dilated box projects into (one small kernel the second time a view and
 *                          frame shape are seen, once the tree has stood unchanged for max(64, records / 512) such views; DESIGN 3
 *                          "Miss tiles" has the proof); those pixels take the miss outputs at once (1080p dragon 0.0454 -> 0.0379 ms). 0: every pixel is marched (A/B, tests). */
#define VRT_OPT_RAY_TABLES 1
#define VRT_OPT_EMPTY_OCTANTS 2
#define VRT_OPT_DISPLAY_KERNEL 3
#define VRT_OPT_FULL_OPAQUE 4
#define VRT_OPT_HEAVY_TILES 5
#define VRT_OPT_MISS_TILES 6
int vrt_set_option(vrt_ctx *ctx, int option, int value);

/* The feedback scheduler's order, read and overridden. vrt_get_tile_order copies the current workgroup-group order for the shape last
 * launched on `stream` (NULL: the context's) into out[cap] and returns the number of groups n (0 while no order has been derived);
 * when cap > n, out[n] receives how many groups at the head of the order VRT_MODE_FULL launches trace as part-tile waves
 * (VRT_OPT_HEAVY_TILES; 0 for shapes of other modes).
 * vrt_set_tile_order(enable = 1) makes one-view launches of the default kernel take caller-owned DEVICE buffers instead of the
 * scheduler's: d_group_order (a permutation of the launch's groups of four 8x8 tiles, or NULL: row-major) and d_tile_cost (one uint32
 * per tile, receives each tile's clock ticks, or NULL); enable = 0 hands the launches back to the scheduler. Any permutation renders
 * the same pixels. */
long vrt_get_tile_order(vrt_ctx *ctx, void *stream, uint32_t *out, size_t cap);
int vrt_set_tile_order(vrt_ctx *ctx, int enable, const void *d_group_order, void *d_tile_cost);

const char *vrt_version(void);

#ifdef __cplusplus
}
#endif
#endif
