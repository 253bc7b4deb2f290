// vrt_internal.h -- what the translation units of libvrt_hip.so share: the context behind `vrt_ctx` (every device buffer it keeps
// is a DevBuf member of it or of its nested structs: `delete c` frees them all), the kernel variant table, error plumbing and the
// few helpers that cross files. Host code only; nothing here is exported.
//
//   vrt_devbuf.h       DevBuf<T>, the owner of every device buffer below: reserve() is the one way to grow, the destructor the one
//                      free. A new buffer is a DevBuf member, its owner waits for what may still use the old block in front of
//                      reserve(), and vrt_destroy gets no line for it
//   vrt_stage.h        Stage, the staging of every entry point that takes host buffers: the planes a call declares give the size of
//                      its block, each plane's device pointer, the copies up, the copies down and the final wait
//   vrt_scene.cpp      create / destroy, uniforms, camera, uploads, the layouts on the device (ensure_analysis); what every launch
//                      takes from them: the scene and light blocks of KArgs, the base variant, the profiling slot; growth of the
//                      buffers the context's stream orders (reserve_synced: scratch images, staging, the accumulation's groups)
//   vrt_dispatch.cpp   enqueue(), a frame launch in steps: views, variant, frame block of KArgs, feedback scheduling, the form of the
//                      full path tracer; the caches behind them (ray tables, miss masks, seed buffers); the vrt_dispatch* entry points
//   vrt_display.cpp    the display pass and the fused frame call
//   vrt_patch.cpp      edits without re-upload: patch plan / apply / batches / compaction
//   vrt_query.cpp      world queries on the device tree: ray casts (picking), voxel lookups
//   vrt_rays.cpp       pathTrace for ray batches of the caller's (vrt_shade_rays): arguments without a camera, the staging buffers
//   vrt_accum.cpp      progressive multi-sample accumulation (any mode, sub-pixel jitter): begin / add / resolve, the restart rule,
//                      and the launches of one step of it (launch_accum_step, called by enqueue())
//   vrt_guides.cpp     guide planes (vrt_accum_guides, vrt_guide_rays): the accumulation's guide state, the samples it still lacks,
//                      their launch through enqueue() (an AccumStep with `guides`), the resolve; the stateless ray-batch form
//   vrt_meter.cpp      light metering (vrt_meter_hdr, vrt_tonemap_hdr, vrt_accum_resolve_hdr_metered): validation, the launches, the
//                      host forms' staging; the rule itself is vrt_meter.h's, shared with the finishing kernel
//   vrt_bloom.cpp      bloom (vrt_bloom_hdr, vrt_accum_resolve_hdr_bloomed): validation, the 2 L launches of a call, the host form's
//                      staging; the pyramid's sizes and the workspace's layout are vrt_bloom.h's
//   vrt_raygen.cpp     per-projection ray-generation tables (pure host arithmetic)
//   vrt_launch_*.hip   the ONLY files that hold device code: kernel instantiations behind vrt_launch.h
//   vrt_multi.hip      several devices behind one handle (uses the public API of the per-device contexts; its shard and band
//                      images are DevBufs too)
#pragma once
#include "../../include/vrt.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "vrt_args.h"
#include "vrt_sun.h"
#include "vrt_emitters.h"
#include "vrt_devbuf.h"
#include "vrt_layout.h"
#include "vrt_miss.h"

// Variant 0 is what the library ships: the v4 traversal, seven waves per SIMD (five for the full path tracer, which runs
// v4's general march loop); the dispatcher takes v3 when a primary / primary + shadow launch has its eye inside a medium,
// v2 when the scene has no wide form, v1 when it has a unit-size internal node. Variants 1, 4 and 20 select those fallbacks
// explicitly, and 22 is variant 0 without the full path tracer's opaque and two-pass forms (tests). vrt_set_variant() refuses
// every other number. A wave traces an 8 x 8 pixel tile; a workgroup is one wave for the wide traversals (v3, v4) and four
// for the record-array ones (v1, v2).
struct Variant {
    int id;     // the public number (vrt_set_variant)
    int trav;   // 4, 3: wide layout (vrt_kernels_v4.hip.h, vrt_kernels_wide.hip.h); 2: bit-indexed descent with restart
                // anchors (vrt_kernels.hip.h); 1: baseline (vrt_kernels_v1.hip.h)
    int wpe;    // waves per SIMD the register allocator is held to (1 = unconstrained)
    int block() const { return trav >= 3 ? 64 : 256; }   // threads per workgroup
};

inline constexpr Variant kVariants[] = {
    {0, 4, 7},
    {1, 1, 1},
    {4, 2, 1},
    {20, 3, 6},   // v3 as round 1 shipped it (six waves per SIMD; seven with the shadow march)
    {22, 4, 7},   // == variant 0 but for the dispatcher's choice of the full path tracer's form
};
inline const Variant *find_variant(int id) {
    for (const Variant &v : kVariants)
        if (v.id == id) return &v;
    return nullptr;
}

// Feedback scheduling state of one launch shape on one stream. Launches that repeat a shape on a stream (the frames of
// a camera path) share it: every sched_period-th of them also records what each tile cost, tile_order_kernel turns that
// into a heaviest-first workgroup order on the same stream, and the launches that follow start their workgroups in
// that order. The order is a permutation whatever the costs are, so a stale one (camera moved, scene edited) only
// loses speed, never pixels; states are per stream because the order buffer is rewritten in stream order.
struct SchedState {
    hipStream_t stream = nullptr;
    int width = 0, n_rows = 0, row0 = 0, row_stride = 0, tile_rows = 0, mode = 0;
    uint32_t n_tiles = 0, n_groups = 0;
    DevBuf<uint32_t> d_cost, d_order;
    bool valid = false;        // d_order holds an order
    float cam[6] = {0, 0, 0, 0, 0, 0};  // eye and viewing direction of the launch the order was measured on (trace states)
    uint64_t launches = 0;
    uint64_t last_use = 0;
};

struct vrt_ctx {
    int device = 0;
    int n_cus = 256;
    hipStream_t stream = nullptr;
    DevBuf<uint2> d_nodes;    // the record array: bytes() is its capacity, info.n_records what it holds
    bool have_scene = false;
    bool have_camera = false;
    vrt_scene_info info{};
    vrt_params params{};
    float inv_proj[16]{}, inv_view[16]{}, cam_pos[4]{};
    float lens[2] = {0.0f, 1.0f};   // vrt_set_lens: aperture, focus distance (the progressive accumulation only)
    int path_depth = 1;             // vrt_set_path_depth: the samples of VRT_MODE_FULL in accumulations and ray batches (frames: always 1)
    float sun_disc = 0.0f;          // vrt_set_sun_disc: the tangent of the sun's angular radius, honoured where the path depth is
    bool emitter_sampling = false;  // vrt_set_emitter_sampling: next-event estimation towards the emitter list, honoured where the path depth is
    int emitter_importance = VRT_EMIT_UNIFORM;   // vrt_set_emitter_importance: how a vertex picks from the list; read only where sampling is on and the list is not empty
    bool emitter_mis = false;       // vrt_set_emitter_mis: read only where sampling is on, the list is not empty and the mode is VRT_EMIT_POWER
    // the emitter list (vrt_emitters.cpp ensure_emitters()) of the tree generation and world bounds it was made for
    struct Emitters {
        bool built = false;
        uint64_t tree_gen = 0;
        int wmin[3] = {0, 0, 0}, wmax[3] = {0, 0, 0};
        uint64_t n = 0;                  // N; above VRT_MAX_EMITTERS nothing is held
        std::vector<int32_t> list;       // 4 per entry: lo.x, lo.y, lo.z, size
        DevBuf<int32_t> d_list;          // the same on the device
        std::vector<uint32_t> cdf;       // one threshold per entry (vrt_emitters.h emitter_cdf()), made and uploaded with the list
        DevBuf<uint32_t> d_cdf;
        uint64_t wtot = 0;               // the sum of the list's integer weights W_j, kept when the table is made (vrt_set_emitter_mis)
    };
    Emitters emitters;
    int variant = 0;
    int denoise_variant = 0;  // VRT_OPT_DISPLAY_KERNEL = denoise::Args::rows_path: 0 each wave the cheaper walk; 2, 3: one walk forced
    // scratch outputs for the host-buffer dispatch
    DevBuf<void> d_rgba, d_id, d_shown;
    size_t scratch_pixels = 0;
    // ... and the two float images of vrt_denoise_hdr_host (vrt_display.cpp)
    DevBuf<void> d_hdr_in, d_hdr_out;
    size_t hdr_scratch_pixels = 0;
    // the guided filter's scratch (vrt_filter.cpp): the packed guides and the two level images of vrt_filter_hdr and vrt_filter_hdr_var,
    // shared by their calls on any stream -- `done` is recorded after each call's launches and awaited by a call on another stream --
    // and the staging of their host forms (inputs and outputs: vrt_filter.cpp declare())
    struct FilterScratch {
        DevBuf<float4> d_pack, d_ping, d_pong;
        hipEvent_t done = nullptr;
        hipStream_t last = nullptr;
        bool used = false;
        DevBuf<float> d_host;
        FilterScratch() = default;
        FilterScratch(const FilterScratch &) = delete;
        FilterScratch &operator=(const FilterScratch &) = delete;
        ~FilterScratch() { if (done) (void)hipEventDestroy(done); }
    };
    FilterScratch filter;
    // the staging of vrt_temporal_hdr_host (vrt_temporal.cpp, where its planes are declared): both histories, the inputs and the outputs
    DevBuf<float4> d_temporal;
    // vrt_guide_frame* (vrt_guides.cpp): the guide state of one sample per pixel of a frame, 40 bytes per pixel, grown and never
    // shrunk; the march and every growth are ordered on the context's stream, a caller's stream that resolves it is joined back
    struct GuideFrame {
        DevBuf<void> d_state;
        DevBuf<float> d_host;                    // vrt_guide_frame's four planes on their way to the host
        hipEvent_t marched = nullptr, read = nullptr;
        GuideFrame() = default;
        GuideFrame(const GuideFrame &) = delete;
        GuideFrame &operator=(const GuideFrame &) = delete;
        ~GuideFrame() {
            if (marched) (void)hipEventDestroy(marched);
            if (read) (void)hipEventDestroy(read);
        }
    };
    GuideFrame guide_frame;
    // the staging of vrt_upsample_hdr_host (vrt_upsample.cpp, where its planes are declared)
    DevBuf<float> d_upsample;
    // the staging of vrt_meter_hdr_host and vrt_tonemap_hdr_host (vrt_meter.cpp, where their planes are declared)
    DevBuf<float> d_meter;
    // the staging of vrt_bloom_hdr_host (vrt_bloom.cpp, where its planes are declared): input, record, pyramid, outputs
    DevBuf<float4> d_bloom;
    // device buffers behind vrt_cast_rays / vrt_find_voxels (vrt_query.cpp)
    DevBuf<void> d_query;
    // device buffers behind vrt_shade_rays (vrt_rays.cpp)
    DevBuf<void> d_rays;
    // edits collected between vrt_patch_begin and vrt_patch_end: applied to the host structures at once, sent to the
    // device together
    struct PatchBatch {
        bool open = false, dirty = false;
        size_t records_before = 0, cells_before = 0;
        std::vector<uint32_t> rewritten_records;
        std::vector<size_t> repointed_cells;
        bool roots_changed = false, wide_invalid = false;
        long texel_delta = 0;
    };
    PatchBatch batch;
    // vrt_dispatch_async: two lanes, each a stream + device images + "the copies have landed" event
    struct AsyncLane {
        hipStream_t stream = nullptr;
        DevBuf<void> d_rgba, d_id;
        size_t pixels = 0;
        hipEvent_t done = nullptr;
        bool busy = false;
    };
    AsyncLane lane[2];
    int next_lane = 0;
    // optional per-launch hipEvent pairs (vrt_set_profiling)
    bool profiling = false;
    std::vector<hipEvent_t> prof_events;  // 2 per slot
    size_t prof_count = 0, prof_cap = 0;  // slots recorded / slots of the current vrt_set_profiling (the events of a larger earlier one are kept)
    size_t prof_seen = 0, prof_stride = 1;  // every prof_stride-th launch is bracketed
    // host copy of the records: lets the dispatcher check the bit-indexed traversal's precondition
    // against the CURRENT world bounds (they arrive separately, through vrt_set_params)
    std::vector<vrt::Record> host_records;
    size_t uploaded_records = 0;  // size of host_records after the last full upload (patches append to it)
    size_t stream_texels = 0;     // texels of the reference's stream for the current tree (kept current by patches)
    bool dim_from_texels = false; // the uploaded tex_dim was ceil(cbrt(texels)): patches keep it that way
    bool analysis_valid = false;
    bool unit_internal = false;
    // wide layout (vrt_layout.h), rebuilt whenever the tree or the world bounds change
    bool wide_ok = false;
    vrt::WideTree wide;
    DevBuf<uint2> d_cells;        // cells_capacity cells in the layout of vrt_layout.h, then as many in the v4 form (cells4)
    DevBuf<uint32_t> d_roots;     // 16 words: record and wide node of each wide root (vrt_common.hip.h KArgs::root_table)
    size_t cells_capacity = 0;
    // feedback scheduling of the default kernel (see SchedState)
    int sched_period = 16;                   // every n-th launch of a shape measures its tiles; 0 = off
    std::vector<SchedState> sched;
    uint64_t sched_tick = 0;
    bool order_lds_raised = false;            // tile_order_kernel's dynamic-LDS ceiling raised on THIS context's device
    // ray-generation tables, one per (inverse projection, width, height) seen lately (ray_table() below)
    struct RayTable {
        float inv_proj[16]{};
        int width = 0, height = 0;
        bool ok = false;            // the projection has the separable shape and the tables are on the device
        float z = 0.0f;
        DevBuf<float> d_tab;        // width floats (x per column) then height floats (y per row)
        bool fit_ok = false;        // `fit` holds the miss-tile build's part of the tables (vrt_raygen.cpp miss_table_fit)
        vrt::miss::TableFit fit{};
        uint64_t last_use = 0;
    };
    std::vector<RayTable> ray_tables;
    uint64_t ray_tick = 0;
    // miss tiles (VRT_OPT_MISS_TILES, vrt_miss.h): the occupancy boxes (vrt_layout.h occupancy_boxes) of the tree and world bounds
    // the last mask was built for; and one mask per (view, frame shape, tree_gen, bounds) seen lately
    bool miss_tiles_on = true;
    struct Occupancy {
        bool built = false, ok = false;
        uint64_t tree_gen = 0;
        int wmin[3] = {0, 0, 0}, wmax[3] = {0, 0, 0};
        uint64_t seen_gen = ~0ull;         // the tree generation and bounds mask requests have seen, and for how many requests
        int seen_wmin[3] = {0, 0, 0}, seen_wmax[3] = {0, 0, 0};
        uint64_t stable = 0;
        DevBuf<int> d_boxes;               // n_boxes vrt::miss::Box
        size_t n_boxes = 0;
    };
    Occupancy occ;
    struct MissMask {
        float inv_proj[16]{}, inv_view[16]{}, gro[3]{};
        int width = 0, height = 0;
        uint64_t tree_gen = 0;             // ... the tree and world bounds it was made for
        int wmin[3] = {0, 0, 0}, wmax[3] = {0, 0, 0};
        bool pending = false;              // the key has been seen once: the next sight builds the mask
        bool ok = false;                   // d_mask holds this view's mask (or is being built on `stream`)
        DevBuf<uint32_t> d_mask;           // View::miss: the header word, a spare word, then the tile bytes
        uint8_t stamp = 0;                 // of the last build: View::miss_stamp
        bool shared = false;               // a launch on another stream than `stream` has read it since the build
        hipStream_t stream = nullptr;
        hipEvent_t built = nullptr;        // recorded on `stream` right after the build
        uint64_t last_use = 0;
    };
    std::vector<MissMask> miss_masks;
    uint64_t miss_tick = 0;
    // VRT_MODE_FULL as two passes (vrt_launch.h trace_full_two_pass): the option, what the uploaded tree allows, the seed buffers
    bool two_pass_on = true;                     // vrt_set_option(VRT_OPT_FULL_OPAQUE)
    bool heavy_split_on = true;                  // KArgs::split_count (VRT_OPT_HEAVY_TILES)
    int two_pass_form = 6;                       // 6 (default): both stages in one kernel built for six waves per SIMD; 5, 7: for five, seven; 1: two kernels
    bool scene_opaque = false;                   // every leaf has alpha 0, or alpha 255 and a refraction byte that is a surface (not 0 / 85)
    bool scene_opaque_valid = false;
    struct SeedBuffer { hipStream_t stream = nullptr; DevBuf<uint32_t> d; size_t tiles = 0; uint64_t last_use = 0; };
    std::vector<SeedBuffer> seeds;               // one per stream: launches on different streams may overlap
    uint64_t seed_tick = 0;
    bool tight_root_on = true;                   // VRT_OPT_EMPTY_OCTANTS 2 = on without the tighter root
    bool root0_only_on = true;                   // VRT_OPT_EMPTY_OCTANTS 0: never tell the kernels that the world is empty outside wide root 0
    bool ray_tables_on = true;                   // VRT_OPT_RAY_TABLES 0: always the shader's own prologue (A/B, tests)
    // every change of the tree (upload, patch, batch end, compaction) counts one: the accumulation's restart rule compares it
    uint64_t tree_gen = 0;
    // the progressive accumulation of VRT_MODE_FULL (vrt_accum.cpp): one per context
    struct Accum {
        bool begun = false;
        int width = 0, height = 0;
        uint32_t first = 0;                      // initRNG sampleIndex of the first sample in the sums
        uint32_t total = 0;                      // samples in the sums
        bool pass1 = false;                      // d_seed and d_pass1 hold pass 1 of the current samples (opaque path)
        int mode = VRT_MODE_FULL;                // vrt_accum_begin_ex: the mode and VRT_ACCUM_* flags of the samples
        uint32_t flags = 0;
        bool frame = false;                      // d_pass1 and d_id hold the mode's unjittered frame (jitter, or modes 0 / 1)
        // what every sample depends on, as it was at the first sample in the sums
        float inv_proj[16]{}, inv_view[16]{}, cam_pos[4]{};
        float lens[2] = {0.0f, 1.0f};
        int path_depth = 1;
        float sun_disc = 0.0f;
        bool emitter_sampling = false;
        const int32_t *emit_list = nullptr;      // the context's emitter list as the add that queues a step found it (emitters.d_list, N)
        uint32_t emit_n = 0;
        int emitter_importance = VRT_EMIT_UNIFORM;
        const uint32_t *emit_cdf = nullptr;      // ... and its thresholds (emitters.d_cdf)
        bool emitter_mis = false;                // vrt_set_emitter_mis as the sums took it: the flag where it is read, false elsewhere
        float emit_inv_power = 0.0f;             // ... and 1 / Wtot of the list (emitter_inv_power())
        vrt_params params{};
        uint64_t tree_gen = 0;
        DevBuf<uint32_t> d_sums;                 // 4 words per pixel
        DevBuf<uint32_t> d_pass1;                // pass 1's rgba8 (opaque path), or the unjittered frame's (`frame`)
        DevBuf<int2> d_id;                       // the frame's (voxel ID, dist)
        DevBuf<uint32_t> d_seed;                 // pass 1's seeds, tile-major (kSeedPlanesHost words per pixel)
        size_t pixels = 0, seed_tiles = 0;       // what the four above were last sized for
        hipEvent_t added = nullptr, read = nullptr;   // ordering against a caller's stream in vrt_accum_resolve_device
        // vrt_accum_begin_adaptive: the stopping rule; per pixel, the count in the fourth word of d_sums and Q in d_sq
        bool adaptive = false;
        uint32_t min_samples = 0, max_samples = 0, tolerance = 0;
        DevBuf<uint64_t> d_sq;
        DevBuf<uint32_t> d_tiles;                // the round's tile list [tile_cap], then its count and vrt_accum_counts' count
        size_t sq_pixels = 0, tile_cap = 0;      // what the two above were last sized for
        // vrt_accum_keep_hdr as it stood at the begin: the float64 sums of the samples' float colours beside everything above
        bool hdr = false;
        DevBuf<double> d_hsum;                   // 3 doubles per pixel
        DevBuf<float> d_hframe;                  // 3 floats per pixel: the corner frame's (or pass 1's) float colour
        size_t hdr_pixels = 0;                   // what the two above were last sized for
        DevBuf<float> d_hrgb;                    // vrt_accum_resolve_hdr's float image on its way to the host
        DevBuf<float> d_hmean;                   // vrt_accum_resolve_hdr_shown*: the float mean the display pass reads, made at the first such call
        // vrt_accum_keep_moments as it stood at the begin of an HDR accumulation: the two float64 sums of the samples' luminance and its square
        bool moments = false;
        DevBuf<double> d_msum;                   // 2 doubles per pixel
        size_t mom_pixels = 0;                   // what it was last sized for
        DevBuf<float> d_mvar;                    // M3's plane: vrt_accum_variance's way to the host, the variance-guided resolve's input; made at the first such call
        // vrt_accum_guides (vrt_guides.cpp): the guide state, made at the first such call. `epoch` counts the starts of the sums (every
        // begin and every restart of vrt_accum_add); the state holds the guides of the first guide_total samples of epoch guide_epoch
        uint64_t epoch = 0, guide_epoch = 0;
        uint32_t guide_total = 0;
        DevBuf<void> d_guides;                   // vrt_guides.h State: 40 bytes per pixel
        size_t guide_pixels = 0;                 // what it was last sized for
        DevBuf<float> d_gout;                    // vrt_accum_guides' four planes on their way to the host
        bool guide_glass = false;                // vrt_set_guide_glass as it stood at the begin: the rule of every sample in the guide state
        DevBuf<float> d_filter;                  // vrt_accum_resolve_hdr_filtered*: mean, planes and outputs (vrt_filter.cpp declare());
                                                 // vrt_accum_resolve_hdr_temporal*: those, the integrated image and the host form's histories (vrt_temporal.cpp temporal_accum())
    };
    Accum accum;
    bool accum_keep_hdr = false;                 // vrt_accum_keep_hdr: read by the next vrt_accum_begin*
    bool accum_keep_moments = false;             // vrt_accum_keep_moments: likewise, and only where that begin keeps HDR sums
    bool guide_glass = false;                    // vrt_set_guide_glass: read by the next vrt_accum_begin*, and by vrt_guide_rays* at the call
    const uint32_t *dbg_group_order = nullptr;  // vrt_set_tile_order: caller-owned buffers instead of the scheduler's
    uint32_t *dbg_tile_cost = nullptr;
    bool dbg_sched = false;
    std::string err;
};

inline int vrt_fail(vrt_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}

#define VRT_HIP(c, call)                                                                   \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess)                                                              \
            return vrt_fail((c), VRT_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace vrt_internal {

// vrt_scene.cpp
int ensure_analysis(vrt_ctx *c);     // (re)derives what depends on the world bounds: wide layout on the device, root table
int reserve_cells(vrt_ctx *c, size_t n_cells);
int upload_cells(vrt_ctx *c, size_t from, size_t n);
int upload_roots(vrt_ctx *c);
uint32_t dim_of_texels(size_t texels);   // src/main.cpp:266-268
int check_frame(vrt_ctx *c, int width, int height);
// Growth of buffers that only work ordered by the context's stream touches: waits for that stream, then reserves every
// {buffer, bytes} of `wants`. The caller has found one of them too small, and sets the count they share once this has succeeded.
struct Want { DevMem *buf; size_t bytes; };
int reserve_synced(vrt_ctx *c, std::initializer_list<Want> wants);
int reserve_staging(vrt_ctx *c, DevMem &buf, size_t bytes);   // ... one staging buffer (queries, ray batches), grown to 1.5 x bytes
int ensure_scratch(vrt_ctx *c, size_t px);   // device images behind the host-buffer entry points
// a vrt_tonemap the header defines (NULL: VRT_TONEMAP_CLAMP, exposure 1), else VRT_E_INVALID in the name of `what`
int check_tonemap(vrt_ctx *c, const char *what, const vrt_tonemap *tm);
// What frames, ray batches and queries put into KArgs the same way (after ensure_analysis). The scene block: everything a kernel
// reads of the tree and the world, wide root 0 as build_wide() found it -- and not root0_only, which each caller decides for
// itself. The light block: the uniforms of the shading and the shadow ray's set-up.
void fill_scene_args(const vrt_ctx *c, vrt::KArgs &a);
void fill_light_args(const vrt_ctx *c, vrt::KArgs &a);
// The context's emitter list for the current tree and bounds (vrt_emitters.cpp), made if it is not: c->emitters. VRT_E_STATE before an
// upload and while a patch batch is open; with `sampling` also where the list exceeds VRT_MAX_EMITTERS.
int ensure_emitters(vrt_ctx *c, const char *what, bool sampling);
// sun_block(light_dir, tan_radius), the sun disc's block for a launch whose light direction is light_dir: vrt_sun.h
// The context's variant (vrt_set_variant) as this scene allows it: the record-array kernels without a wide layout, the
// explicit-AABB ones where a unit-size node is internal. Frames and ray batches start from it.
Variant base_variant(const vrt_ctx *c);
// The event pair of the next bracketed launch (vrt_set_profiling), or nothing: taken before a launch that could carry events
// (every prof_stride-th of them while slots are left), committed once that launch has succeeded.
struct ProfSlot {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool taken = false;
    static ProfSlot take(vrt_ctx *c) {
        ProfSlot p;
        p.taken = c->profiling && (c->prof_seen++ % c->prof_stride) == 0 && c->prof_count < c->prof_cap;
        if (p.taken) { p.ev0 = c->prof_events[2 * c->prof_count]; p.ev1 = c->prof_events[2 * c->prof_count + 1]; }
        return p;
    }
    void commit(vrt_ctx *c) const { if (taken) ++c->prof_count; }
};

// vrt_dispatch.cpp
// AccumStep: instead of rendering a frame, add samples first .. first + n - 1 of VRT_MODE_FULL to the context's accumulation
// (vrt_accum.cpp; whole frame, the context's camera, d_rgba / d_id unused)
// (jitter: the jittered samples of VRT_ACCUM_JITTER, in `mode`; vrt_accum.hip.h JitterSource)
// (aperture > 0: the samples of a thin lens, vrt_set_lens; vrt_accum.hip.h LensSource, vrt_lens.hip.h)
// (adaptive: n rounds of the context's adaptive accumulation, vrt_accum_begin_adaptive; the kernels' adaptive forms)
// (moments, with hdr: the accumulation keeps luminance moments, vrt_accum_keep_moments; the kernels' MOM forms)
// (hdr: an HDR accumulation, vrt_accum_keep_hdr; the kernels' HDR forms. frame_only, with hdr, modes 0 / 1 from the corner: no
// sample, but the mode's frame -- bytes, id_dist, float colour -- into the accumulation's buffers, for the repeat path)
// (paths: what selects the kernels of VRT_MODE_FULL, as the add that queues the step read it)
// (guides, in VRT_MODE_PRIMARY: not the samples' colour into the sums but their first-hit guides into the accumulation's guide
// state, vrt_guides.cpp; jitter, aperture and focus as above, nothing else of the step is read. glass: by the past-glass rule --
// enqueue() takes the plain kernels all the same where the tree holds no translucent leaf and every origin is in empty space)
// PathSetup: the settings that select the family of path tracer kernels of a VRT_MODE_FULL launch and fill its argument block
// (vrt_launch.h select_paths()), as an accumulation step or a ray batch read them
struct PathSetup {
    int path_depth = 1;             // vrt_set_path_depth
    float sun_radius = 0.0f;        // vrt_set_sun_disc: the tangent of the radius, 0: no disc
    bool sampling = false;          // vrt_set_emitter_sampling
    int importance = VRT_EMIT_UNIFORM;   // vrt_set_emitter_importance
    bool mis = false;               // vrt_set_emitter_mis
    const int32_t *list = nullptr;  // the context's emitter list, its length, its thresholds and 1 / Wtot (vrt_emitters.cpp)
    uint32_t n = 0;
    const uint32_t *cdf = nullptr;
    float inv_power = 0.0f;
    // emitter sampling as a launch sees it -- an empty list gives the launches of sampling off: the general path tracer over
    // EmitPaths<...>, never the opaque routes
    bool emit() const { return sampling && n > 0; }
};
struct AccumStep {
    uint32_t first, n;
    bool jitter;
    float aperture = 0.0f, focus = 1.0f;
    bool adaptive = false, hdr = false, frame_only = false;
    PathSetup paths{};
    bool guides = false;
    bool glass = false;             // with guides: the past-glass rule (vrt_set_guide_glass as the accumulation's begin read it)
    bool moments = false;
    void *guide_state = nullptr;    // with guides: the state to march into instead of the accumulation's (vrt_guide_frame, whose frame
                                    // size is the launch's own); nothing of the accumulation is read or written then
};
int enqueue(vrt_ctx *c, int width, int height, int row0, int n_rows, int tile_rows, int row_stride, int compact, int mode,
            void *d_rgba, void *d_id, hipStream_t s, const vrt_view *views = nullptr, int n_views = 1, const AccumStep *acc = nullptr);
SchedState *sched_state(vrt_ctx *c, hipStream_t s, int width, int n_rows, int row0, int row_stride, int tile_rows, int mode,
                        uint32_t n_tiles, uint32_t n_groups);
bool measuring_launch(uint64_t launches, int period);
int launch_order_kernel(vrt_ctx *c, SchedState *st, hipStream_t s);
constexpr long kSchedMinGroups = 768;    // an eighth of a 1080p frame (1,013 groups) still gains 4 %; below, the 9 us order kernel costs more
constexpr long kSchedMaxGroups = 36864;  // tile_order_kernel keeps one word per group in LDS (144 KiB of 160)
constexpr size_t kSchedMaxStates = 16;
constexpr int kSchedDenoise = 100;              // SchedState::mode of the display pass
constexpr int kSchedDenoiseHdr = kSchedDenoise + 1;   // ... and of its HDR form (vrt_denoise_hdr): states, counters and orders of its own
constexpr long kSchedMinDenoiseGroups = 256;    // two workgroups fit a CU: 1,024 tiles are two rounds
constexpr long kSchedMaxDenoiseGroups = 2048;   // beyond ~8,000 tiles (16 rounds) the tail is small and heaviest-first starts cost the halo reads their L2 locality: 4K nature 0.147 ms row-major, 0.157 ordered

// vrt_accum.cpp
// The launches of one AccumStep, for enqueue(): `a`, `vs`, `v`, `grid` and `two_pass` as it made them for a frame of `mode`, `lsel`
// the lens selection (as constructed when there is no lens). Points a.defer_rec, and pass 1's outputs, at the accumulation's buffers.
hipError_t launch_accum_step(vrt_ctx::Accum &ac, vrt::KArgs &a, vrt::ViewSet &vs, const Variant &v, int mode, int grid, bool two_pass,
                             const vrt::LensSel &lsel, const AccumStep &acc, hipStream_t s);
// does the next sample still belong to the samples in the sums? (what vrt_accum_add's restart rule compares)
bool accum_inputs_current(const vrt_ctx *c);
// the call-order checks of everything that reads the accumulation, in the name of `what`: begun, holds samples, and with need_hdr keeps HDR sums
int accum_state(vrt_ctx *c, const char *what, bool need_hdr);
// M3's plane of an accumulation that keeps moments (the caller has checked), enqueued on s into d_variance
int accum_variance_into(vrt_ctx *c, float *d_variance, hipStream_t s);
// ... and room for it in the accumulation's own scratch (Accum::d_mvar, 4 bytes per pixel)
int ensure_variance_plane(vrt_ctx *c);
// A read of the accumulation on stream s, ordered against the context's: the samples were added on the context's stream, and later adds must not
// overtake this read (nor, through `read`, the last call's use of the float mean). Nothing to do when s is the context's stream.
template <class BODY>
int accum_joined(vrt_ctx *c, hipStream_t s, const BODY &body) {
    vrt_ctx::Accum &ac = c->accum;
    if (s != c->stream) {
        VRT_HIP(c, hipEventRecord(ac.added, c->stream));
        VRT_HIP(c, hipStreamWaitEvent(s, ac.added, 0));
    }
    const int r = body();
    if (r) return r;
    if (s != c->stream) {
        VRT_HIP(c, hipEventRecord(ac.read, s));
        VRT_HIP(c, hipStreamWaitEvent(c->stream, ac.read, 0));
    }
    return VRT_OK;
}

// vrt_filter.cpp
// What vrt_filter_hdr_var checks of its filter, tone map and colour outputs (one of which must not be null), in the name of `what`,
// before anything is enqueued; and the call itself in that name: the chain of vrt_accum_resolve_hdr_temporal (vrt_temporal.cpp)
int filter_var_check(vrt_ctx *c, const char *what, const vrt_filter_var *f, const vrt_tonemap *tm, const void *out_rgb, const void *out_rgba8);
int filter_var_frame(vrt_ctx *c, const char *what, int width, int height, const void *d_rgb, const void *d_normal, const void *d_albedo,
                     const void *d_depth, const void *d_coverage, const void *d_variance, const vrt_filter_var *f, const vrt_tonemap *tm,
                     void *d_out_rgb, void *d_out_rgba8, void *d_out_variance, void *stream);

// vrt_guides.cpp
// vrt_guide_frame_device in the name of `what` with the guide-glass rule given (the entry points: the context's at the call; the
// upsampled resolve: the accumulation's as begun): the planes of one corner sample per pixel of a width x height frame from the
// context's current inputs, marched on the context's stream into the context's own state, resolved on s
int guide_frame_planes(vrt_ctx *c, const char *what, int width, int height, bool glass, float *d_normal, float *d_albedo, float *d_depth,
                       float *d_coverage, hipStream_t s);

// vrt_rays.cpp
// The kernel arguments of a caller's ray batch of n rays as an image of `width` (after ensure_analysis): the scene and light blocks
// as a frame carries them, and nothing derived from an eye -- no first lookup, ray table, miss mask or tightened root
void fill_ray_batch_args(const vrt_ctx *c, size_t n, int width, vrt::KArgs &a, vrt::ViewSet &vs);

// vrt_raygen.cpp
bool build_ray_table(const float *m, int W, int H, std::vector<float> &tab, float &z_out);
bool view_matrix_in_range(const float *m);
bool miss_table_fit(const float *tab, float z, int W, int H, vrt::miss::TableFit &f);
bool miss_view_params(const float *inv_view, const float gro[3], const vrt::miss::TableFit &f, vrt::miss::ViewParams &v);

}  // namespace vrt_internal
