// vrt_dispatch.cpp -- the dispatch boundary (src/main.cpp:941-946): enqueue() makes one frame launch as a sequence of steps -- the
// views, the kernel variant the scene and the views allow, the frame block of the kernel arguments (the scene and light blocks are
// vrt_scene.cpp's), the feedback tile scheduler, the form of the full path tracer -- over the caches above it (scheduling states, ray
// tables, miss masks), and carries the vrt_dispatch* entry points of include/vrt.h. Host code; the kernels are behind vrt_launch.h.
#include "vrt_stage.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>

using namespace vrt_internal;
#include "vrt_launch.h"

namespace vrt_internal {

// The scheduling state for this launch shape on this stream (created on first use; the least recently used one is
// recycled when there are kSchedMaxStates). nullptr when device memory for it cannot be had: the launch then runs plain.
SchedState *sched_state(vrt_ctx *c, hipStream_t s, int width, int n_rows, int row0, int row_stride, int tile_rows, int mode,
                        uint32_t n_tiles, uint32_t n_groups) {
    uint64_t &tick = c->sched_tick;
    ++tick;
    for (SchedState &st : c->sched)
        if (st.stream == s && st.width == width && st.n_rows == n_rows && st.row0 == row0 && st.row_stride == row_stride &&
            st.tile_rows == tile_rows && st.mode == mode && st.n_tiles == n_tiles && st.n_groups == n_groups) {
            st.last_use = tick;
            return &st;
        }
    SchedState *slot = nullptr;
    if (c->sched.size() < kSchedMaxStates) {
        c->sched.emplace_back();
        slot = &c->sched.back();
    } else {
        for (SchedState &st : c->sched)
            if (!slot || st.last_use < slot->last_use) slot = &st;
        // the recycled buffers may still be read by launches in flight on the old stream
        if (hipDeviceSynchronize() != hipSuccess) return nullptr;
        *slot = SchedState{};   // frees them
    }
    // whole groups of ticks; the words past the last tile are never written and must read as zero
    const size_t cost_bytes = (size_t)n_groups * vrt::kGroupTiles * sizeof(uint32_t);
    if (slot->d_cost.reserve(cost_bytes) != hipSuccess ||
        slot->d_order.reserve(((size_t)n_groups + 1) * sizeof(uint32_t)) != hipSuccess ||   // + KArgs::split_count
        hipMemsetAsync(slot->d_cost, 0, cost_bytes, s) != hipSuccess) {
        *slot = SchedState{};  // an empty state matches no launch and is the first to be recycled
        (void)hipGetLastError();
        return nullptr;
    }
    slot->stream = s; slot->width = width; slot->n_rows = n_rows; slot->row0 = row0; slot->row_stride = row_stride;
    slot->tile_rows = tile_rows; slot->mode = mode; slot->n_tiles = n_tiles; slot->n_groups = n_groups;
    slot->last_use = tick;
    return slot;
}

// An order measured from one pose says little about a frame from a very different one: re-measure at once, instead of
// waiting out the period, when the eye has moved by more than 16 world units or the view has turned by more than ~8
// degrees since the order was taken (a cut, a teleport; ordinary camera motion stays far below both per period).
bool camera_jumped(const float was[6], const float now[6]) {
    float d2 = 0.0f, dot = 0.0f, n0 = 0.0f, n1 = 0.0f;
    for (int k = 0; k < 3; ++k) {
        d2 += (now[k] - was[k]) * (now[k] - was[k]);
        dot += now[3 + k] * was[3 + k];
        n0 += was[3 + k] * was[3 + k];
        n1 += now[3 + k] * now[3 + k];
    }
    if (!(d2 <= 16.0f * 16.0f)) return true;           // also true for NaN
    return !(dot * dot >= 0.98f * n0 * n1 && dot >= 0.0f);  // cos(8 deg)^2 = 0.98
}

// Which launches of a shape record tile times: the second one (warm), then every period-th; period 1 = all of them.
bool measuring_launch(uint64_t launches, int period) {
    return period == 1 || launches % (uint64_t)period == 1;
}

// After a measuring launch, on the same stream: reads that launch's ticks, rewrites the order the next launches read.
int launch_order_kernel(vrt_ctx *c, SchedState *st, hipStream_t s) {
    bool &raised = c->order_lds_raised;   // per context, i.e. per device: the attribute does not carry over to another one
    const bool raise = (size_t)st->n_groups * sizeof(uint32_t) > 48 * 1024 && !raised;
    // the general full path tracer is built for five waves per SIMD; the other states never read the split count
    const uint32_t wave_slots = st->mode == VRT_MODE_FULL ? (uint32_t)c->n_cus * 4u * 5u : 0u;
    VRT_HIP(c, vrt::launch::tile_order(st->d_cost, st->n_groups, st->d_order, wave_slots, raise, (size_t)kSchedMaxGroups * sizeof(uint32_t), s));
    if (raise) raised = true;
    st->valid = true;
    return VRT_OK;
}

// The view's table, from the cache or built and uploaded now (a synchronous 12 KB copy, once per projection and frame
// shape). nullptr: this projection has no table. Eight tables are kept; the least recently used one is replaced after a
// device synchronize (launches on any stream may still read it).
vrt_ctx::RayTable *ray_table(vrt_ctx *c, const float *inv_proj, int W, int H) {
    if (!c->ray_tables_on) return nullptr;
    vrt_ctx::RayTable *hit = nullptr, *lru = nullptr;
    for (auto &t : c->ray_tables) {
        if (t.width == W && t.height == H && std::memcmp(t.inv_proj, inv_proj, sizeof t.inv_proj) == 0) hit = &t;
        if (!lru || t.last_use < lru->last_use) lru = &t;
    }
    if (hit) {
        hit->last_use = ++c->ray_tick;
        return hit->ok ? hit : nullptr;
    }
    std::vector<float> tab;
    float z = 0.0f;
    const bool ok = build_ray_table(inv_proj, W, H, tab, z);
    vrt_ctx::RayTable *t;
    if (c->ray_tables.size() < 8) {
        c->ray_tables.emplace_back();
        t = &c->ray_tables.back();
    } else {
        t = lru;
        if (t->ok && hipDeviceSynchronize() != hipSuccess) return nullptr;
    }
    std::memcpy(t->inv_proj, inv_proj, sizeof t->inv_proj);
    t->width = W; t->height = H; t->z = z; t->ok = false;
    t->last_use = ++c->ray_tick;
    if (!ok) return nullptr;
    if (t->d_tab.reserve(tab.size() * sizeof(float)) != hipSuccess) return nullptr;
    if (hipMemcpy(t->d_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    t->fit_ok = miss_table_fit(tab.data(), z, W, H, t->fit);
    t->ok = true;
    return t;
}

// The occupancy boxes of the current tree and world bounds on the device (vrt_layout.h occupancy_boxes), made when a mask is about
// to be built (miss_mask(), second sight) and the list on the device is not for the current tree_gen (uploads, patches, batches and
// compaction all advance it) and bounds. Never on a dispatch that builds no mask: an application that edits before every frame
// never pays for it (a key that holds tree_gen is new after every edit). Host time: the walk of the record array, 0.9 ms for
// dragon.vox, 33 ms for the config-4 terrain (2.7 M records, 408 K boxes), plus the copy. False: no list (too many boxes, a world
// beyond the proof's bounds, a malformed tree, no device memory).
bool occupancy(vrt_ctx *c) {
    vrt_ctx::Occupancy &o = c->occ;
    const bool same = o.built && o.tree_gen == c->tree_gen && std::memcmp(o.wmin, c->params.world_min, sizeof o.wmin) == 0 &&
                      std::memcmp(o.wmax, c->params.world_max, sizeof o.wmax) == 0;
    if (same) return o.ok;
    o.built = true; o.ok = false;
    o.tree_gen = c->tree_gen;
    std::memcpy(o.wmin, c->params.world_min, sizeof o.wmin);
    std::memcpy(o.wmax, c->params.world_max, sizeof o.wmax);
    for (int k = 0; k < 3; ++k)   // the proof's bound on a march position (DESIGN §3 "Miss tiles"): a world inside [-2^11, 2^11]^3
        if (o.wmin[k] < -vrt::miss::kMaxWorld || o.wmax[k] > vrt::miss::kMaxWorld) return false;
    std::vector<int> boxes;
    if (!vrt::occupancy_boxes(c->host_records, o.wmin, o.wmax, (size_t)vrt::miss::kMaxBoxes, boxes)) return false;
    const size_t bytes = boxes.size() * sizeof(int);
    // launches in flight may read the old list (through the masks built from it: they read the masks only)
    if (hipDeviceSynchronize() != hipSuccess) return false;
    if (o.d_boxes.reserve(bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (bytes && hipMemcpy(o.d_boxes, boxes.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return false; }
    o.n_boxes = boxes.size() / 6;
    o.ok = true;
    return true;
}

// The miss mask of one view (vrt_miss.h), from the cache or built now on stream s by miss_mask_kernel over the occupancy boxes.
// The key is what the mask depends on: the projection and the frame shape (the ray tables), the view matrix, the eye in voxels,
// the tree generation and the world bounds. A mask is built the SECOND time its key is seen: a camera that moves every frame would pay a build per frame (5.2 us
// at 1080p on the dragon) for less than that back (profiles/miss_tiles_moving.txt: the frame right after a build gains little), a
// camera that holds still pays one build and gains every frame after (8.5 us). A build writes a
// new stamp into the tiles it marks (View::miss_stamp), so it needs no clearing pass. Eight keys are kept; the least recently used
// one is replaced -- its buffer rebuilt at once when only its own stream read it (stream order keeps the launches that did before
// the rebuild), after a device synchronize otherwise. Every build records an event on its stream right after the kernel; a launch on
// another stream waits for it (the build's stream, which may be a caller's, is never touched again). nullptr: no mask for this view
// (yet).
const uint8_t *miss_mask(vrt_ctx *c, const vrt::View &w, const vrt_ctx::RayTable &t, float voxel_scale, hipStream_t s, uint32_t &stamp) {
    // The box list costs a walk of the whole record array (~12 ns per record: 0.9 ms for dragon.vox, 33 ms for the config-4 terrain)
    // and a frame gains ~10 us: masks are made only once the tree and the bounds have stood unchanged for max(kStableMin, records /
    // kStablePerRecords) of these requests -- an application that edits every few frames never pays for a list it could not
    // amortise (tools/miss_tiles_edit.py), and the walk costs at most ~6 us per frame of the stable stretch before it.
    vrt_ctx::Occupancy &o = c->occ;
    if (o.seen_gen != c->tree_gen || std::memcmp(o.seen_wmin, c->params.world_min, sizeof o.seen_wmin) != 0 ||
        std::memcmp(o.seen_wmax, c->params.world_max, sizeof o.seen_wmax) != 0) {
        o.seen_gen = c->tree_gen;
        std::memcpy(o.seen_wmin, c->params.world_min, sizeof o.seen_wmin);
        std::memcpy(o.seen_wmax, c->params.world_max, sizeof o.seen_wmax);
        o.stable = 0;
    }
    const uint64_t need = std::max<uint64_t>(vrt::miss::kStableMin, c->host_records.size() / vrt::miss::kStablePerRecords);
    if (o.stable < need) { ++o.stable; return nullptr; }
    const float gro[3] = {w.cam_pos[0] * voxel_scale, w.cam_pos[1] * voxel_scale, w.cam_pos[2] * voxel_scale};   // the kernel's gro
    // an eye outside the world: the march's first step goes to the world face in the direction of travel, which lies BEHIND a ray
    // that leaves that face's half-space (t < 0), and rounding can land it inside -- the proof's t >= 0 does not hold: no mask
    if (!vrt::miss::eye_in_world(gro, c->params.world_min, c->params.world_max)) return nullptr;
    const int W = t.width, H = t.height;
    vrt_ctx::MissMask *hit = nullptr, *lru = nullptr;
    for (auto &m : c->miss_masks) {
        if (m.width == W && m.height == H && m.tree_gen == c->tree_gen && std::memcmp(m.wmin, c->params.world_min, sizeof m.wmin) == 0 &&
            std::memcmp(m.wmax, c->params.world_max, sizeof m.wmax) == 0 && std::memcmp(m.inv_proj, w.inv_proj, sizeof m.inv_proj) == 0 &&
            std::memcmp(m.inv_view, w.inv_view, sizeof m.inv_view) == 0 && std::memcmp(m.gro, gro, sizeof m.gro) == 0)
            hit = &m;
        if (!lru || m.last_use < lru->last_use) lru = &m;
    }
    if (hit && !hit->pending) {
        hit->last_use = ++c->miss_tick;
        if (!hit->ok) return nullptr;
        if (hit->stream != s) {
            if (hipStreamWaitEvent(s, hit->built, 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            hit->shared = true;
        }
        stamp = hit->stamp;
        return reinterpret_cast<const uint8_t *>(hit->d_mask.get());
    }
    if (!hit) {   // first sight: note the key, build nothing (the slot's buffer, which launches in flight may read, stays as it is)
        vrt_ctx::MissMask *m;
        if (c->miss_masks.size() < 8) {
            c->miss_masks.emplace_back();
            m = &c->miss_masks.back();
        } else {
            m = lru;
        }
        std::memcpy(m->inv_proj, w.inv_proj, sizeof m->inv_proj);
        std::memcpy(m->inv_view, w.inv_view, sizeof m->inv_view);
        std::memcpy(m->gro, gro, sizeof m->gro);
        m->width = W; m->height = H; m->tree_gen = c->tree_gen;
        std::memcpy(m->wmin, c->params.world_min, sizeof m->wmin);
        std::memcpy(m->wmax, c->params.world_max, sizeof m->wmax);
        m->ok = false;
        m->pending = true;
        m->last_use = ++c->miss_tick;
        return nullptr;
    }
    vrt_ctx::MissMask *m = hit;   // second sight: build
    m->pending = false;
    m->last_use = ++c->miss_tick;
    vrt::miss::ViewParams vp;
    if (!t.fit_ok || !miss_view_params(w.inv_view, gro, t.fit, vp)) return nullptr;
    if (!m->built && hipEventCreateWithFlags(&m->built, hipEventDisableTiming) != hipSuccess) { m->built = nullptr; (void)hipGetLastError(); return nullptr; }
    if (!occupancy(c)) return nullptr;
    if (m->d_mask && (m->shared || m->stream != s) && hipDeviceSynchronize() != hipSuccess) return nullptr;
    const size_t bytes = 8 + (size_t)vp.tiles_x * (size_t)vp.tiles_y;
    if (bytes > m->d_mask.bytes()) {
        if (m->d_mask && hipDeviceSynchronize() != hipSuccess) return nullptr;   // any stream may still read the old buffer
        if (m->d_mask.reserve(bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        m->stamp = 0;   // a new block: cleared below
    }
    if (m->stamp == 255u) m->stamp = 0u;   // wrapped: bytes of every stamp may be left, cleared below
    m->stamp = (uint8_t)(m->stamp + 1u);
    if (m->stamp == 1u && hipMemsetAsync(m->d_mask, 0, m->d_mask.bytes(), s) != hipSuccess) { (void)hipGetLastError(); return nullptr; }   // new or wrapped
    if (vrt::launch::miss_mask(vp, c->occ.d_boxes, (uint32_t)c->occ.n_boxes, m->d_mask, m->stamp, s) != hipSuccess ||
        hipEventRecord(m->built, s) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    m->stream = s;
    m->shared = false;
    m->ok = true;
    stamp = m->stamp;
    return reinterpret_cast<const uint8_t *>(m->d_mask.get());
}

namespace {

// ---- enqueue(), step by step: each function below is one decision of a frame launch, called in this order -------------------------

// Views: per view the camera block and the images, the eye's cell (-> eyes[i]), what the host looks up there for the kernels (the
// leaf that holds the eye, the wide kernels' first lookup) and the ray table of its projection (-> tables[i], nullptr: none).
void fill_views(vrt_ctx *c, const vrt_view *views, int n_views, void *d_rgba, void *d_id, int width, int height, vrt::ViewSet &vs,
                int eyes[][3], const vrt_ctx::RayTable *tables[]) {
    std::memset(&vs, 0, sizeof vs);
    for (int i = 0; i < n_views; ++i) {
        vrt::View &w = vs.v[i];
        std::memcpy(w.inv_proj, views ? views[i].inv_projection : c->inv_proj, sizeof w.inv_proj);
        std::memcpy(w.inv_view, views ? views[i].inv_view : c->inv_view, sizeof w.inv_view);
        std::memcpy(w.cam_pos, views ? views[i].camera_pos : c->cam_pos, sizeof w.cam_pos);
        w.out_rgba = (uint32_t *)(views ? views[i].d_rgba8 : d_rgba);
        w.out_id = (int2 *)(views ? views[i].d_id_dist : d_id);
        // the shader's lookup at the eye (comp:445-449), same arithmetic: floor(cameraPos * u_voxelScale)
        int *eye = eyes[i];
        for (int k = 0; k < 3; ++k) {
            const float g = floorf(w.cam_pos[k] * c->params.voxel_scale);
            // float -> int as the device converts: NaN -> 0, out of range saturates (and is outside any world)
            eye[k] = g != g ? 0 : (g >= 2147483648.0f ? 2147483647 : (g < -2147483648.0f ? (-2147483647 - 1) : (int)g));
        }
        vrt::eye_lookup(c->host_records, c->params.world_min, c->params.world_max, eye, w.eye0, w.eye1);
        vrt::FirstFind ff;
        w.first_valid = (c->wide_ok && vrt::first_find(c->wide, c->params.world_min, c->params.world_max, eye, vrt::v3::kAnchorShift, ff)) ? 1 : 0;
        if (w.first_valid) {
            w.first_w0 = ff.w0; w.first_w1 = ff.w1; w.first_node = ff.node; w.first_anode = ff.anode;
            w.first_s = ff.s; w.first_as = ff.as;
        }
        w.gen_x = w.gen_y = nullptr; w.gen_z = 0.0f; w.gen_fast = 0u;
        w.miss = nullptr;
        w.miss_stamp = 0u;
        tables[i] = nullptr;
        if (view_matrix_in_range(w.inv_view)) {
            if (const vrt_ctx::RayTable *t = ray_table(c, w.inv_proj, width, height)) {
                w.gen_x = t->d_tab; w.gen_y = t->d_tab + width; w.gen_z = t->z; w.gen_fast = 1u;
                tables[i] = t;
            }
        }
    }
}

// A thin lens (vrt_set_lens; accumulations only): every sample has an origin of its own, anywhere in a box of cells around the
// eye. What fill_views() made at the eye is kept only where it holds at every origin of that box (vrt_layout.h lens_select()):
// otherwise the lens kernels look the medium up per lane and the wide kernels make their own first lookup. False: no lens.
bool select_lens(const vrt_ctx *c, const AccumStep *acc, vrt::ViewSet &vs, vrt::LensSel &lsel) {
    if (!acc || !(acc->aperture > 0.0f)) return false;
    vrt::lens_select(c->host_records, c->wide_ok ? &c->wide : nullptr, c->params.world_min, c->params.world_max, c->params.voxel_scale,
                     vs.v[0].cam_pos, vs.v[0].inv_view, acc->aperture, lsel);
    if (!lsel.first_shared) vs.v[0].first_valid = 0;
    return true;
}

// The variant of this launch: the scene's (base_variant()) in the shape the mode asks for, v3 for eyes the v4 kernels do not take
Variant launch_variant(const vrt_ctx *c, int mode, bool accumulating, const vrt::ViewSet &vs, int n_views, bool lens, const vrt::LensSel &lsel) {
    Variant v = base_variant(c);
    if (mode == VRT_MODE_FULL) {
        // the full path tracer takes the wide traversals at five waves per SIMD (96 VGPRs and no extra spills measured 8-10 %
        // faster than the unconstrained 105-VGPR build); the default takes v4 here too (one march loop, for rays that start in
        // any medium: 96 registers without spills; 9 % faster than v3, profiles/r02_f_full_shader_v4_ab.jsonl), variant 20 v3
        if (v.trav >= 3) v.wpe = 5;
    } else if (!accumulating && mode == VRT_MODE_PRIMARY_SHADOW && c->variant == 20 && v.trav == 3) {
        // round 1's default: the shadow march was 1.5 % faster seven waves deep, the primary one six deep (the accumulation's
        // primary kernels, vrt_launch_accum.hip, exist in the table's shapes only)
        v.wpe = 7;
    }
    if (v.trav == 4 && mode != VRT_MODE_FULL) {
        // the v4 primary kernels hold the march loop for rays that start in refraction byte 85 (1.0) only: an eye inside a
        // medium (comp:445-449: refraction byte 1..254 of the voxel that holds it) takes the v3 kernels
        bool eye_in_medium = false;
        for (int i = 0; i < n_views; ++i) {
            const uint32_t b = vs.v[i].eye1 & 0xffu;
            eye_in_medium = eye_in_medium || (b >= 1u && b <= 254u && b != 85u);
        }
        if (lens) eye_in_medium = !lsel.no_medium;   // ... any origin of the lens inside one
        if (eye_in_medium) { v.trav = 3; v.wpe = 6; }
    }
    return v;
}

// The frame block of KArgs: the rows of this launch, the prologue's index arithmetic for its `tiles` tiles, and what a frame from
// these eyes may assume of the world outside wide root 0 (after fill_scene_args(): it may replace root 0 by a deeper node).
void fill_frame_args(const vrt_ctx *c, vrt::KArgs &a, int width, int height, int row0, int n_rows, int tile_rows, int row_stride, int compact,
                     long tiles, const int eyes[][3], int n_views, bool lens, const vrt::LensSel &lsel) {
    a.n_views = n_views; a.width = width; a.height = height;
    a.row0 = row0; a.n_rows = n_rows; a.tile_rows = tile_rows; a.row_stride = row_stride; a.compact = compact;
    // index arithmetic of the prologue without integer divisions where the shapes allow it
    const unsigned long tiles_x = (unsigned long)((width + 7) / 8);
    // q = (n * M) >> 32 with M = floor(2^32 / d) + 1 equals n / d while n * d < 2^32 (the error term n * (M * d - 2^32) stays below 2^32)
    a.tiles_x_magic = (tiles_x > 1 && (unsigned long)(tiles + 4) * tiles_x < (1ul << 32)) ? (uint32_t)((1ul << 32) / tiles_x + 1) : 0u;
    a.row_mode = tile_rows >= n_rows ? 1 : (tile_rows == 8 ? 2 : 0);
    // nothing outside wide root 0? (the shipped maps: the octree root's only child is the octant [0, 1024)^3) -- then rays
    // that leave it are done (find() in vrt_kernels_v4.hip.h), and the same argument one level down, as often as it holds,
    // lets a deeper node stand in for it: a shorter descent whenever a lookup restarts there, leaving rays done sooner.
    // dragon.vox: [0, 1024)^3 holds everything in its cell [0, 256)^3, whose 64-unit cells the model spreads over: root 0
    // becomes [0, 256)^3 for eyes inside it. Not below the anchor level (a node of side 2^kAnchorShift).
    a.root0_only = (a.n_roots == 1u && c->root0_only_on && vrt::content_only_in_root0(c->host_records, c->wide)) ? 1 : 0;
    if (a.root0_only && c->tight_root_on && !lens)
        vrt::tighten_root0(c->wide, eyes, n_views, vrt::v3::kAnchorShift, a.root0_node, a.root0_shift, a.root0_min);
    if (a.root0_only && c->tight_root_on && lens && lsel.box_valid) {   // a lens: every origin is an eye
        const int corners[2][3] = {{lsel.lo[0], lsel.lo[1], lsel.lo[2]}, {lsel.hi[0], lsel.hi[1], lsel.hi[2]}};
        vrt::tighten_root0(c->wide, corners, 2, vrt::v3::kAnchorShift, a.root0_node, a.root0_shift, a.root0_min);
    }
    a.group_order = nullptr; a.tile_cost = nullptr; a.split_count = nullptr;   // schedule() and the launch's form set these
    a.defer_rec = nullptr; a.defer_count = nullptr; a.defer_cap = 0;
}

// Feedback scheduling: wide-traversal kernels, one view, launches large enough to have a tail worth shaping. Sets a.group_order /
// a.tile_cost (the caller's buffers under vrt_set_tile_order) and returns the grid: the tiles' workgroups, or whole groups under an order.
// st: the state of this launch shape, when the scheduler runs it; measure: this launch records its tile times.
long schedule(vrt_ctx *c, hipStream_t s, const Variant &v, bool accumulating, int mode, long tiles, const vrt::ViewSet &vs, vrt::KArgs &a,
              SchedState *&st, bool &measure) {
    const int waves = v.block() / 64;
    long grid = (tiles + waves - 1) / waves;
    if (grid < 1) grid = 1;
    const bool sched_kernel = !accumulating && v.trav >= 3 && a.n_views == 1;
    const long groups = (tiles + vrt::kGroupTiles - 1) / vrt::kGroupTiles;
    if (sched_kernel && c->dbg_sched) {
        a.group_order = c->dbg_group_order;
        a.tile_cost = c->dbg_tile_cost;
    } else if (sched_kernel && c->sched_period > 0 && groups >= kSchedMinGroups && groups <= kSchedMaxGroups) {
        st = sched_state(c, s, a.width, a.n_rows, a.row0, a.row_stride, a.tile_rows, mode, (uint32_t)tiles, (uint32_t)groups);
        if (st) {
            // eye = invView's translation column, viewing direction = minus its third column (column-major)
            const float *iv = vs.v[0].inv_view;
            const float now[6] = {iv[12], iv[13], iv[14], -iv[8], -iv[9], -iv[10]};
            // the first launch of a shape is never the one measured: it may be the process's first launch of the kernel
            // (code object load, cold instruction cache and TLB), and its tile times would shape the next period's order
            measure = measuring_launch(st->launches, c->sched_period) || (st->valid && camera_jumped(st->cam, now));
            if (measure) std::memcpy(st->cam, now, sizeof now);
            a.group_order = st->valid ? st->d_order : nullptr;
            a.tile_cost = measure ? st->d_cost : nullptr;
        }
    }
    if (a.group_order) grid = groups * (vrt::kGroupTiles / waves);  // whole groups: the last one may hold tiles past the end
    return grid;
}

// Does the tree hold no translucent leaf (vrt::tree_is_opaque), derived once per tree
bool scene_opaque(vrt_ctx *c) {
    if (!c->scene_opaque_valid) { c->scene_opaque = vrt::tree_is_opaque(c->host_records); c->scene_opaque_valid = true; }
    return c->scene_opaque;
}

// The full path tracer as two tile-coherent passes, where the scene and the view allow it
bool opaque_two_pass(vrt_ctx *c, int mode, const Variant &v, const vrt::ViewSet &vs, int n_views, bool lens, const vrt::LensSel &lsel) {
    if (!(mode == VRT_MODE_FULL && c->two_pass_on && v.trav == 4 && n_views == 1 && c->variant == 0 && vs.v[0].out_rgba)) return false;
    (void)scene_opaque(c);
    if (lens) return c->scene_opaque && lsel.empty;   // every origin of the lens in empty space
    const uint32_t eye_alpha = vs.v[0].eye0 >> 24, eye_b = vs.v[0].eye1 & 0xffu;
    return c->scene_opaque && eye_alpha == 0u && (eye_b == 0u || eye_b == 85u || eye_b == 255u);
}

// The seed buffer of stream s (one per stream: launches on different streams may overlap; eight are kept, the least recently
// used one changes streams once its own has drained), grown to `need` tiles -> a.defer_rec
int stream_seeds(vrt_ctx *c, hipStream_t s, size_t need, vrt::KArgs &a) {
    vrt_ctx::SeedBuffer *sb = nullptr;
    for (auto &b : c->seeds)
        if (b.stream == s) sb = &b;
    if (!sb) {
        if (c->seeds.size() < 8) {
            c->seeds.emplace_back();
            sb = &c->seeds.back();
        } else {
            for (auto &b : c->seeds)
                if (!sb || b.last_use < sb->last_use) sb = &b;
            VRT_HIP(c, hipStreamSynchronize(sb->stream));   // its launches may still be in flight there
        }
        sb->stream = s;
    }
    if (need > sb->tiles) {
        VRT_HIP(c, hipStreamSynchronize(s));
        VRT_HIP(c, sb->d.reserve(need * vrt::kSeedPlanesHost * 64 * sizeof(uint32_t)));
        sb->tiles = need;
    }
    sb->last_use = ++c->seed_tick;
    a.defer_rec = reinterpret_cast<float *>(sb->d.get());
    return VRT_OK;
}

}  // namespace

// views == nullptr: one view, the context's camera (vrt_set_camera) rendering into d_rgba / d_id.
int enqueue(vrt_ctx *c, int width, int height, int row0, int n_rows, int tile_rows, int row_stride, int compact,
            int mode, void *d_rgba, void *d_id, hipStream_t s, const vrt_view *views, int n_views, const AccumStep *acc) {
    if (!c->have_scene) return vrt_fail(c, VRT_E_STATE, "vrt_dispatch: no octree uploaded (call vrt_upload_octree first)");
    if (c->batch.open) return vrt_fail(c, VRT_E_STATE, "vrt_dispatch: a patch batch is open (call vrt_patch_end first)");
    if (!views && !c->have_camera) return vrt_fail(c, VRT_E_STATE, "vrt_dispatch: no camera set (call vrt_set_camera first)");
    if (n_views < 1 || n_views > vrt::kMaxViews) return vrt_fail(c, VRT_E_INVALID, "vrt_dispatch_views: 1 to 4 views per launch");
    if (mode != VRT_MODE_PRIMARY && mode != VRT_MODE_PRIMARY_SHADOW && mode != VRT_MODE_FULL)
        return vrt_fail(c, VRT_E_INVALID, "unknown mode");
    if (n_rows <= 0) return VRT_OK;
    const int ra = ensure_analysis(c);
    if (ra) return ra;
    vrt::KArgs a;
    vrt::ViewSet vs;
    int eyes[vrt::kMaxViews][3];
    const vrt_ctx::RayTable *tables[vrt::kMaxViews] = {};
    fill_views(c, views, n_views, d_rgba, d_id, width, height, vs, eyes, tables);
    vrt::LensSel lsel;
    const bool lens = select_lens(c, acc, vs, lsel);
    const Variant v = launch_variant(c, mode, acc != nullptr, vs, n_views, lens, lsel);
    // miss tiles: the EYE85 primary kernels (v4, seven waves per SIMD) read a mask for every view with ray tables
    if (c->miss_tiles_on && !acc && v.trav == 4 && v.wpe == 7 && mode != VRT_MODE_FULL)
        for (int i = 0; i < n_views; ++i)
            if (tables[i]) vs.v[i].miss = miss_mask(c, vs.v[i], *tables[i], c->params.voxel_scale, s, vs.v[i].miss_stamp);
    const long tiles = (long)((width + 7) / 8) * (long)((n_rows + 7) / 8);   // 8 x 8 pixel tiles, one per wave
    fill_scene_args(c, a);
    fill_light_args(c, a);
    fill_frame_args(c, a, width, height, row0, n_rows, tile_rows, row_stride, compact, tiles, eyes, n_views, lens, lsel);
    SchedState *st = nullptr;
    bool measure = false;
    long grid = schedule(c, s, v, acc != nullptr, mode, tiles, vs, a, st, measure);
    const ProfSlot prof = acc ? ProfSlot{} : ProfSlot::take(c);
    const bool two_pass = !(acc && acc->paths.emit()) && opaque_two_pass(c, mode, v, vs, n_views, lens, lsel);   // emitter sampling: the general path tracer
    // the general full path tracer starts the heaviest groups of an ordered launch, measuring or not, as part-tile waves (KArgs::split_count)
    if (mode == VRT_MODE_FULL && !two_pass && st && a.group_order && c->heavy_split_on) {
        a.split_count = st->d_order + st->n_groups;
        grid += (long)vrt::kSplitMaxGroups * vrt::kGroupTiles * (vrt::kSplitParts - 1);
        // a measuring launch: the part-tile waves of a tile meet in its ticks with atomicMax
        if (a.tile_cost) VRT_HIP(c, hipMemsetAsync(st->d_cost, 0, (size_t)st->n_groups * vrt::kGroupTiles * sizeof(uint32_t), s));
    }
    hipError_t e;
    if (acc) {   // progressive accumulation (vrt_accum.cpp): the frame's samples go into the context's sums
        if (mode == VRT_MODE_FULL) a.path_depth = (uint32_t)c->accum.path_depth;   // frames keep fill_scene_args()'s 1: the shader
        AccumStep step = *acc;
        // guides past glass: a tree without a translucent leaf whose rays all start in empty space (trav 4) has every first hit
        // opaque, so the chain ends on it and the plain kernels give the same planes
        if (step.guides && step.glass && v.trav == 4 && scene_opaque(c)) step.glass = false;
        e = launch_accum_step(c->accum, a, vs, v, mode, (int)grid, two_pass, lsel, step, s);
    } else if (two_pass && c->two_pass_form >= 5) {
        e = vrt::launch::trace_full_opaque(a, vs, (int)grid, c->two_pass_form, s, prof.ev0, prof.ev1);
    } else if (two_pass) {
        const int rs = stream_seeds(c, s, (size_t)(a.group_order ? (tiles + vrt::kGroupTiles - 1) / vrt::kGroupTiles * vrt::kGroupTiles : tiles), a);   // whole groups
        if (rs) return rs;
        e = vrt::launch::trace_full_two_pass(a, vs, (int)grid, s, prof.ev0, prof.ev1);
    } else {
        e = vrt::launch::trace(mode, v, a, vs, (int)grid, s, prof.ev0, prof.ev1);
    }
    if (e != hipSuccess) return vrt_fail(c, VRT_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    if (st) {
        ++st->launches;
        if (measure) {
            const int rr = launch_order_kernel(c, st, s);
            if (rr) return rr;
        }
    }
    prof.commit(c);
    return VRT_OK;
}

}  // namespace vrt_internal

extern "C" {

int vrt_dispatch_rows(vrt_ctx *c, int width, int height, int row_begin, int row_end, int mode, void *d_rgba8,
                      void *d_id_dist, void *stream) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (row_begin < 0 || row_end > height || row_begin > row_end) return vrt_fail(c, VRT_E_INVALID, "vrt_dispatch_rows: bad row range");
    VRT_HIP(c, hipSetDevice(c->device));
    const int n = row_end - row_begin;
    return enqueue(c, width, height, row_begin, n, n > 0 ? n : 1, 0, 0, mode, d_rgba8, d_id_dist,
                   stream ? (hipStream_t)stream : c->stream);
}

int vrt_shard_rows(int height, int tile_rows, int shard, int n_shards) {
    if (height < 1 || tile_rows < 1 || n_shards < 1 || shard < 0 || shard >= n_shards) return VRT_E_INVALID;
    const int tiles = (height + tile_rows - 1) / tile_rows;
    int rows = 0;
    for (int t = shard; t < tiles; t += n_shards) {
        const int r0 = t * tile_rows;
        rows += (r0 + tile_rows <= height) ? tile_rows : height - r0;
    }
    return rows;
}

int vrt_dispatch_shard(vrt_ctx *c, int width, int height, int tile_rows, int shard, int n_shards, int mode,
                       void *d_rgba8, void *d_id_dist, void *stream) {
    int r = check_frame(c, width, height);
    if (r) return r;
    const int rows = vrt_shard_rows(height, tile_rows, shard, n_shards);
    if (rows < 0) return vrt_fail(c, VRT_E_INVALID, "vrt_dispatch_shard: bad tile_rows/shard/n_shards");
    VRT_HIP(c, hipSetDevice(c->device));
    return enqueue(c, width, height, shard * tile_rows, rows, tile_rows, tile_rows * n_shards, 1, mode, d_rgba8,
                   d_id_dist, stream ? (hipStream_t)stream : c->stream);
}

int vrt_dispatch_tiles(vrt_ctx *c, int width, int height, int tile_rows, int shard, int n_shards, int mode, void *d_frame_rgba8,
                       void *d_frame_id_dist, void *stream) {
    int r = check_frame(c, width, height);
    if (r) return r;
    const int rows = vrt_shard_rows(height, tile_rows, shard, n_shards);
    if (rows < 0) return vrt_fail(c, VRT_E_INVALID, "vrt_dispatch_tiles: bad tile_rows/shard/n_shards");
    VRT_HIP(c, hipSetDevice(c->device));
    // the shard's tiles at their frame rows (compact = 0): the frame may be local, a peer's, or an IPC mapping
    return enqueue(c, width, height, shard * tile_rows, rows, tile_rows, tile_rows * n_shards, 0, mode, d_frame_rgba8, d_frame_id_dist,
                   stream ? (hipStream_t)stream : c->stream);
}

int vrt_dispatch_views(vrt_ctx *c, int width, int height, int tile_rows, int shard, int n_shards, int mode,
                       const vrt_view *views, int n_views, void *stream) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (!views) return vrt_fail(c, VRT_E_INVALID, "vrt_dispatch_views: null views");
    const int rows = vrt_shard_rows(height, tile_rows, shard, n_shards);
    if (rows < 0) return vrt_fail(c, VRT_E_INVALID, "vrt_dispatch_views: bad tile_rows/shard/n_shards");
    VRT_HIP(c, hipSetDevice(c->device));
    return enqueue(c, width, height, shard * tile_rows, rows, tile_rows, tile_rows * n_shards, 1, mode, nullptr, nullptr,
                   stream ? (hipStream_t)stream : c->stream, views, n_views);
}

int vrt_dispatch(vrt_ctx *c, int width, int height, int mode, uint8_t *out_rgba8, int32_t *out_id_dist) {
    int r = check_frame(c, width, height);
    if (r) return r;
    VRT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * (size_t)height;
    r = ensure_scratch(c, px);
    if (r) return r;
    vrt_stage::Stage st(4);
    const int rgba = st.out(px * 4, out_rgba8, c->d_rgba), id = st.out(px * 8, out_id_dist, c->d_id);
    r = enqueue(c, width, height, 0, height, height, 0, 0, mode, st.at(rgba), st.at(id), c->stream);
    return r ? r : st.download(c, c->stream);
}

int vrt_dispatch_wait(vrt_ctx *c, int ticket) {
    if (!c || ticket < 0 || ticket > 1) return c ? vrt_fail(c, VRT_E_INVALID, "vrt_dispatch_wait: ticket") : VRT_E_INVALID;
    vrt_ctx::AsyncLane &ln = c->lane[ticket];
    if (!ln.busy) return VRT_OK;
    VRT_HIP(c, hipSetDevice(c->device));
    VRT_HIP(c, hipEventSynchronize(ln.done));
    ln.busy = false;
    return VRT_OK;
}

int vrt_dispatch_async(vrt_ctx *c, int width, int height, int mode, uint8_t *out_rgba8, int32_t *out_id_dist, int *ticket) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (!ticket) return vrt_fail(c, VRT_E_INVALID, "vrt_dispatch_async: null ticket");
    VRT_HIP(c, hipSetDevice(c->device));
    const int k = c->next_lane;
    vrt_ctx::AsyncLane &ln = c->lane[k];
    r = vrt_dispatch_wait(c, k);   // at most two frames in flight
    if (r) return r;
    const size_t px = (size_t)width * (size_t)height;
    if (!ln.stream) {
        VRT_HIP(c, hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
        VRT_HIP(c, hipEventCreateWithFlags(&ln.done, hipEventDisableTiming));
    }
    if (px > ln.pixels) {   // nothing to wait for: vrt_dispatch_wait above has seen the lane's last copies land
        VRT_HIP(c, ln.d_rgba.reserve(px * 4));
        VRT_HIP(c, ln.d_id.reserve(px * 8));
        ln.pixels = px;
    }
    r = enqueue(c, width, height, 0, height, height, 0, 0, mode, out_rgba8 ? ln.d_rgba : nullptr, out_id_dist ? ln.d_id : nullptr, ln.stream);
    if (r) return r;
    if (out_rgba8) VRT_HIP(c, hipMemcpyAsync(out_rgba8, ln.d_rgba, px * 4, hipMemcpyDeviceToHost, ln.stream));
    if (out_id_dist) VRT_HIP(c, hipMemcpyAsync(out_id_dist, ln.d_id, px * 8, hipMemcpyDeviceToHost, ln.stream));
    VRT_HIP(c, hipEventRecord(ln.done, ln.stream));
    ln.busy = true;
    *ticket = k;
    c->next_lane = k ^ 1;
    return VRT_OK;
}

int vrt_host_alloc(vrt_ctx *c, size_t bytes, void **host_ptr) {
    if (!c || !host_ptr || bytes == 0) return VRT_E_INVALID;
    *host_ptr = nullptr;
    VRT_HIP(c, hipSetDevice(c->device));
    VRT_HIP(c, hipHostMalloc(host_ptr, bytes, hipHostMallocDefault));
    return VRT_OK;
}

int vrt_host_free(vrt_ctx *c, void *host_ptr) {
    if (!c) return VRT_E_INVALID;
    if (host_ptr) VRT_HIP(c, hipHostFree(host_ptr));
    return VRT_OK;
}

int vrt_dispatch_timed(vrt_ctx *c, int width, int height, int row_begin, int row_end, int mode, void *d_rgba8,
                       void *d_id_dist, void *stream, int iters, float *ms_out) {
    int r = check_frame(c, width, height);
    if (r) return r;
    if (iters < 1 || !ms_out) return vrt_fail(c, VRT_E_INVALID, "vrt_dispatch_timed: iters/ms_out");
    if (row_begin < 0 || row_end > height || row_begin >= row_end) return vrt_fail(c, VRT_E_INVALID, "vrt_dispatch_timed: bad row range");
    VRT_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    std::vector<hipEvent_t> ev((size_t)iters * 2, nullptr);
    int rc = VRT_OK;
    hipError_t he = hipSuccess;
    for (auto &e : ev)
        if (he == hipSuccess) he = hipEventCreate(&e);
    const int n = row_end - row_begin;
    for (int i = 0; i < iters && rc == VRT_OK && he == hipSuccess; ++i) {
        he = hipEventRecord(ev[2 * i], s);
        if (he == hipSuccess) rc = enqueue(c, width, height, row_begin, n, n, 0, 0, mode, d_rgba8, d_id_dist, s);
        if (he == hipSuccess && rc == VRT_OK) he = hipEventRecord(ev[2 * i + 1], s);
    }
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    for (int i = 0; i < iters && rc == VRT_OK && he == hipSuccess; ++i) he = hipEventElapsedTime(&ms_out[i], ev[2 * i], ev[2 * i + 1]);
    for (auto &e : ev)
        if (e) (void)hipEventDestroy(e);   // on every path
    if (rc == VRT_OK && he != hipSuccess) rc = vrt_fail(c, VRT_E_HIP, std::string("vrt_dispatch_timed: ") + hipGetErrorString(he));
    return rc;
}

int vrt_set_profiling(vrt_ctx *c, int max_launches) {
    if (!c) return VRT_E_INVALID;
    VRT_HIP(c, hipSetDevice(c->device));
    c->prof_count = 0;
    c->prof_seen = 0;
    c->profiling = max_launches > 0;
    c->prof_cap = 0;
    while (c->profiling && c->prof_events.size() < (size_t)max_launches * 2) {
        hipEvent_t e;
        VRT_HIP(c, hipEventCreate(&e));
        c->prof_events.push_back(e);
    }
    if (c->profiling) c->prof_cap = (size_t)max_launches;   // not events.size() / 2: an earlier call may have asked for more
    return VRT_OK;
}

int vrt_set_profiling_stride(vrt_ctx *c, int every) {
    if (!c || every < 1) return VRT_E_INVALID;
    c->prof_stride = (size_t)every;
    return VRT_OK;
}

int vrt_profile_read(vrt_ctx *c, float *ms_out, int cap) {
    if (!c || !ms_out || cap < 0) return VRT_E_INVALID;
    VRT_HIP(c, hipSetDevice(c->device));
    int n = 0;
    for (size_t i = 0; i < c->prof_count && n < cap; ++i, ++n) {
        VRT_HIP(c, hipEventSynchronize(c->prof_events[2 * i + 1]));
        VRT_HIP(c, hipEventElapsedTime(&ms_out[n], c->prof_events[2 * i], c->prof_events[2 * i + 1]));
    }
    c->prof_count = 0;
    return n;
}

int vrt_set_tile_scheduling(vrt_ctx *c, int period) {
    if (!c) return VRT_E_INVALID;
    if (period < 0) return vrt_fail(c, VRT_E_INVALID, "vrt_set_tile_scheduling: period must be >= 0");
    c->sched_period = period;
    return VRT_OK;
}


// ---- documented switches (include/vrt.h): pixels never depend on them ----------------------------------------------------------
int vrt_set_option(vrt_ctx *c, int option, int value) {
    if (!c) return VRT_E_INVALID;
    switch (option) {
        case VRT_OPT_RAY_TABLES:
            if (value != 0 && value != 1) break;
            c->ray_tables_on = value != 0;
            return VRT_OK;
        case VRT_OPT_EMPTY_OCTANTS:
            if (value < 0 || value > 2) break;
            c->root0_only_on = value != 0;
            c->tight_root_on = value == 1;   // 2: the shortcut with wide root 0 as build_wide() found it
            return VRT_OK;
        case VRT_OPT_FULL_OPAQUE:
            if (value != 0 && value != 1 && (value < 5 || value > 7)) break;
            c->two_pass_on = value != 0;
            c->two_pass_form = value;   // 1: two kernels and a seed buffer; 5, 6, 7: both stages in one kernel at that many waves per SIMD
            return VRT_OK;
        case VRT_OPT_HEAVY_TILES:
            if (value != 0 && value != 1) break;
            c->heavy_split_on = value != 0;
            return VRT_OK;
        case VRT_OPT_MISS_TILES:
            if (value != 0 && value != 1) break;
            c->miss_tiles_on = value != 0;
            return VRT_OK;
        case VRT_OPT_DISPLAY_KERNEL:
            if (value != 0 && value != 2 && value != 3) break;
            c->denoise_variant = value;
            return VRT_OK;
        default:
            return vrt_fail(c, VRT_E_INVALID, "vrt_set_option: unknown option");
    }
    return vrt_fail(c, VRT_E_INVALID, "vrt_set_option: value out of range");
}

int vrt_set_tile_order(vrt_ctx *c, int enable, const void *d_group_order, void *d_tile_cost) {
    if (!c) return VRT_E_INVALID;
    c->dbg_sched = enable != 0;
    c->dbg_group_order = enable ? (const uint32_t *)d_group_order : nullptr;
    c->dbg_tile_cost = enable ? (uint32_t *)d_tile_cost : nullptr;
    return VRT_OK;
}

long vrt_get_tile_order(vrt_ctx *c, void *stream, uint32_t *out, size_t cap) {
    if (!c) return VRT_E_INVALID;
    const SchedState *best = nullptr;
    for (const SchedState &st : c->sched)
        if (st.stream == (stream ? (hipStream_t)stream : c->stream) && (!best || st.last_use > best->last_use)) best = &st;
    if (!best || !best->valid) return 0;
    VRT_HIP(c, hipSetDevice(c->device));
    VRT_HIP(c, hipStreamSynchronize(best->stream));
    const size_t n = (size_t)best->n_groups + 1 < cap ? (size_t)best->n_groups + 1 : cap;   // the order, then the split count (KArgs::split_count)
    if (out && n) VRT_HIP(c, hipMemcpy(out, best->d_order, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return (long)best->n_groups;
}

}  // extern "C"
