// vrt_query.hip.h -- world queries against the tree the frames are rendered from (vrt.h vrt_cast_rays, vrt_find_voxels):
// the reference's CPU ray cast (src/octree.cpp:364-485, which the test oracle restates), the build
// click's neighbour cell (src/main.cpp:315-360) and octree_find (src/octree.cpp:102-130), one lane per ray or point.
//
// The lookup is the v4 traversal's find() (vrt_kernels_v4.hip.h), its walk state carried from one step of a ray to the
// next as march() carries it. find() reports the cube of the deepest node on the path -- a leaf, or the absent child the
// point falls in -- through its planes: with dpos = "direction > 0" per axis they are exactly the faces _octree_find_leaf's
// caller steps to (nmax where d > 0, else nmin), with dpos = 0 they are the cube's minimum corner. Wide cells are aligned
// cubes of side 2^t; above the wide roots (the reference's [-1023, 1024) world is not a power of two) the record walk uses
// the reference's own midpoints, lo + (hi - lo) / 2. find() runs with forward = false, so the root0_only shortcut (an
// answer the shader may take, the ray cast may not) never applies, and the query reads wide root 0 as uploaded: the
// tighter root of VRT_OPT_EMPTY_OCTANTS is a launch argument of the tracing kernels only.
//
// What the device tree cannot tell apart. Records and wide cells keep a leaf's words, not its voxel.coord. For every leaf
// octree_insert / octree_remove make that holds a real voxel, coord is the node's minimum corner: a unit leaf is its own
// cell; a merged volume gets coord = lbb (:258-285); the F1 "lazy point" split of such a volume (:227-249, taken when
// lbb.y or coord.y is 0) moves it into the octant that holds coord = lbb, child 0, whose lbb it is again. Leaves with
// record words 0/0 are empty space in both layouts, and the query reads them so. Most are the phantom leaves of F3
// (:174-179: the invalid voxel, coord.y = MIN_HEIGHT, never a hit). But a phantom whose node has lbb.x = lbb.z = 0 and
// lbb.y != 0 passes vmm's "equality" with its coord (0, MIN_HEIGHT, 0) when the node is split, so _split_node fills all
// 8 children as a volume with coord = their lbb -- and those "ghost" leaves, split and merged further as any volume, are
// hits for the reference's ray cast and octree_find (dragon.vox: 38 leaves, nature.vox: 682; alpha 0, so no frame shows
// them). Words 0/0 cannot tell a ghost from a phantom, nor from a voxel inserted with colour 0 and zero material: the
// queries answer as the reference does on the tree with every such leaf's has_voxel cleared (tests/test_gpu_queries.py
// holds them to exactly that, and checks that ghost hits are the only rays answered otherwise on the tree as built).
#pragma once
#include "vrt_kernels_v4.hip.h"
#include "vrt_query.h"

namespace vrt {
namespace query {

constexpr int kMinHeight = -1024;   // src/octree.cpp:12-14
constexpr int kMaxSteps = 512;      // src/octree.cpp:418

using T = v4::TravT<false>;

// (int)floorf(x) as the reference's x86-64 build executes it: cvttss2si gives INT_MIN for NaN and out-of-range values
// (the device's v_cvt_i32_f32 would saturate, and give 0 for NaN)
VRT_DEV int to_int_x86(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : (int)0x80000000u; }
VRT_DEV I3 floor_x86(F3 p) {
    return I3{to_int_x86(__builtin_floorf(p.x)), to_int_x86(__builtin_floorf(p.y)), to_int_x86(__builtin_floorf(p.z))};
}
// _coord_is_outside (src/octree.cpp:80-87) against the root's cube = the world bounds of vrt_params
VRT_DEV bool outside_root(const KArgs &a, I3 p) {
    return p.x < a.wmin[0] || p.x >= a.wmax[0] || p.y < a.wmin[1] || p.y >= a.wmax[1] || p.z < a.wmin[2] || p.z >= a.wmax[2];
}
// the record words of the cell find() returned (to_cell4() undone; the refraction byte reads 0 under alpha 0, as both
// layouts store it)
VRT_DEV void leaf_words(const v4::Found &f, uint32_t &w0, uint32_t &w1) {
    const uint32_t m = f.y & 0xffu;
    const bool refr0 = m == 85u && (((f.y >> 29) & 1u) != 0u || (f.x >> 24) == 0u);
    w0 = f.x;
    w1 = (refr0 ? 0u : m) | (f.y & 0x007fff00u) | (((f.y >> 28) & 1u) << 23);
}
// a corner of the cube find() reports for p (in the world) -- the minimum one for up = 0, the maximum (exclusive) one for
// up = 1 -- and the words of what it holds
VRT_DEV I3 node_corner(const KArgs &a, const T::Ctx &c, I3 p, v4::Walk &w, int up, uint32_t &w0, uint32_t &w1) {
    v4::Found f;
    (void)T::find(a, c, p, I3{up, up, up}, w, f, false);
    leaf_words(f, w0, w1);
    return I3{(int)f.plane.x, (int)f.plane.y, (int)f.plane.z};
}
VRT_DEV I3 node_min(const KArgs &a, const T::Ctx &c, I3 p, v4::Walk &w, uint32_t &w0, uint32_t &w1) {
    return node_corner(a, c, p, w, 0, w0, w1);
}

// Whether octree_find's descent reaches the node [nlo, nhi) that holds p. The tree is split at lo + (hi - lo) / 2
// (_create_children, :150), but octree_find picks the child of p at (lbb + rtf) / 2, vmm's truncating division (:111, 126):
// where lo + hi is odd and negative -- the planes -512, -768, -896, ... of the reference's [-1023, 1024) world -- a point
// in [lo + (hi - lo) / 2, (lo + hi) / 2) is sent to the low child, fails that child's outside test and is not found.
VRT_DEV bool find_reaches(const KArgs &a, I3 p, I3 nlo, I3 nhi) {
    int lo[3] = {a.wmin[0], a.wmin[1], a.wmin[2]}, hi[3] = {a.wmax[0], a.wmax[1], a.wmax[2]};
    const int pc[3] = {p.x, p.y, p.z};
    for (int level = 0; level < 32; ++level) {
        if (lo[0] == nlo.x && lo[1] == nlo.y && lo[2] == nlo.z && hi[0] == nhi.x && hi[1] == nhi.y && hi[2] == nhi.z) return true;
        bool inside = true;
        for (int k = 0; k < 3; ++k) {
            const int routed = (lo[k] + hi[k]) / 2;          // octree_find's midpoint (C division truncates)
            const int split = lo[k] + (hi[k] - lo[k]) / 2;   // the tree's
            if (pc[k] >= routed) lo[k] = split; else hi[k] = split;
            inside = inside && pc[k] >= lo[k] && pc[k] < hi[k];
        }
        if (!inside) return false;
    }
    return false;
}

// octree_ray_cast (src/octree.cpp:405-485) + get_placement_coord (src/main.cpp:315-360): one lane per ray, no LDS
__global__ void __launch_bounds__(64) cast_rays_kernel(KArgs a, RayArgs q) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= q.n) return;
    const float *op = q.origins + (size_t)q.origin_stride * i;
    const float *dp = q.dirs + (size_t)3 * i;
    const F3 ro{op[0], op[1], op[2]}, rd{dp[0], dp[1], dp[2]};
    F3 inv;
    inv.x = (__builtin_fabsf(rd.x) < 1e-8f) ? 1e20f : 1.0f / rd.x;
    inv.y = (__builtin_fabsf(rd.y) < 1e-8f) ? 1e20f : 1.0f / rd.y;
    inv.z = (__builtin_fabsf(rd.z) < 1e-8f) ? 1e20f : 1.0f / rd.z;
    const I3 dpos{rd.x > 0.0f ? 1 : 0, rd.y > 0.0f ? 1 : 0, rd.z > 0.0f ? 1 : 0};
    T::Ctx c;
    c.root = a.nodes[0];
    v4::Walk w;
    T::reset(w);
    v4::Found f;
    F3 rp = ro;
    I3 mp = floor_x86(rp);
    bool hit = false;
    int steps = 0;
    uint32_t w0 = 0u, w1 = 0u;
    I3 coord{-1, -1, -1};
    for (int it = 0; it < kMaxSteps; ++it) {
        steps = it + 1;
        F3 plane;
        if (it == 0 && outside_root(a, mp)) {
            // _octree_find_leaf returns NULL without writing the bounds: the caller's worldMin / worldMax stand
            plane = F3{dpos.x ? q.box_hi[0] : q.box_lo[0], dpos.y ? q.box_hi[1] : q.box_lo[1], dpos.z ? q.box_hi[2] : q.box_lo[2]};
        } else {
            if (T::find(a, c, mp, dpos, w, f, false) == v4::kOutside) T::reset(w);   // not reached: mp is in the world
            leaf_words(f, w0, w1);
            if ((w0 | w1) != 0u) {   // a leaf: the hit test is has_voxel && coord.y > MIN_HEIGHT (:434)
                uint32_t u0, u1;
                coord = node_min(a, c, mp, w, u0, u1);
                if (coord.y > kMinHeight) { hit = true; break; }
            }
            plane = f.plane;
        }
        const float tx = (plane.x - rp.x) * inv.x;
        const float ty = (plane.y - rp.y) * inv.y;
        const float tz = (plane.z - rp.z) * inv.z;
        const float m_yz = ty < tz ? ty : tz;
        float t = tx < m_yz ? tx : m_yz;
        const int axis = (tx < ty) ? ((tx < tz) ? 0 : 2) : ((ty < tz) ? 1 : 2);
        if (t < 0.0001f) t = 0.0001f;
        rp.x = rp.x + rd.x * t;
        rp.y = rp.y + rd.y * t;
        rp.z = rp.z + rd.z * t;
        F3 tp = rp;
        if (axis == 0) tp.x = tp.x + rd.x * 0.001f;
        else if (axis == 1) tp.y = tp.y + rd.y * 0.001f;
        else tp.z = tp.z + rd.z * 0.001f;
        mp = floor_x86(tp);
        if (outside_root(a, mp)) break;
    }
    RayHit h;
    h.steps = steps;
    h.hit = hit ? 1 : 0;
    h.leaf[0] = hit ? w0 : 0u;
    h.leaf[1] = hit ? w1 : 0u;
    I3 place{-1, -1, -1};
    if (hit) {
        place = coord;
        // get_placement_coord: the slab test against the unit box at coord, plain division (0 gives inf / NaN)
        const F3 bmin{(float)coord.x, (float)coord.y, (float)coord.z};
        const F3 bmax{bmin.x + 1.0f, bmin.y + 1.0f, bmin.z + 1.0f};
        float tminx = (bmin.x - ro.x) / rd.x, tmaxx = (bmax.x - ro.x) / rd.x;
        float tminy = (bmin.y - ro.y) / rd.y, tmaxy = (bmax.y - ro.y) / rd.y;
        float tminz = (bmin.z - ro.z) / rd.z, tmaxz = (bmax.z - ro.z) / rd.z;
        if (tminx > tmaxx) { const float s = tminx; tminx = tmaxx; tmaxx = s; }
        if (tminy > tmaxy) { const float s = tminy; tminy = tmaxy; tmaxy = s; }
        if (tminz > tmaxz) { const float s = tminz; tminz = tmaxz; tmaxz = s; }
        const float t_entry = __builtin_fmaxf(__builtin_fmaxf(tminx, tminy), tminz);   // fmax: a NaN operand loses
        if (__builtin_fabsf(t_entry - tminx) < 1e-4f) place.x += (rd.x > 0.0f) ? -1 : 1;
        else if (__builtin_fabsf(t_entry - tminy) < 1e-4f) place.y += (rd.y > 0.0f) ? -1 : 1;
        else place.z += (rd.z > 0.0f) ? -1 : 1;
    } else {
        coord = I3{-1, -1, -1};
    }
    h.coord[0] = coord.x; h.coord[1] = coord.y; h.coord[2] = coord.z;
    h.place[0] = place.x; h.place[1] = place.y; h.place[2] = place.z;
    q.out[i] = h;
}

// octree_find (src/octree.cpp:102-130) as isVoxelSolid (src/main.cpp:100-105) reads it: the voxel of the node on the path
// whose coord "equals" p by vmm's ivec3_equal_vec -- x and z equal, both y non-zero -- and coord.y > MIN_HEIGHT,
// provided octree_find's own routing reaches that node (find_reaches)
__global__ void __launch_bounds__(64) find_voxels_kernel(KArgs a, PointArgs q) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= q.n) return;
    const I3 p{q.coords[3 * (size_t)i], q.coords[3 * (size_t)i + 1], q.coords[3 * (size_t)i + 2]};
    uint32_t present = 0u, w0 = 0u, w1 = 0u;
    if (!outside_root(a, p)) {
        T::Ctx c;
        c.root = a.nodes[0];
        v4::Walk w;
        T::reset(w);
        const I3 lo = node_min(a, c, p, w, w0, w1);
        present = ((w0 | w1) != 0u && lo.x == p.x && lo.z == p.z && lo.y != 0 && p.y != 0 && lo.y > kMinHeight) ? 1u : 0u;
        if (present) {
            uint32_t u0, u1;
            const I3 hi = node_corner(a, c, p, w, 1, u0, u1);
            present = find_reaches(a, p, lo, hi) ? 1u : 0u;
        }
    }
    uint32_t *o = q.out + 3 * (size_t)i;
    o[0] = present;
    o[1] = present ? w0 : 0u;
    o[2] = present ? w1 : 0u;
}

}  // namespace query
}  // namespace vrt
