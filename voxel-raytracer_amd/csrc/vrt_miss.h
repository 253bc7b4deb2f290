// vrt_miss.h -- miss tiles of the primary trace (include/vrt.h VRT_OPT_MISS_TILES, DESIGN §3 "Miss tiles"): which 8 x 8 frame tiles
// may hold only rays that provably hit nothing. Shared by the host (the test-support library, tests/test_miss_tiles.py) and
// the device (miss_mask_kernel, vrt_launch_misc.hip): no HIP runtime, no kernel headers.
//
// The proof, in short (DESIGN §3 "Miss tiles" has it in full): a primary ray of the EYE85 kernel from an eye inside the world, whose
// direction has no component in (-1e-8, 0], computes every march position within delta < 0.25 voxel of its half-line gro + s * dir, s >= 0, in every axis,
// and a lookup returns the cell that holds floor() of such a position. The occupancy boxes cover every cell that can stop the
// ray (medium byte other than 85); a half-line that misses every box dilated by kDilate >= delta never loads such a cell and
// the pixel's outputs are the miss outputs. The mask marks a tile "traced" wherever the bounding rectangle of the projection of
// a dilated box's corners, widened by margin_px pixels, touches it; a box wholly behind the eye's plane marks nothing, and one
// that is neither wholly behind nor wholly in front by kMinDepth marks the whole view.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define VRT_MISS_HD __host__ __device__ inline
#else
#define VRT_MISS_HD inline
#endif

namespace vrt {
namespace miss {

constexpr int kTile = 8;               // the trace kernel's tile: 8 x 8 pixels, tiles indexed by FRAME row and column
// delta of the proof, per axis, in voxels: the march's 1,024 steps each add two roundings of a coordinate of at most 2^11 (the sum
// rp + dir * t and the push; half an ulp, 2^-14, each) and the push itself, 1e-4, and the roundings of the products dir * t add up to
// 2^-24 of the distance travelled, below 0.001: 0.001 + 1024 * (2 * 2^-14 + 1e-4) = 0.2284 (DESIGN §3 "Miss tiles", "The bound")
constexpr double kDelta = 0.24;
constexpr double kDilate = 0.25;       // voxels added to every side of a box: delta rounded up
static_assert(kDilate >= kDelta, "the mask must dilate the occupancy boxes by at least the proof's bound");
static_assert(kDelta >= 0.001 + 1024.0 * (2.0 / 16384.0 + 1e-4), "delta must cover the three terms of the proof");
constexpr double kMinDepth = 0.25;     // a dilated box whose corners are not all this far in front of the eye marks the view
constexpr int kMaxBoxes = 1 << 21;     // more boxes than this: no mask (the per-view build would cost more than it saves)
constexpr double kMaxEye = 65536.0;    // |gro| per axis above this: no mask (the proof's bound on the first step's rounding)
constexpr int kStableMin = 64;         // mask requests with an unchanged tree and bounds before a box list is made (at least) ...
constexpr int kStablePerRecords = 512; // ... and one per this many records of the tree
constexpr int kMaxWorld = 2048;        // world bounds beyond [-kMaxWorld, kMaxWorld]: no mask (the proof's bound on a position)

struct Box { int mn[3], mx[3]; };      // voxel cells [mn, mx) per axis

// floor(gro) inside the world: the march starts in the eye's cell and every step has t >= 0 (DESIGN §3 "Miss tiles"). From outside,
// the first step goes to the world's face in the direction of travel, behind rays that move away from it: such views get no mask.
VRT_MISS_HD bool eye_in_world(const float gro[3], const int wmin[3], const int wmax[3]) {
    for (int k = 0; k < 3; ++k)
        if (!((double)gro[k] >= (double)wmin[k] && (double)gro[k] < (double)wmax[k])) return false;   // NaN too
    return true;
}

// One view in the coordinates of its ray tables (View::gen_x / gen_y / gen_z). The kernel's ray through pixel (px, py) has the
// direction inv_view3x3 * (gen_x[px], gen_y[py], gen_z) up to rounding, so a point P lies on it when q = m * (P - eye) is a
// positive multiple of that vector: m is the inverse of inv_view's 3x3, eye = gro (cam_pos * voxel_scale) in voxels.
struct ViewParams {
    double m[9];              // row-major
    double eye[3];
    double gx0, gdx;          // gen_x[px] = gx0 + px * gdx up to rounding (affine in px: vrt_raygen.cpp)
    double gy0, gdy;
    double gz;                // gen_z
    double margin_px;         // pixels added to every side of a projected rectangle (float error of the tables and of the rays)
    int width, height, tiles_x, tiles_y;
};

// What a view's parameters take from its ray tables (vrt_raygen.cpp miss_table_fit(): once per table)
struct TableFit {
    double gx0, gdx, gy0, gdy, gz;
    double dev_px;            // the tables' largest distance from the affine fit, in pixels
    double gmax2;             // the largest |(gen_x, gen_y, gen_z)|^2
    int width, height;
};

// The projection of one box, in three steps that the host runs one after the other (box_tiles()) and the device build runs with one
// lane per corner, eight lanes per box (miss_mask_kernel): the same functions, hence the same arithmetic.
//   project_corner()  corner c (bit 0: x, 1: y, 2: z at the maximum) of b dilated by kDilate: its table coordinates, or behind / near
//   Extent            what the eight corners give together: the bounding rectangle, how many lie behind, whether one is near
//   extent_tiles()    the rectangle -> tiles
struct Extent {
    double lo_x, hi_x, lo_y, hi_y;
    int behind;      // corners behind the eye's plane
    int near;        // corners in front of it by less than kMinDepth
};
VRT_MISS_HD Extent empty_extent() { return Extent{1e300, -1e300, 1e300, -1e300, 0, 0}; }
VRT_MISS_HD Extent project_corner(const ViewParams &v, const Box &b, int c) {
    const double p[3] = {(double)((c & 1) ? b.mx[0] : b.mn[0]) + ((c & 1) ? kDilate : -kDilate) - v.eye[0],
                         (double)((c & 2) ? b.mx[1] : b.mn[1]) + ((c & 2) ? kDilate : -kDilate) - v.eye[1],
                         (double)((c & 4) ? b.mx[2] : b.mn[2]) + ((c & 4) ? kDilate : -kDilate) - v.eye[2]};
    const double qx = v.m[0] * p[0] + v.m[1] * p[1] + v.m[2] * p[2];
    const double qy = v.m[3] * p[0] + v.m[4] * p[1] + v.m[5] * p[2];
    const double qz = v.m[6] * p[0] + v.m[7] * p[1] + v.m[8] * p[2];
    const double depth = qz / v.gz;   // the ray parameter (in units of the table vector) of the corner's plane
    Extent e = empty_extent();
    if (depth < 0.0) { e.behind = 1; return e; }
    if (!(depth >= kMinDepth)) { e.near = 1; return e; }
    const double gx = qx / depth, gy = qy / depth;   // the table coordinates of the ray through the corner
    e.lo_x = e.hi_x = gx;
    e.lo_y = e.hi_y = gy;
    return e;
}
VRT_MISS_HD Extent merge_extent(Extent a, Extent b) {
    a.lo_x = b.lo_x < a.lo_x ? b.lo_x : a.lo_x; a.hi_x = b.hi_x > a.hi_x ? b.hi_x : a.hi_x;
    a.lo_y = b.lo_y < a.lo_y ? b.lo_y : a.lo_y; a.hi_y = b.hi_y > a.hi_y ? b.hi_y : a.hi_y;
    a.behind += b.behind; a.near += b.near;
    return a;
}

// The tiles a box with the extent e (all eight corners merged) may be seen through: 0 none (wholly behind the eye, or off the
// frame), 1 the inclusive rectangle t = {x0, y0, x1, y1}, 2 every tile of the view (the box reaches the eye's plane or the
// projection is not finite).
VRT_MISS_HD int extent_tiles(const ViewParams &v, const Extent &e, int t[4]) {
    if (e.behind == 8) return 0;             // convex and wholly behind: no ray of the view reaches it
    if (e.behind || e.near) return 2;
    // table coordinates -> pixels (either direction of the tables), widened by the margin
    double px0 = (e.lo_x - v.gx0) / v.gdx, px1 = (e.hi_x - v.gx0) / v.gdx;
    double py0 = (e.lo_y - v.gy0) / v.gdy, py1 = (e.hi_y - v.gy0) / v.gdy;
    if (px0 > px1) { const double s = px0; px0 = px1; px1 = s; }
    if (py0 > py1) { const double s = py0; py0 = py1; py1 = s; }
    px0 -= v.margin_px; px1 += v.margin_px; py0 -= v.margin_px; py1 += v.margin_px;
    if (!(px0 == px0) || !(px1 == px1) || !(py0 == py0) || !(py1 == py1)) return 2;
    if (px1 < 0.0 || py1 < 0.0 || px0 > (double)(v.width - 1) || py0 > (double)(v.height - 1)) return 0;   // off the frame
    const double x0 = px0 < 0.0 ? 0.0 : px0, y0 = py0 < 0.0 ? 0.0 : py0;
    const double x1 = px1 > (double)(v.width - 1) ? (double)(v.width - 1) : px1;
    const double y1 = py1 > (double)(v.height - 1) ? (double)(v.height - 1) : py1;
    t[0] = (int)x0 / kTile; t[1] = (int)y0 / kTile;   // pixel floor (non-negative), then its tile
    t[2] = (int)x1 / kTile; t[3] = (int)y1 / kTile;
    return 1;
}

// The tiles box b may be seen through (extent_tiles() of its eight corners)
VRT_MISS_HD int box_tiles(const ViewParams &v, const Box &b, int t[4]) {
    Extent e = empty_extent();
    for (int c = 0; c < 8; ++c) e = merge_extent(e, project_corner(v, b, c));
    return extent_tiles(v, e, t);
}

// Marks the tiles of box b "traced" in mask (tiles_x * tiles_y bytes): writes `stamp` there. A tile is traced when its byte equals
// the stamp of the build, so a mask buffer is rebuilt without clearing it first (the dispatcher steps the stamp per build and
// clears the buffer only when the stamp wraps). Returns true when b needs every tile of the view, which the caller then marks.
// The host's form (the test-support library); the device build splits the same steps over eight lanes per box.
VRT_MISS_HD bool mark_box(const ViewParams &v, const Box &b, uint8_t *mask, uint8_t stamp) {
    int t[4];
    const int r = box_tiles(v, b, t);
    if (r == 2) return true;
    if (r == 1)
        for (int ty = t[1]; ty <= t[3]; ++ty)
            for (int tx = t[0]; tx <= t[2]; ++tx) mask[ty * v.tiles_x + tx] = stamp;
    return false;
}

}  // namespace miss
}  // namespace vrt
