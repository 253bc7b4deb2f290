// vrt_lens.hip.h -- the thin lens of the progressive accumulation (include/vrt.h vrt_set_lens), its LensSource in vrt_accum.hip.h.
// Lens sample k of a pixel is the sample of the accumulation (jittered or not, per its flags) traced from a point of the lens
// towards the point where the pinhole ray meets the plane of focus (vrt_common.hip.h lens_ray()); sample 0, the lens centre, is
// the frame. The lens point depends on k alone, so it is wave-uniform: its 24-bit sequence and the concentric disc map are made
// once per sample by every lane alike, on scalar loads of the direction numbers. The origin differs per lane only where a ray does
// not point forward (it keeps the eye), but nothing below relies on that.
//
// What the frame kernels take from the one eye of a view is taken from the view only where the dispatcher proved it for
// every origin the lens can produce (vrt_dispatch.cpp, vrt_layout.h lens_select()): the eye lookup (View::eye0 / eye1, or
// Lens::lane_eye and record_find() at the lane's own floor(o * u_voxelScale)), the first lookup of the wide traversals
// (View::first_valid, else their own find()), root 0's tightening, the v4 primary loop and the opaque chain.
#pragma once
#include "vrt_accum.h"
#include "vrt_full.hip.h"

namespace vrt {
namespace accum {

// Direction numbers of the lens sequence: x^3+x+1 with m = 1,1,5 (u) and x^3+x^2+1 with m = 1,3,1 (v)
struct LensDirs { uint32_t u[32], v[32]; };
constexpr void lens_dirs(uint32_t poly, const uint32_t (&m)[3], uint32_t (&v)[32]) {
    for (int i = 0; i < 3; ++i) v[i] = m[i] << (31 - i);
    for (int i = 3; i < 32; ++i) {
        uint32_t x = v[i - 3] ^ (v[i - 3] >> 3);
        if (poly & 2u) x ^= v[i - 1];
        if (poly & 1u) x ^= v[i - 2];
        v[i] = x;
    }
}
constexpr LensDirs make_lens_dirs() {
    LensDirs d{};
    lens_dirs(1u, {1u, 1u, 5u}, d.u);
    lens_dirs(2u, {1u, 3u, 1u}, d.v);
    return d;
}
__constant__ const LensDirs kLensDirs = make_lens_dirs();

// The lens point of sample k on the unit disc: (lu, lv) in [0, 1)^2, shifted by 1/2 so that sample 0 is the centre, then the
// concentric map (Shirley-Chiu) with the conventions' sin / cos
VRT_DEV void lens_point(uint32_t k, float &lx, float &ly) {
    uint32_t gu = 0u, gv = 0u;
    for (uint32_t i = 0, b = k; b; ++i, b >>= 1)
        if (b & 1u) { gu ^= kLensDirs.u[i]; gv ^= kLensDirs.v[i]; }
    const float lu = (float)((gu >> 8) ^ 0x800000u) * 0x1p-24f, lv = (float)((gv >> 8) ^ 0x800000u) * 0x1p-24f;
    full::concentric_disc(lu, lv, lx, ly);
}

// sample's lens ray of pixel (px, py), the medium at its origin included
VRT_DEV LensRay lens_sample(const KArgs &a, const View &vw, const Lens &L, int px, int py, uint32_t sample) {
    float lx, ly;
    lens_point(sample, lx, ly);
    const float jx = L.jitter ? jitter_x(sample) : 0.0f, jy = L.jitter ? jitter_y(sample) : 0.0f;
    LensRay lr = lens_ray(a, vw, px, py, jx, jy, L.aperture, L.focus, lx, ly);
    if (L.lane_eye) record_find(a, floor_i3(scale3(lr.o, a.voxel_scale)), lr.eye0, lr.eye1);
    else { lr.eye0 = vw.eye0; lr.eye1 = vw.eye1; }
    return lr;
}

}  // namespace accum
}  // namespace vrt
