// vrt_sun.h -- the sun disc's block for a launch (include/vrt.h vrt_set_sun_disc, step 1), made by the host beside the light block
// (vrt_scene.cpp fill_light_args()): a header of its own so that the test library (test/vrt_test.hip vrt_test_sun_block) holds the
// product's function to the checker's basis. Every translation unit that includes it is compiled without contraction.
#pragma once
#include <math.h>

#include "vrt_args.h"

inline vrt::Sun sun_block(const float light_dir[3], float tan_radius) {
    // float32, one rounding per operation (this file is compiled without contraction): dot3 = (x*x + y*y) + z*z, len3 = sqrt(dot3),
    // normalize3(v) = v * (1 / sqrt(dot3(v))), cross3 as vrt_full.hip.h has it
    struct V3 { float x, y, z; };
    const auto dot = [](V3 p, V3 q) { return (p.x * q.x + p.y * q.y) + p.z * q.z; };
    const auto normalize = [&](V3 p) { const float s = 1.0f / sqrtf(dot(p, p)); return V3{p.x * s, p.y * s, p.z * s}; };
    const auto cross = [](V3 p, V3 q) { return V3{p.y * q.z - q.y * p.z, p.z * q.x - q.z * p.x, p.x * q.y - q.x * p.y}; };
    const V3 L{light_dir[0], light_dir[1], light_dir[2]};
    const V3 Ln = normalize(L);
    const V3 up = fabsf(Ln.z) < 0.999f ? V3{0.0f, 0.0f, 1.0f} : V3{1.0f, 0.0f, 0.0f};   // cosine_hemisphere's choice
    const V3 T = normalize(cross(up, Ln));
    const V3 B = cross(Ln, T);
    vrt::Sun s;
    s.tan_radius = tan_radius;
    s.ll = sqrtf(dot(L, L));
    s.Ln[0] = Ln.x; s.Ln[1] = Ln.y; s.Ln[2] = Ln.z;
    s.T[0] = T.x; s.T[1] = T.y; s.T[2] = T.z;
    s.B[0] = B.x; s.B[1] = B.y; s.B[2] = B.z;
    return s;
}
