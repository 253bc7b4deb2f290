// vrt_query.h -- the arguments of the query kernels (vrt_query.hip.h), shared by the host side (vrt_query.cpp) and the
// launch file (vrt_launch_query.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vrt {
namespace query {

// vrt_ray_hit (include/vrt.h), as the kernel stores it
struct RayHit {
    int32_t hit;
    int32_t coord[3];
    int32_t place[3];
    uint32_t leaf[2];
    int32_t steps;
};
static_assert(sizeof(RayHit) == 40, "vrt_ray_hit is 40 bytes");

struct RayArgs {
    const float *origins;         // n x 3, or one origin when origin_stride == 0
    int origin_stride;            // floats between origins: 0 or 3
    const float *dirs;            // n x 3
    float box_lo[3], box_hi[3];   // (float)(int) of the caller's worldMin / worldMax (ivec3_vec3 truncates)
    RayHit *out;
    uint32_t n;
};

struct PointArgs {
    const int32_t *coords;   // n x 3
    uint32_t *out;           // n x 3: present, leaf word 0, leaf word 1
    uint32_t n;
};

}  // namespace query
}  // namespace vrt
