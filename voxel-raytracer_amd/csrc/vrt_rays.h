// vrt_rays.h -- the arguments of the ray-batch kernels (vrt_rays.hip.h), shared by the host side (vrt_rays.cpp) and the launch
// file (vrt_launch_rays.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vrt {
namespace rays {

// The kernels' third argument, behind KArgs and ViewSet (whose places in the kernarg segment late_args() / late_view() rely on)
struct Args {
    const float *origins;     // n x 3, or one origin when origin_stride == 0
    const float *dirs;        // n x 3
    uint32_t *out_rgba;       // n packed R | G<<8 | B<<16 | A<<24, or null
    int2 *out_id;             // n (voxelID, dist), or null
    uint32_t n;
    int origin_stride;        // floats between origins: 0 or 3
    uint32_t width;           // the batch as an image of this width: ray i seeds initRNG(i % width, i / width, sample)
    uint32_t tiles_x;         // != 0: a wave takes the 8 x 8 tile blockIdx.x of that image, tiles_x tiles per row; 0: 64 consecutive rays
    uint32_t first, n_samples;
};

// Which mapping a batch takes (vrt_rays.hip.h ray_of_lane()): images -- at least 8 wide and two rows high -- keep the frame kernels'
// 8 x 8 tiles, everything else is a list. Returns the grid (waves) and sets tiles_x.
inline uint32_t plan(uint32_t n, uint32_t width, uint32_t &tiles_x) {
    tiles_x = 0u;
    if (width >= 8u && n / width >= 2u) {
        const uint32_t rows = (n + width - 1u) / width;
        tiles_x = (width + 7u) / 8u;
        return tiles_x * ((rows + 7u) / 8u);
    }
    return (n + 63u) / 64u;
}

}  // namespace rays
}  // namespace vrt
