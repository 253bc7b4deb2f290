// vrt_rays.h -- the arguments of the ray-batch kernels (vrt_rays.hip.h), shared by the host side (vrt_rays.cpp) and the launch
// file (vrt_launch_rays.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

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

// The HDR forms (include/vrt.h vrt_shade_rays_hdr): the kernels' template parameter HDR picks this type (ArgsOf), so the plain
// kernels keep Args and their code. Args::out_rgba takes the tone-mapped bytes of the mean; Args::n_samples is the call's own
// in every mode (the primary modes trace one sample and add it n_samples times over).
struct HdrArgs : Args {
    double *sums;             // n x 3 float64, read before the first sample and written after the last, or null (start at +0.0)
    float *out_rgb;           // n x 3 floats: the mean, or null
    uint32_t n_total;         // n_prior + n_samples: what the mean divides by
    int32_t op;               // VRT_TONEMAP_*
    float exposure;
};
template <bool HDR>
using ArgsOf = typename std::conditional<HDR, HdrArgs, Args>::type;

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
