// vrt_launch_denoise_hdr.hip -- the HDR instances of the display pass (vrt_denoise.hip.h, include/vrt.h vrt_denoise_hdr) in a launch
// file of their own: the byte instances in vrt_launch_misc.hip keep their object code.
#include <hip/hip_runtime.h>

#include "vrt_launch.h"
#include "vrt_denoise.hip.h"

namespace vrt {
namespace launch {

hipError_t denoise_hdr(const DenoiseHdr &d, bool whole_groups, hipStream_t s) {
    using namespace vrt::denoise;
    Args a;
    a.rgba = nullptr;
    a.id = (const int2 *)d.id;
    a.out = (uint32_t *)d.out_rgba;
    a.width = d.width;
    a.height = d.height;
    denoise_tiling(d.width, d.height, a.tiles_x, a.n_tiles);
    a.group_order = d.group_order;
    a.tile_cost = d.tile_cost;
    a.rows_path = d.rows_path;
    a.rgb = (const float *)d.rgb;
    a.out_rgb = (float *)d.out_rgb;
    a.op = d.op;
    a.exposure = d.exposure;
    if (!whole_groups) {
        const dim3 grid((unsigned)a.tiles_x, (unsigned)(a.n_tiles / a.tiles_x));
        hipLaunchKernelGGL((denoise_px_kernel<2, 16, false, true>), grid, dim3(kTW / 2, 16), 0, s, a);
    } else {
        const long groups = ((long)a.n_tiles + kGroupTiles - 1) / kGroupTiles;
        hipLaunchKernelGGL((denoise_px_kernel<2, 16, true, true>), dim3((unsigned)(groups * kGroupTiles)), dim3(kTW / 2, 16), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace launch
}  // namespace vrt
