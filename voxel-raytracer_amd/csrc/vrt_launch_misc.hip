// vrt_launch_misc.hip -- the kernels beside the tracer: the display pass (vrt_denoise.hip.h), the tile-order kernel of the
// feedback scheduler and the kernarg layout probe (both vrt_common.hip.h).
#include <hip/hip_runtime.h>

#include "vrt_launch.h"
#include "vrt_sched.hip.h"
#include "vrt_denoise.hip.h"

namespace vrt {
namespace launch {

hipError_t tile_order(const uint32_t *d_cost, uint32_t n_groups, uint32_t *d_order, uint32_t wave_slots, bool raise_lds, size_t lds_ceiling, hipStream_t s) {
    const size_t lds = (size_t)n_groups * sizeof(uint32_t);
    if (raise_lds) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&tile_order_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_ceiling);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(1024), lds, s, (const uint4 *)d_cost, n_groups, d_order, wave_slots);
    return hipGetLastError();
}

// Eight lanes per box, one per corner (vrt_miss.h project_corner), their extents merged across the eight with shuffles, then the
// box's tiles (extent_tiles) marked by the eight lanes together. A box that needs the whole view writes the stamp into the header
// word instead, which the trace kernels read as "every tile traced" (View::miss). No atomics, no fences: every store of a build
// writes the same value, and the trace launch that reads the mask follows in stream order.
constexpr uint32_t kMissLanes = 8;
__global__ __launch_bounds__(256) void miss_mask_kernel(const miss::ViewParams v, const miss::Box *boxes, uint32_t n, uint32_t *hdr,
                                                        uint32_t stamp) {
    uint8_t *mask = reinterpret_cast<uint8_t *>(hdr + 2);
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = g / kMissLanes, c = g % kMissLanes;
    if (i >= n) return;   // the same for the eight lanes of a box: every shuffle below reads a lane that takes part
    miss::Extent e = miss::project_corner(v, boxes[i], (int)c);
    for (int d = 1; d < (int)kMissLanes; d <<= 1) {
        miss::Extent o;
        o.lo_x = __shfl_xor(e.lo_x, d, kMissLanes); o.hi_x = __shfl_xor(e.hi_x, d, kMissLanes);
        o.lo_y = __shfl_xor(e.lo_y, d, kMissLanes); o.hi_y = __shfl_xor(e.hi_y, d, kMissLanes);
        o.behind = __shfl_xor(e.behind, d, kMissLanes); o.near = __shfl_xor(e.near, d, kMissLanes);
        e = miss::merge_extent(e, o);
    }
    int t[4];
    const int r = miss::extent_tiles(v, e, t);
    if (r == 2 && c == 0) hdr[0] = stamp;
    if (r == 1) {
        const uint32_t w = (uint32_t)(t[2] - t[0] + 1), cnt = w * (uint32_t)(t[3] - t[1] + 1);
        for (uint32_t k = c; k < cnt; k += kMissLanes) mask[(uint32_t)(t[1] + (int)(k / w)) * (uint32_t)v.tiles_x + (uint32_t)t[0] + k % w] = (uint8_t)stamp;
    }
}

hipError_t miss_mask(const miss::ViewParams &v, const int *d_boxes, uint32_t n, uint32_t *d_mask, uint8_t stamp, hipStream_t s) {
    const uint32_t blocks = n ? (uint32_t)(((uint64_t)n * kMissLanes + 255u) / 256u) : 1u;
    hipLaunchKernelGGL(miss_mask_kernel, dim3(blocks), dim3(256), 0, s, v, reinterpret_cast<const miss::Box *>(d_boxes), n, d_mask,
                       (uint32_t)stamp);
    return hipGetLastError();
}

hipError_t kernarg_probe(const KArgs &a, const ViewSet &vs, uint32_t *d_bad, hipStream_t s) {
    hipLaunchKernelGGL(kernarg_probe_kernel, dim3(1, kMaxViews), dim3(64), 0, s, a, vs, d_bad);
    return hipGetLastError();
}

void denoise_tiling(int width, int height, int &tiles_x, int &n_tiles) {
    tiles_x = (width + denoise::kTW - 1) / denoise::kTW;
    n_tiles = tiles_x * ((height + 15) / 16);
}

hipError_t denoise(const Denoise &d, bool whole_groups, hipStream_t s) {
    using namespace vrt::denoise;
    Args a;
    a.rgba = (const uint32_t *)d.rgba;
    a.id = (const int2 *)d.id;
    a.out = (uint32_t *)d.out;
    a.width = d.width;
    a.height = d.height;
    denoise_tiling(d.width, d.height, a.tiles_x, a.n_tiles);
    a.group_order = d.group_order;
    a.tile_cost = d.tile_cost;
    a.rows_path = d.rows_path;
    a.rgb = nullptr;   // the HDR instances' (vrt_launch_denoise_hdr.hip)
    a.out_rgb = nullptr;
    a.op = 0;
    a.exposure = 1.0f;
    if (!whole_groups) {
        const dim3 grid((unsigned)a.tiles_x, (unsigned)(a.n_tiles / a.tiles_x));
        hipLaunchKernelGGL((denoise_px_kernel<2, 16>), grid, dim3(kTW / 2, 16), 0, s, a);
    } else {
        const long groups = ((long)a.n_tiles + kGroupTiles - 1) / kGroupTiles;
        hipLaunchKernelGGL((denoise_px_kernel<2, 16, true>), dim3((unsigned)(groups * kGroupTiles)), dim3(kTW / 2, 16), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace launch
}  // namespace vrt
