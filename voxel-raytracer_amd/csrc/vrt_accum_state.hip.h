// vrt_accum_state.hip.h -- the progressive accumulation's kernels that trace nothing: the resolves of the integer sums, the list of
// an adaptive round's tiles and vrt_accum_counts' kernel (vrt_accum.hip.h: the kernels that add samples). Included by
// vrt_launch_accum.hip alone: these are not templates.
#pragma once
#include "vrt_accum.hip.h"

namespace vrt {
namespace accum {

__global__ __launch_bounds__(256) void accum_resolve_kernel(const Resolve q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= q.pixels) return;
    const uint4 s = reinterpret_cast<const uint4 *>(q.sums)[i];
    const uint32_t h = q.n >> 1;
    q.out_rgba[i] = ((s.x + h) / q.n) | (((s.y + h) / q.n) << 8) | (((s.z + h) / q.n) << 16) | (255u << 24);
}

// An adaptive accumulation's resolve: each pixel by its own count (the fourth word; >= 1 after the first round, as min >= 2)
__global__ __launch_bounds__(256) void adaptive_resolve_kernel(const Resolve q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= q.pixels) return;
    const uint4 s = reinterpret_cast<const uint4 *>(q.sums)[i];
    const uint32_t n = s.w > 0u ? s.w : 1u, h = n >> 1;
    q.out_rgba[i] = ((s.x + h) / n) | (((s.y + h) / n) << 8) | (((s.z + h) / n) << 16) | (255u << 24);
}

// One lane per tile: does it hold an active pixel? Active tiles of a wave are appended with one atomic (ballot, mbcnt offsets);
// the list's order does not matter, as every pixel's samples depend on that pixel alone.
__global__ __launch_bounds__(256) void compact_tiles_kernel(const Tiles t) {
    const int tiles_x = (t.width + 7) / 8, n_tiles = tiles_x * ((t.height + 7) / 8);
    const int tile = (int)(blockIdx.x * 256u + threadIdx.x);
    bool any = false;
    if (tile < n_tiles) {
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int x1 = min(tx * 8 + 8, t.width), y1 = min(ty * 8 + 8, t.height);
        for (int y = ty * 8; y < y1 && !any; ++y)
            for (int x = tx * 8; x < x1 && !any; ++x) {
                const size_t o = (size_t)y * (size_t)t.width + (size_t)x;
                const uint4 s = reinterpret_cast<const uint4 *>(t.sums)[o];
                any = adaptive_active(s.w, (uint64_t)s.x + s.y + s.z, t.sq[o], t.min, t.max, t.tol);
            }
    }
    const uint64_t mask = __ballot(any);
    if (mask == 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0u;
    if (lane == (uint32_t)(__ffsll((unsigned long long)mask) - 1)) base = atomicAdd(t.n_tiles, (uint32_t)__popcll(mask));
    base = __shfl(base, __ffsll((unsigned long long)mask) - 1);
    if (any) t.tiles[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)tile;
}

// vrt_accum_counts: a grid-stride loop, one pixel per lane per step; each wave counts its active pixels with ballots and adds
// them with one atomic at the end (one atomic per pixel wave serialised on the one word: 0.25 ms at 1080p)
__global__ __launch_bounds__(256) void adaptive_counts_kernel(const Counts c) {
    const uint32_t stride = gridDim.x * 256u;
    uint32_t wave_active = 0u;
    for (uint32_t base = blockIdx.x * 256u + (threadIdx.x & ~63u); base < c.pixels; base += stride) {   // uniform per wave
        const uint32_t i = base + (threadIdx.x & 63u);
        bool act = false;
        if (i < c.pixels) {
            const uint4 s = reinterpret_cast<const uint4 *>(c.sums)[i];
            c.out[i] = s.w;
            act = adaptive_active(s.w, (uint64_t)s.x + s.y + s.z, c.sq[i], c.min, c.max, c.tol);
        }
        wave_active += (uint32_t)__popcll(__ballot(act));
    }
    if ((threadIdx.x & 63u) == 0u && wave_active != 0u) atomicAdd(c.n_active, wave_active);
}

}  // namespace accum
}  // namespace vrt
