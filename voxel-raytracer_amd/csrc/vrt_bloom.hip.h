// vrt_bloom.hip.h -- bloom on the device (include/vrt.h vrt_bloom_hdr, points B0-B8): the bright pass and the down-sampling pyramid,
// the up-sampling chain, and the composite fused with the tone map.
//
// bloom_down_kernel<FIRST, KARIS, GATHER>: one level of B4, one lane per destination pixel, a workgroup per kTX x kTY destination
// tile (a 1-D grid of tiles: a frame one pixel wide has more rows of tiles than a grid has in y). With GATHER false the workgroup
// stages the (2 kTX + 2) x (2 kTY + 2) source window in LDS as float4 first -- FIRST applies B2 / B3 while staging, so an input pixel
// is bright-passed once per tile that holds it, not once per tap -- and each lane then reads its 16 taps with 16-byte LDS loads. A
// window row lies as two planes, the even columns and the odd ones: lane lx reads entries lx and lx + 1 of each, so the 16 lanes that
// share an LDS cycle read 256 contiguous bytes, every bank once; with the columns interleaved they would read every other float4 and
// meet two-way conflicts. The planes are kHalf = 36 entries apart so that the staging stores, whose lanes alternate between the two,
// fall 16 banks apart too. With GATHER true each lane takes its 16 taps from memory (FIRST: through B2 / B3 each). Both forms add in
// the same order -- the lane's own, B4's -- and give the same bits; profiles/bloom_ab.txt has both measured, the launch file
// instantiates the one that is kept (kGather).
// bloom_up_kernel<LAST>: one step of B6, one lane per destination pixel: four gathered float4 taps of the coarser level (B5) added to
// the lane's own pixel in place. LAST is B7 / B8 instead: the taps of U_1, the input pixel, f and its tone-mapped bytes.
// No inline assembly. The resources are in profiles/bloom_resource_usage.txt.
#pragma once
#include "vrt_accum.hip.h"   // accum::hdr_value, accum::mom_luminance (E1), accum::tone_map, unorm8
#include "vrt_bloom.h"

namespace vrt {
namespace bloom {

constexpr int kTX = 32, kTY = 8, kBlock = kTX * kTY;
constexpr int kWinW = 2 * kTX + 2, kWinH = 2 * kTY + 2;
constexpr int kHalf = 36, kRow = 2 * kHalf;   // a window row in LDS: its even columns, then its odd ones
static_assert(kHalf >= kTX + 1 && kTX == 32, "a plane holds the kTX + 1 columns of its parity; the lane mapping shifts by five");
#ifndef VRT_BLOOM_GATHER
#define VRT_BLOOM_GATHER 0   // the form the library is built with (profiles/bloom_ab.txt)
#endif
constexpr bool kGather = VRT_BLOOM_GATHER != 0;
constexpr float kFloatMax = 3.402823466e38f;

VRT_DEV float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
VRT_DEV float4 scale4(const float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
VRT_DEV int clamp_i(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// B4's T: [1 3 3 1] with additions only
VRT_DEV float4 tent(const float4 a0, const float4 a1, const float4 a2, const float4 a3) {
    const float4 p0 = add4(a0, a1), p1 = add4(a1, a2), p2 = add4(a2, a3);
    return add4(add4(p0, p1), add4(p1, p2));
}

// B1 (and E9's e): the record's exposure with the caller's
VRT_DEV float record_exposure(const vrt_exposure *record, float exposure) {
    if (!record) return exposure;
    return fmin_c(exposure * record->exposure, kFloatMax);
}

// B2, B3 of the input pixel at c
template <bool KARIS>
VRT_DEV float4 bright_pixel(const float *c, float eb, const Bright &q) {
    const float in[3] = {c[0], c[1], c[2]};
    const float ye = fmin_c(accum::mom_luminance(in) * eb, kFloatMax);
    const float d = ye - q.threshold;
    float soft = 0.0f;
    if (q.knee > 0.0f) {
        const float s = fmin_c(fmax_c(d + q.knee, 0.0f), q.knee + q.knee);
        soft = (s * s) / (4.0f * q.knee);
    }
    const float a = fmax_c(fmax_c(soft, d), 0.0f);
    const float g = fmin_c(a / fmax_c(ye, 0x1p-16f), 1.0f);
    float b[3] = {accum::hdr_value(in[0]) * g, accum::hdr_value(in[1]) * g, accum::hdr_value(in[2]) * g};
    float w = 1.0f;
    if (KARIS) {
        w = 1.0f / (1.0f + accum::mom_luminance(b));
        b[0] = b[0] * w;
        b[1] = b[1] * w;
        b[2] = b[2] * w;
    }
    return make_float4(b[0], b[1], b[2], w);
}

template <bool FIRST, bool KARIS, bool GATHER>
__global__ __launch_bounds__(kBlock) void bloom_down_kernel(const DownArgs q) {
    const uint32_t tiles_x = ((uint32_t)q.dw + kTX - 1u) / kTX;
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int lx = (int)(threadIdx.x & (kTX - 1)), ly = (int)(threadIdx.x >> 5);
    const int X = (int)(tile_x * kTX) + lx, Y = (int)(tile_y * kTY) + ly;
    const float eb = FIRST ? record_exposure(q.bright.record, q.bright.exposure) : 0.0f;   // one address for every lane
    // the source pixel (gx, gy) with B4's clamp: always inside the sw x sh source
    const auto fetch = [&](int gx, int gy) -> float4 {
        const size_t p = (size_t)clamp_i(gy, q.sh - 1) * (size_t)q.sw + (size_t)clamp_i(gx, q.sw - 1);
        if (FIRST) return bright_pixel<KARIS>(q.rgb + p * 3u, eb, q.bright);
        return reinterpret_cast<const float4 *>(q.src)[p];
    };
    float4 r[4];
    if (GATHER) {
        if (X >= q.dw || Y >= q.dh) return;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gy = 2 * Y - 1 + j, gx = 2 * X - 1;
            r[j] = tent(fetch(gx, gy), fetch(gx + 1, gy), fetch(gx + 2, gy), fetch(gx + 3, gy));
        }
    } else {
        __shared__ float4 s_win[kWinH * kRow];
        const int x0 = 2 * (int)(tile_x * kTX) - 1, y0 = 2 * (int)(tile_y * kTY) - 1;
        for (int i = (int)threadIdx.x; i < kWinW * kWinH; i += kBlock) {
            const int sy = i / kWinW, sx = i - sy * kWinW;
            s_win[sy * kRow + (sx & 1) * kHalf + (sx >> 1)] = fetch(x0 + sx, y0 + sy);
        }
        __syncthreads();
        if (X >= q.dw || Y >= q.dh) return;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 *row = s_win + (2 * ly + j) * kRow + lx;   // window columns 2 lx .. 2 lx + 3
            r[j] = tent(row[0], row[kHalf], row[1], row[kHalf + 1]);
        }
    }
    float4 v = scale4(tent(r[0], r[1], r[2], r[3]), 0.015625f);
    if (FIRST && KARIS) v = make_float4(v.x / v.w, v.y / v.w, v.z / v.w, 1.0f);
    reinterpret_cast<float4 *>(q.dst)[(size_t)Y * (size_t)q.dw + (size_t)X] = v;
}

// B5's lerp and up(S, ., .) at destination (x, y); S is sw x sh
VRT_DEV float4 lerp4(const float4 fa, const float4 ne) { return scale4(add4(add4(fa, ne), add4(ne, ne)), 0.25f); }
VRT_DEV float4 up_sample(const float4 *s, int sw, int sh, int x, int y) {
    const int nx = x >> 1, ny = y >> 1;
    const int fx = clamp_i(nx + ((x & 1) ? 1 : -1), sw - 1), fy = clamp_i(ny + ((y & 1) ? 1 : -1), sh - 1);
    const float4 *rf = s + (size_t)fy * (size_t)sw, *rn = s + (size_t)ny * (size_t)sw;
    return lerp4(lerp4(rf[fx], rf[nx]), lerp4(rn[fx], rn[nx]));
}

template <bool LAST>
__global__ __launch_bounds__(kBlock) void bloom_up_kernel(const UpArgs q) {
    const uint32_t tiles_x = ((uint32_t)q.dw + kTX - 1u) / kTX;
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x = (int)(tile_x * kTX) + (int)(threadIdx.x & (kTX - 1)), y = (int)(tile_y * kTY) + (int)(threadIdx.x >> 5);
    if (x >= q.dw || y >= q.dh) return;
    // nx = x >> 1 <= (dw - 1) >> 1 <= sw - 1 (sw = half_up(dw)): the near tap needs no clamp
    const float4 u = up_sample(reinterpret_cast<const float4 *>(q.src), q.sw, q.sh, x, y);
    const size_t p = (size_t)y * (size_t)q.dw + (size_t)x;
    if (!LAST) {
        float4 *d = reinterpret_cast<float4 *>(q.dst) + p;
        *d = add4(*d, u);
        return;
    }
    const float e = record_exposure(q.record, q.exposure);
    const float *c = q.rgb + p * 3u;
    const float fr = accum::hdr_value(accum::hdr_value(c[0]) + q.intensity * (u.x * q.inv_levels));
    const float fg = accum::hdr_value(accum::hdr_value(c[1]) + q.intensity * (u.y * q.inv_levels));
    const float fb = accum::hdr_value(accum::hdr_value(c[2]) + q.intensity * (u.z * q.inv_levels));
    if (q.out_rgb) {
        float *o = q.out_rgb + p * 3u;
        o[0] = fr;
        o[1] = fg;
        o[2] = fb;
    }
    if (q.out_rgba)
        q.out_rgba[p] = unorm8(accum::tone_map(fr, q.op, e)) | (unorm8(accum::tone_map(fg, q.op, e)) << 8) |
                        (unorm8(accum::tone_map(fb, q.op, e)) << 16) | (255u << 24);
}

}  // namespace bloom
}  // namespace vrt
