// vrt_filter.hip.h -- the guided filter (include/vrt.h vrt_filter_hdr, points 1-5): an edge-avoiding a-trous filter on a float
// image, its edge weights from the guide planes. One lane per pixel in every kernel:
//   filter_prepass_kernel         g() of the guides, the live bit and the centre's depth slopes into the packed planes (vrt_filter.h)
//   filter_level_lattice_kernel   one level's 25 taps from a window staged in LDS: the levels of step 1, 2 and 4. FIRST reads the
//                                 caller's image as h(c) / m
//   filter_level_kernel           one level's 25 taps gathered from memory: the levels of step 8 and above
//   filter_through_kernel         levels == 0
// Either level kernel's LAST form remodulates, clamps, tone-maps and stores either output: no extra pass over the image at either
// end. Which form serves which step is what was measured (profiles/filter_levels_ab.txt). In both the sum order is the lane's own
// loop order over the same values, so the bits do not depend on the form or the launch shape. Every expression is the header's,
// operation by operation; tests/oracle_filter_hdr.c restates them.
#pragma once
#include "vrt_hdr.hip.h"
#include "vrt_filter.h"

namespace vrt {
namespace filter {

constexpr int kBlockX = 64, kBlockY = 4;   // a wave is 64 pixels of one row

// g(v) of point 1: NaN -> 0, anything else into [-65504, 65504]
VRT_DEV float guide_value(float v) { return v != v ? 0.0f : fmin_c(fmax_c(-accum::kHdrMax, v), accum::kHdrMax); }

// m of point 2 for one channel
VRT_DEV float modulation(float albedo, float coverage) { return fmax_c(albedo + (1.0f - coverage), 1.0f / 255.0f); }

VRT_DEV uint32_t tone_mapped(const float f[3], int op, float e) {
    return unorm8(accum::tone_map(f[0], op, e)) | (unorm8(accum::tone_map(f[1], op, e)) << 8) | (unorm8(accum::tone_map(f[2], op, e)) << 16) |
           (255u << 24);
}

VRT_DEV void store_pixel(float *out_rgb, uint32_t *out_rgba, size_t p, const float f[3], int op, float e) {
    if (out_rgb) { out_rgb[p * 3 + 0] = f[0]; out_rgb[p * 3 + 1] = f[1]; out_rgb[p * 3 + 2] = f[2]; }
    if (out_rgba) out_rgba[p] = tone_mapped(f, op, e);
}

// the smaller |Z_n - Z_p| over the two neighbours `stride` floats either side of p that exist (lo / hi) and are live; 0 if none
VRT_DEV float depth_slope(const Guides &g, size_t p, size_t stride, bool lo, bool hi, float zp) {
    float s = 0.0f;
    bool have = false;
    if (lo && guide_value(g.coverage[p - stride]) > 0.0f) {
        s = __builtin_fabsf(guide_value(g.depth[p - stride]) - zp);
        have = true;
    }
    if (hi && guide_value(g.coverage[p + stride]) > 0.0f) {
        const float d = __builtin_fabsf(guide_value(g.depth[p + stride]) - zp);
        s = have ? fmin_c(s, d) : d;
    }
    return s;
}

// The two kernels that are no templates live in one object, vrt_launch_filter.o: vrt_launch_filter_var.hip, which shares the device
// functions and launches these through vrt_launch.h, defines VRT_FILTER_NO_PLAIN_KERNELS
#ifndef VRT_FILTER_NO_PLAIN_KERNELS
__global__ __launch_bounds__(kBlockX *kBlockY) void filter_prepass_kernel(const Prepass q) {
    const int x = (int)(blockIdx.x * kBlockX + threadIdx.x), y = (int)(blockIdx.y * kBlockY + threadIdx.y);
    if (x >= q.width || y >= q.height) return;
    const size_t px = (size_t)q.width * (size_t)q.height, p = (size_t)y * (size_t)q.width + (size_t)x;
    const float cov = guide_value(q.g.coverage[p]);
    const bool live = cov > 0.0f;
    const float z = guide_value(q.g.depth[p]);
    float gx = 0.0f, gy = 0.0f;
    if (live) {
        gx = depth_slope(q.g, p, 1, x > 0, x + 1 < q.width, z);
        gy = depth_slope(q.g, p, (size_t)q.width, y > 0, y + 1 < q.height, z);
    }
    q.pack[p] = make_float4(guide_value(q.g.normal[p * 3 + 0]), guide_value(q.g.normal[p * 3 + 1]), guide_value(q.g.normal[p * 3 + 2]),
                            live ? z : __uint_as_float(0x7fc00000u));
    q.pack[px + p] = make_float4(guide_value(q.g.albedo[p * 4 + 0]), guide_value(q.g.albedo[p * 4 + 1]), guide_value(q.g.albedo[p * 4 + 2]),
                                 guide_value(q.g.albedo[p * 4 + 3]));
    q.pack[2 * px + p] = make_float4(gx, gy, cov, 0.0f);
}
#endif

// e of one tap from the guides (point 4): n_* = normal and depth, a_* = albedo of the centre p and the tap q,
// slope = gx * |ox| s + gy * |oy| s, zfloor = Z_p / 256. The variance-guided kernels (vrt_filter_var.hip.h) add their term to it.
VRT_DEV float tap_exponent(float kn, float ka, float sigma_depth, const float4 &n_p, const float4 &a_p, const float4 &n_q, const float4 &a_q,
                           float slope, float zfloor) {
    const float dx = n_q.x - n_p.x, dy = n_q.y - n_p.y, dz = n_q.z - n_p.z;
    const float dn2 = (dx * dx + dy * dy) + dz * dz;
    const float a0 = a_q.x - a_p.x, a1 = a_q.y - a_p.y, a2 = a_q.z - a_p.z, a3 = a_q.w - a_p.w;
    const float da2 = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
    const float dzq = __builtin_fabsf(n_q.w - n_p.w);
    const float den = sigma_depth * (slope + zfloor) + 0x1p-20f;
    return (dn2 * kn + da2 * ka) + dzq / den;
}

// w of one tap (point 4): b = B[|oy|] * B[|ox|]
VRT_DEV float tap_weight(const Level &q, const float4 &n_p, const float4 &a_p, const float4 &n_q, const float4 &a_q, float slope, float zfloor,
                         float b) {
    return b * det_expf(-tap_exponent(q.kn, q.ka, q.sigma_depth, n_p, a_p, n_q, a_q, slope, zfloor));
}

VRT_DEV float b3(int a) { return a == 0 ? 0.375f : (a == 1 ? 0.25f : 0.0625f); }

// u of pixel t as the first level reads it: h(c) / m (a_t: its albedo word)
VRT_DEV float4 first_colour(const Level &q, size_t px, size_t t, const float4 &a_t) {
    float4 u = make_float4(accum::hdr_value(q.rgb[t * 3 + 0]), accum::hdr_value(q.rgb[t * 3 + 1]), accum::hdr_value(q.rgb[t * 3 + 2]), 0.0f);
    if (q.demodulate) {   // the same in every lane; without it m = 1 and h(c) / 1 is h(c)
        const float cov = q.pack[2 * px + t].z;
        u.x = u.x / modulation(a_t.x, cov);
        u.y = u.y / modulation(a_t.y, cov);
        u.z = u.z / modulation(a_t.z, cov);
    }
    return u;
}

// a pixel that is not live: h(c), from the last level only (no level reads it as a tap)
template <bool LAST>
VRT_DEV void pass_through(const Level &q, size_t p) {
    if (LAST) {
        const float f[3] = {accum::hdr_value(q.rgb[p * 3 + 0]), accum::hdr_value(q.rgb[p * 3 + 1]), accum::hdr_value(q.rgb[p * 3 + 2])};
        store_pixel(q.out_rgb, q.out_rgba, p, f, q.op, q.exposure);
    }
}

// u' = sum / sumw into the next level's image, or (point 5) remodulated, clamped and tone-mapped into the outputs
template <bool LAST>
VRT_DEV void finish_pixel(const Level &q, size_t p, const float sum[3], float sumw, const float4 &a_p, float cov) {
    const float r[3] = {sum[0] / sumw, sum[1] / sumw, sum[2] / sumw};
    if (LAST) {
        float m[3] = {1.0f, 1.0f, 1.0f};
        if (q.demodulate) { m[0] = modulation(a_p.x, cov); m[1] = modulation(a_p.y, cov); m[2] = modulation(a_p.z, cov); }
        const float f[3] = {accum::hdr_value(r[0] * m[0]), accum::hdr_value(r[1] * m[1]), accum::hdr_value(r[2] * m[2])};
        store_pixel(q.out_rgb, q.out_rgba, p, f, q.op, q.exposure);
    } else {
        q.dst[p] = make_float4(r[0], r[1], r[2], 0.0f);
    }
}

// The gather form: tap (ox, oy) of every lane of a wave lies s * ox pixels along the same row, so each of a tap's loads moves 64
// adjacent 16-byte words whatever the step. Never the first level (step 1 takes the lattice form).
template <bool LAST>
__global__ __launch_bounds__(kBlockX *kBlockY) void filter_level_kernel(const Level q) {
    const int x = (int)(blockIdx.x * kBlockX + threadIdx.x), y = (int)(blockIdx.y * kBlockY + threadIdx.y);
    if (x >= q.width || y >= q.height) return;
    const size_t px = (size_t)q.width * (size_t)q.height, p = (size_t)y * (size_t)q.width + (size_t)x;
    const float4 n_p = q.pack[p];
    if (!(n_p.w == n_p.w)) return pass_through<LAST>(q, p);
    const float4 a_p = q.pack[px + p], c_p = q.pack[2 * px + p];
    const float gx = c_p.x, gy = c_p.y;
    const float zfloor = n_p.w * (1.0f / 256.0f);
    const int s = q.step;
    float sumw = 0.0f, sum[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int oy = -2; oy <= 2; ++oy) {
        const int ty = y + oy * s;
        if (ty < 0 || ty >= q.height) continue;
        const int ay = oy < 0 ? -oy : oy;
        const float ry = gy * (float)(ay * s);
#pragma unroll
        for (int ox = -2; ox <= 2; ++ox) {
            const int tx = x + ox * s;
            if (tx < 0 || tx >= q.width) continue;
            const size_t t = (size_t)ty * (size_t)q.width + (size_t)tx;
            const float4 n_q = q.pack[t];
            if (!(n_q.w == n_q.w)) continue;
            const float4 a_q = q.pack[px + t];
            const int ax = ox < 0 ? -ox : ox;
            const float w = tap_weight(q, n_p, a_p, n_q, a_q, gx * (float)(ax * s) + ry, zfloor, b3(ay) * b3(ax));
            const float4 u = q.src[t];
            sumw = sumw + w;
            sum[0] = sum[0] + w * u.x;
            sum[1] = sum[1] + w * u.y;
            sum[2] = sum[2] + w * u.z;
        }
    }
    finish_pixel<LAST>(q, p, sum, sumw, a_p, c_p.z);
}

// The lattice form: the same level with its taps staged in LDS. At step s a workgroup owns a kLatX x kLatY tile of ONE residue class (x mod s, y mod s):
// in that class's own lattice the 25 taps are dense, so a (kLatX + 4) x (kLatY + 4) window of packed words and colours serves the
// whole tile -- 1.7 loads per pixel and plane instead of 25 -- and the first level's h(c) / m is evaluated once per staged pixel.
// The residue is the fastest-varying part of the block index: the s workgroups whose lanes share cache lines are dispatched together.
// A word outside the image is staged as not live. The sums run in the same order over the same values: the same bits. A lane's
// loads and stores lie s words apart, which is what the form pays: it wins up to step 4 and loses from step 8 on.
constexpr int kLatX = 32, kLatY = 8, kWinX = kLatX + 4, kWinY = kLatY + 4;

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kLatX *kLatY) void filter_level_lattice_kernel(const Level q) {
    __shared__ float4 s_n[kWinX * kWinY], s_a[kWinX * kWinY], s_u[kWinX * kWinY];
    const int s = q.step;
    const int rx = (int)(blockIdx.x % (unsigned)s), ry = (int)(blockIdx.y % (unsigned)s);
    const int lx0 = (int)(blockIdx.x / (unsigned)s) * kLatX, ly0 = (int)(blockIdx.y / (unsigned)s) * kLatY;
    if (rx + s * lx0 >= q.width || ry + s * ly0 >= q.height) return;   // the whole workgroup: this class has fewer tiles
    const size_t px = (size_t)q.width * (size_t)q.height;
    for (int i = (int)(threadIdx.y * kLatX + threadIdx.x); i < kWinX * kWinY; i += kLatX * kLatY) {
        const int wy = i / kWinX, wx = i - wy * kWinX;
        const int x = rx + s * (lx0 - 2 + wx), y = ry + s * (ly0 - 2 + wy);
        float4 n = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x7fc00000u)), a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), u = a;
        if (x >= 0 && x < q.width && y >= 0 && y < q.height) {
            const size_t t = (size_t)y * (size_t)q.width + (size_t)x;
            n = q.pack[t];
            if (n.w == n.w) {
                a = q.pack[px + t];
                u = FIRST ? first_colour(q, px, t, a) : q.src[t];
            }
        }
        s_n[i] = n;
        s_a[i] = a;
        s_u[i] = u;
    }
    __syncthreads();
    const int x = rx + s * (lx0 + (int)threadIdx.x), y = ry + s * (ly0 + (int)threadIdx.y);
    if (x >= q.width || y >= q.height) return;
    const size_t p = (size_t)y * (size_t)q.width + (size_t)x;
    const int c = ((int)threadIdx.y + 2) * kWinX + (int)threadIdx.x + 2;
    const float4 n_p = s_n[c];
    if (!(n_p.w == n_p.w)) return pass_through<LAST>(q, p);
    const float4 a_p = s_a[c], c_p = q.pack[2 * px + p];
    const float gx = c_p.x, gy = c_p.y;
    const float zfloor = n_p.w * (1.0f / 256.0f);
    float sumw = 0.0f, sum[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int oy = -2; oy <= 2; ++oy) {
        const int ay = oy < 0 ? -oy : oy;
        const float ry_ = gy * (float)(ay * s);
#pragma unroll
        for (int ox = -2; ox <= 2; ++ox) {
            const int i = c + oy * kWinX + ox;
            const float4 n_q = s_n[i];
            if (!(n_q.w == n_q.w)) continue;   // not live, or outside the image
            const int ax = ox < 0 ? -ox : ox;
            const float w = tap_weight(q, n_p, a_p, n_q, s_a[i], gx * (float)(ax * s) + ry_, zfloor, b3(ay) * b3(ax));
            const float4 u = s_u[i];
            sumw = sumw + w;
            sum[0] = sum[0] + w * u.x;
            sum[1] = sum[1] + w * u.y;
            sum[2] = sum[2] + w * u.z;
        }
    }
    finish_pixel<LAST>(q, p, sum, sumw, a_p, c_p.z);
}

#ifndef VRT_FILTER_NO_PLAIN_KERNELS
__global__ __launch_bounds__(256) void filter_through_kernel(const Through q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= q.pixels) return;
    const size_t p = i;
    float f[3] = {accum::hdr_value(q.rgb[p * 3 + 0]), accum::hdr_value(q.rgb[p * 3 + 1]), accum::hdr_value(q.rgb[p * 3 + 2])};
    const float cov = guide_value(q.g.coverage[p]);
    if (q.demodulate && cov > 0.0f) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float m = modulation(guide_value(q.g.albedo[p * 4 + k]), cov);
            f[k] = accum::hdr_value(f[k] / m * m);
        }
    }
    store_pixel(q.out_rgb, q.out_rgba, p, f, q.op, q.exposure);
}
#endif

}  // namespace filter
}  // namespace vrt
