// vrt_filter_var.hip.h -- the variance-guided filter (include/vrt.h vrt_filter_hdr_var, points V1-V4): the guided filter's levels
// with an edge-stopping luminance term whose width is the pixel's own variance, and that variance carried through the levels. One
// lane per pixel in every kernel:
//   filter_variance_kernel            V2: the initial variance of every live pixel into the packed planes -- SPATIAL: the 7 x 7
//                                     guide-weighted estimate from a window staged in LDS; otherwise the caller's plane, demodulated
//   filter_var_level_lattice_kernel   V3 from a window staged in LDS: the levels of step 1, 2 and 4
//   filter_var_level_kernel           V3 gathered from memory: the levels of step 8 and above
// The prepass, levels == 0's colours and every device function the two filters have in common (tap_exponent, b3, first_colour,
// modulation, store_pixel, finish_pixel, pass_through) are vrt_filter.hip.h's: these are new kernels, not new parameters of the old
// ones. The variance rides in words the guide-only filter leaves unused (vrt_filter.h), so a level stages what its guide-only form
// stages: 20,736 bytes of LDS. Every expression is the header's, operation by operation; tests/oracle_filter_var.c restates them.
#pragma once
#include "vrt_filter.hip.h"

namespace vrt {
namespace filter {

constexpr float kVarMax = 65504.0f * 65504.0f;

// V1
VRT_DEV float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// hv(x) of V2 and V4: NaN, -0 and everything negative -> +0, else at most 65504^2
VRT_DEV float var_value(float v) { return fmin_c(fmax_c(0.0f, v), kVarMax); }

// Ym * Ym of a live pixel: the square of the luminance of its modulation; 1 without demodulation
VRT_DEV float modulation_lum2(const Level &q, const float4 &a_p, float cov) {
    if (!q.demodulate) return 1.0f;
    const float ym = luminance(modulation(a_p.x, cov), modulation(a_p.y, cov), modulation(a_p.z, cov));
    return ym * ym;
}

// ---- V2 ----
// A workgroup owns a kVarX x kVarY tile; its 49 taps at step 1 are dense, so a (kVarX + 6) x (kVarY + 6) window serves the tile: the
// two guide words and ONE float of luminance per staged pixel (h(c) / m is evaluated once per staged pixel, not 49 times), 19,152
// bytes. A wave's 16-byte reads are 32 adjacent words of one window row twice: every 16-lane group covers the 16 slots of a bank row.
constexpr int kVarX = 32, kVarY = 8, kVarWinX = kVarX + 6, kVarWinY = kVarY + 6;

template <bool SPATIAL>
__global__ __launch_bounds__(kVarX *kVarY) void filter_variance_kernel(const Variance q) {
    __shared__ float4 s_n[SPATIAL ? kVarWinX * kVarWinY : 1], s_a[SPATIAL ? kVarWinX * kVarWinY : 1];
    __shared__ float s_l[SPATIAL ? kVarWinX * kVarWinY : 1];
    const Level &l = q.l;
    const size_t px = (size_t)l.width * (size_t)l.height;
    const int x0 = (int)blockIdx.x * kVarX, y0 = (int)blockIdx.y * kVarY;
    if (SPATIAL) {
        for (int i = (int)(threadIdx.y * kVarX + threadIdx.x); i < kVarWinX * kVarWinY; i += kVarX * kVarY) {
            const int wy = i / kVarWinX, wx = i - wy * kVarWinX;
            const int x = x0 - 3 + wx, y = y0 - 3 + wy;
            float4 n = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x7fc00000u)), a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float lum = 0.0f;
            if (x >= 0 && x < l.width && y >= 0 && y < l.height) {
                const size_t t = (size_t)y * (size_t)l.width + (size_t)x;
                n = l.pack[t];
                if (n.w == n.w) {
                    a = l.pack[px + t];
                    const float4 u = first_colour(l, px, t, a);
                    lum = luminance(u.x, u.y, u.z);
                }
            }
            s_n[i] = n;
            s_a[i] = a;
            s_l[i] = lum;
        }
        __syncthreads();
    }
    const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
    if (x >= l.width || y >= l.height) return;
    const size_t p = (size_t)y * (size_t)l.width + (size_t)x;
    const int c = ((int)threadIdx.y + 3) * kVarWinX + (int)threadIdx.x + 3;
    const float4 n_p = SPATIAL ? s_n[c] : l.pack[p];
    if (!(n_p.w == n_p.w)) {   // not live: plane 2's .w stays the prepass's 0
        if (q.out_variance) q.out_variance[p] = 0.0f;
        return;
    }
    const float4 a_p = SPATIAL ? s_a[c] : l.pack[px + p], c_p = l.pack[2 * px + p];
    const float ym2 = modulation_lum2(l, a_p, c_p.z);
    float v0;
    if (SPATIAL) {
        const float gx = c_p.x, gy = c_p.y;
        const float zfloor = n_p.w * (1.0f / 256.0f);
        float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int oy = -3; oy <= 3; ++oy) {
            const float ry = gy * (float)(oy < 0 ? -oy : oy);
#pragma unroll
            for (int ox = -3; ox <= 3; ++ox) {
                const int i = c + oy * kVarWinX + ox;
                const float4 n_q = s_n[i];
                if (!(n_q.w == n_q.w)) continue;   // not live, or outside the image
                const float w = det_expf(-tap_exponent(l.kn, l.ka, l.sigma_depth, n_p, a_p, n_q, s_a[i], gx * (float)(ox < 0 ? -ox : ox) + ry, zfloor));
                const float lum = s_l[i];
                sw = sw + w;
                s1 = s1 + w * lum;
                s2 = s2 + w * (lum * lum);
            }
        }
        const float m1 = s1 / sw, m2 = s2 / sw;
        v0 = fmax_c(0.0f, m2 - m1 * m1);
    } else {
        v0 = var_value(q.variance[p]) / ym2;
    }
    q.pack_w[(2 * px + p) * 4 + 3] = v0;
    if (q.out_variance) q.out_variance[p] = var_value(v0 * ym2);
}

// ---- V3 ----
VRT_DEV float g3(int oy, int ox) { return (oy == 0 && ox == 0) ? 0.25f : ((oy == 0 || ox == 0) ? 0.125f : 0.0625f); }

// sl of V3 from the 3 x 3's two sums. __builtin_sqrtf, as vrt_common.hip.h's len3: under this build's flags it is the correctly
// rounded root (the refinement around v_sqrt_f32); this toolchain's __fsqrt_rn is the bare instruction, an ulp off now and then.
VRT_DEV float lum_width(float sigma_lum, float gv, float gs) { return sigma_lum * __builtin_sqrtf(gv / gs) + 0x1p-20f; }

// a pixel that is not live: h(c) and a variance of +0, from the last level only
template <bool LAST>
VRT_DEV void pass_through_var(const LevelVar &q, size_t p) {
    pass_through<LAST>(q.l, p);
    if (LAST && q.out_variance) q.out_variance[p] = 0.0f;
}

// u' and v' into the next level's image, or (V4) into the outputs
template <bool LAST>
VRT_DEV void finish_pixel_var(const LevelVar &q, size_t p, const float sum[3], float sumw, float sumv, const float4 &a_p, float cov) {
    const float v = sumv / (sumw * sumw);
    if (LAST) {
        finish_pixel<true>(q.l, p, sum, sumw, a_p, cov);
        if (q.out_variance) q.out_variance[p] = var_value(v * modulation_lum2(q.l, a_p, cov));
    } else {
        q.l.dst[p] = make_float4(sum[0] / sumw, sum[1] / sumw, sum[2] / sumw, v);
    }
}

// The lattice form (vrt_filter.hip.h): the 3 x 3 of the smoothed variance runs on the same staged lattice
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kLatX *kLatY) void filter_var_level_lattice_kernel(const LevelVar q) {
    __shared__ float4 s_n[kWinX * kWinY], s_a[kWinX * kWinY], s_u[kWinX * kWinY];
    const Level &l = q.l;
    const int s = l.step;
    const int rx = (int)(blockIdx.x % (unsigned)s), ry = (int)(blockIdx.y % (unsigned)s);
    const int lx0 = (int)(blockIdx.x / (unsigned)s) * kLatX, ly0 = (int)(blockIdx.y / (unsigned)s) * kLatY;
    if (rx + s * lx0 >= l.width || ry + s * ly0 >= l.height) return;   // the whole workgroup: this class has fewer tiles
    const size_t px = (size_t)l.width * (size_t)l.height;
    for (int i = (int)(threadIdx.y * kLatX + threadIdx.x); i < kWinX * kWinY; i += kLatX * kLatY) {
        const int wy = i / kWinX, wx = i - wy * kWinX;
        const int x = rx + s * (lx0 - 2 + wx), y = ry + s * (ly0 - 2 + wy);
        float4 n = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x7fc00000u)), a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), u = a;
        if (x >= 0 && x < l.width && y >= 0 && y < l.height) {
            const size_t t = (size_t)y * (size_t)l.width + (size_t)x;
            n = l.pack[t];
            if (n.w == n.w) {
                a = l.pack[px + t];
                if (FIRST) {
                    u = first_colour(l, px, t, a);
                    u.w = l.pack[2 * px + t].w;   // V2's, from filter_variance_kernel
                } else {
                    u = l.src[t];
                }
            }
        }
        s_n[i] = n;
        s_a[i] = a;
        s_u[i] = u;
    }
    __syncthreads();
    const int x = rx + s * (lx0 + (int)threadIdx.x), y = ry + s * (ly0 + (int)threadIdx.y);
    if (x >= l.width || y >= l.height) return;
    const size_t p = (size_t)y * (size_t)l.width + (size_t)x;
    const int c = ((int)threadIdx.y + 2) * kWinX + (int)threadIdx.x + 2;
    const float4 n_p = s_n[c];
    if (!(n_p.w == n_p.w)) return pass_through_var<LAST>(q, p);
    const float4 a_p = s_a[c], c_p = l.pack[2 * px + p], u_p = s_u[c];
    const float gx = c_p.x, gy = c_p.y;
    const float zfloor = n_p.w * (1.0f / 256.0f);
    float gs = 0.0f, gv = 0.0f;
#pragma unroll
    for (int oy = -1; oy <= 1; ++oy) {
#pragma unroll
        for (int ox = -1; ox <= 1; ++ox) {
            const int i = c + oy * kWinX + ox;
            const float nw = s_n[i].w;
            if (!(nw == nw)) continue;
            gs = gs + g3(oy, ox);
            gv = gv + g3(oy, ox) * s_u[i].w;
        }
    }
    const float sl = lum_width(q.sigma_lum, gv, gs);
    const float y_p = luminance(u_p.x, u_p.y, u_p.z);
    float sumw = 0.0f, sumv = 0.0f, sum[3] = {0.0f, 0.0f, 0.0f};
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
            const float4 u = s_u[i];
            const float dl = __builtin_fabsf(luminance(u.x, u.y, u.z) - y_p);
            const float e = tap_exponent(l.kn, l.ka, l.sigma_depth, n_p, a_p, n_q, s_a[i], gx * (float)(ax * s) + ry_, zfloor) + dl / sl;
            const float w = (b3(ay) * b3(ax)) * det_expf(-e);
            sumw = sumw + w;
            sum[0] = sum[0] + w * u.x;
            sum[1] = sum[1] + w * u.y;
            sum[2] = sum[2] + w * u.z;
            sumv = sumv + (w * w) * u.w;
        }
    }
    finish_pixel_var<LAST>(q, p, sum, sumw, sumv, a_p, c_p.z);
}

// The gather form (vrt_filter.hip.h). Never the first level.
template <bool LAST>
__global__ __launch_bounds__(kBlockX *kBlockY) void filter_var_level_kernel(const LevelVar q) {
    const Level &l = q.l;
    const int x = (int)(blockIdx.x * kBlockX + threadIdx.x), y = (int)(blockIdx.y * kBlockY + threadIdx.y);
    if (x >= l.width || y >= l.height) return;
    const size_t px = (size_t)l.width * (size_t)l.height, p = (size_t)y * (size_t)l.width + (size_t)x;
    const float4 n_p = l.pack[p];
    if (!(n_p.w == n_p.w)) return pass_through_var<LAST>(q, p);
    const float4 a_p = l.pack[px + p], c_p = l.pack[2 * px + p], u_p = l.src[p];
    const float gx = c_p.x, gy = c_p.y;
    const float zfloor = n_p.w * (1.0f / 256.0f);
    const int s = l.step;
    float gs = 0.0f, gv = 0.0f;
#pragma unroll
    for (int oy = -1; oy <= 1; ++oy) {
        const int ty = y + oy * s;
        if (ty < 0 || ty >= l.height) continue;
#pragma unroll
        for (int ox = -1; ox <= 1; ++ox) {
            const int tx = x + ox * s;
            if (tx < 0 || tx >= l.width) continue;
            const size_t t = (size_t)ty * (size_t)l.width + (size_t)tx;
            const float nw = l.pack[t].w;
            if (!(nw == nw)) continue;
            gs = gs + g3(oy, ox);
            gv = gv + g3(oy, ox) * l.src[t].w;
        }
    }
    const float sl = lum_width(q.sigma_lum, gv, gs);
    const float y_p = luminance(u_p.x, u_p.y, u_p.z);
    float sumw = 0.0f, sumv = 0.0f, sum[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int oy = -2; oy <= 2; ++oy) {
        const int ty = y + oy * s;
        if (ty < 0 || ty >= l.height) continue;
        const int ay = oy < 0 ? -oy : oy;
        const float ry = gy * (float)(ay * s);
#pragma unroll
        for (int ox = -2; ox <= 2; ++ox) {
            const int tx = x + ox * s;
            if (tx < 0 || tx >= l.width) continue;
            const size_t t = (size_t)ty * (size_t)l.width + (size_t)tx;
            const float4 n_q = l.pack[t];
            if (!(n_q.w == n_q.w)) continue;
            const float4 a_q = l.pack[px + t];
            const int ax = ox < 0 ? -ox : ox;
            const float4 u = l.src[t];
            const float dl = __builtin_fabsf(luminance(u.x, u.y, u.z) - y_p);
            const float e = tap_exponent(l.kn, l.ka, l.sigma_depth, n_p, a_p, n_q, a_q, gx * (float)(ax * s) + ry, zfloor) + dl / sl;
            const float w = (b3(ay) * b3(ax)) * det_expf(-e);
            sumw = sumw + w;
            sum[0] = sum[0] + w * u.x;
            sum[1] = sum[1] + w * u.y;
            sum[2] = sum[2] + w * u.z;
            sumv = sumv + (w * w) * u.w;
        }
    }
    finish_pixel_var<LAST>(q, p, sum, sumw, sumv, a_p, c_p.z);
}

}  // namespace filter
}  // namespace vrt
