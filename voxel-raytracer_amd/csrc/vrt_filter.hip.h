// vrt_filter.hip.h -- the guided filter (include/vrt.h vrt_filter_hdr, points 1-5) and its variance-guided form (vrt_filter_hdr_var,
// points V1-V4): an edge-avoiding a-trous filter on a float image, its edge weights from the guide planes and, in the
// variance-guided form, from a luminance term whose width is the pixel's own variance, carried through the levels. One lane per
// pixel in every kernel:
//   filter_prepass_kernel         g() of the guides, the live bit and the centre's depth slopes into the packed planes (vrt_filter.h)
//   filter_variance_kernel        V2: the initial variance of every live pixel into the packed planes -- SPATIAL: the 7 x 7
//                                 guide-weighted estimate from a window staged in LDS; otherwise the caller's plane, demodulated
//   filter_level_lattice_kernel   one level's 25 taps from a window staged in LDS: the levels of step 1, 2 and 4. FIRST reads the
//                                 caller's image as h(c) / m
//   filter_level_kernel           one level's 25 taps gathered from memory: the levels of step 8 and above
//   filter_through_kernel         levels == 0
// The two level kernels are templates on their argument struct: Level is the guide-only filter, LevelVar the variance-guided one,
// whose parts stand behind the compile-time kVar<Q>. Every instantiation keeps its own kernarg segment and, instruction for
// instruction, the code it had while the variance-guided levels were kernels of their own (profiles/filter_fold_codegen.txt). The
// variance rides in words the guide-only filter leaves unused (vrt_filter.h), so a level stages the same 20,736 bytes of LDS in
// either form.
// Either level kernel's LAST form remodulates, clamps, tone-maps and stores the outputs: no extra pass over the image at either
// end. Which form serves which step is what was measured (profiles/filter_levels_ab.txt, profiles/filter_var_levels_ab.txt). In both
// the sum order is the lane's own loop order over the same values, so the bits do not depend on the form or the launch shape. Every
// expression is the header's, operation by operation; tests/oracle_filter_hdr.c and tests/oracle_filter_var.c restate them.
#pragma once
#include <type_traits>

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

// e of one tap from the guides (point 4): n_* = normal and depth, a_* = albedo of the centre p and the tap q,
// slope = gx * |ox| s + gy * |oy| s, zfloor = Z_p / 256. V3 adds its own term to it.
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

// ---- the variance-guided form's own pieces ----
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

// V2. A workgroup owns a kVarX x kVarY tile; its 49 taps at step 1 are dense, so a (kVarX + 6) x (kVarY + 6) window serves the tile: the
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

// V3's 3 x 3 weights
VRT_DEV float g3(int oy, int ox) { return (oy == 0 && ox == 0) ? 0.25f : ((oy == 0 || ox == 0) ? 0.125f : 0.0625f); }

// sl of V3 from the 3 x 3's two sums. __builtin_sqrtf, as vrt_common.hip.h's len3: under this build's flags it is the correctly
// rounded root (the refinement around v_sqrt_f32); this toolchain's __fsqrt_rn is the bare instruction, an ulp off now and then.
VRT_DEV float lum_width(float sigma_lum, float gv, float gs) { return sigma_lum * __builtin_sqrtf(gv / gs) + 0x1p-20f; }

// ---- one level, in either form ----
template <class Q>
constexpr bool kVar = std::is_same<Q, LevelVar>::value;

// w of one tap (point 4): b = B[|oy|] * B[|ox|]; with VAR the exponent has V3's term dl / sl as well (dl = |Y(u) - Y(u_p)|, sl: the
// width from the centre's 3 x 3)
template <bool VAR>
VRT_DEV float tap_weight(const Level &l, const float4 &n_p, const float4 &a_p, const float4 &n_q, const float4 &a_q, float slope, float zfloor,
                         float b, float dl, float sl) {
    float e = tap_exponent(l.kn, l.ka, l.sigma_depth, n_p, a_p, n_q, a_q, slope, zfloor);
    if (VAR) e = e + dl / sl;
    return b * det_expf(-e);
}

// a pixel that is not live: h(c) and, with VAR, a variance of +0, from the last level only (no level reads it as a tap)
template <bool LAST, class Q>
VRT_DEV void pass_through(const Q &q, size_t p) {
    if (LAST) {
        const Level &l = level_of(q);
        const float f[3] = {accum::hdr_value(l.rgb[p * 3 + 0]), accum::hdr_value(l.rgb[p * 3 + 1]), accum::hdr_value(l.rgb[p * 3 + 2])};
        store_pixel(l.out_rgb, l.out_rgba, p, f, l.op, l.exposure);
        if constexpr (kVar<Q>)
            if (q.out_variance) q.out_variance[p] = 0.0f;
    }
}

// u' = sum / sumw (point 5) remodulated, clamped and tone-mapped into the outputs
VRT_DEV void store_final(const Level &l, size_t p, const float sum[3], float sumw, const float4 &a_p, float cov) {
    const float r[3] = {sum[0] / sumw, sum[1] / sumw, sum[2] / sumw};
    float m[3] = {1.0f, 1.0f, 1.0f};
    if (l.demodulate) { m[0] = modulation(a_p.x, cov); m[1] = modulation(a_p.y, cov); m[2] = modulation(a_p.z, cov); }
    const float f[3] = {accum::hdr_value(r[0] * m[0]), accum::hdr_value(r[1] * m[1]), accum::hdr_value(r[2] * m[2])};
    store_pixel(l.out_rgb, l.out_rgba, p, f, l.op, l.exposure);
}

// u' and, with VAR, v' = sumv / sumw^2 into the next level's image, or (V4) into the outputs
template <bool LAST, class Q>
VRT_DEV void finish_pixel(const Q &q, size_t p, const float sum[3], float sumw, float sumv, const float4 &a_p, float cov) {
    const Level &l = level_of(q);
    float v = 0.0f;
    if (kVar<Q>) v = sumv / (sumw * sumw);
    if (LAST) {
        store_final(l, p, sum, sumw, a_p, cov);
        if constexpr (kVar<Q>)
            if (q.out_variance) q.out_variance[p] = var_value(v * modulation_lum2(l, a_p, cov));
    } else {
        l.dst[p] = make_float4(sum[0] / sumw, sum[1] / sumw, sum[2] / sumw, v);
    }
}

// The gather form: tap (ox, oy) of every lane of a wave lies s * ox pixels along the same row, so each of a tap's loads moves 64
// adjacent 16-byte words whatever the step. Never the first level (step 1 takes the lattice form).
template <class Q, bool LAST>
__global__ __launch_bounds__(kBlockX *kBlockY) void filter_level_kernel(const Q q) {
    constexpr bool VAR = kVar<Q>;
    const Level &l = level_of(q);
    const int x = (int)(blockIdx.x * kBlockX + threadIdx.x), y = (int)(blockIdx.y * kBlockY + threadIdx.y);
    if (x >= l.width || y >= l.height) return;
    const size_t px = (size_t)l.width * (size_t)l.height, p = (size_t)y * (size_t)l.width + (size_t)x;
    const float4 n_p = l.pack[p];
    if (!(n_p.w == n_p.w)) return pass_through<LAST>(q, p);
    const float4 a_p = l.pack[px + p], c_p = l.pack[2 * px + p];
    float4 u_p;
    if (VAR) u_p = l.src[p];   // beside a_p and c_p: the schedule follows this order
    const float gx = c_p.x, gy = c_p.y;
    const float zfloor = n_p.w * (1.0f / 256.0f);
    const int s = l.step;
    float sl = 0.0f, y_p = 0.0f;
    if constexpr (VAR) {   // V3: the smoothed variance of the centre's 3 x 3, in the bounds of the taps below
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
        sl = lum_width(q.sigma_lum, gv, gs);
        y_p = luminance(u_p.x, u_p.y, u_p.z);
    }
    // the sums stay plain locals of the kernel (sumv: V3's, with VAR only): handed to a helper by reference they are promoted to
    // registers in another order, and the variance-guided kernels come out with other registers
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
            float4 u;
            float dl = 0.0f;
            if (VAR) {   // the colour and V3's |Y(u) - Y(u_p)| before the guides' exponent: the schedule follows this order
                u = l.src[t];
                dl = __builtin_fabsf(luminance(u.x, u.y, u.z) - y_p);
            }
            const float w = tap_weight<VAR>(l, n_p, a_p, n_q, a_q, gx * (float)(ax * s) + ry, zfloor, b3(ay) * b3(ax), dl, sl);
            if (!VAR) u = l.src[t];   // the colour after the weight: the schedule follows this order
            sumw = sumw + w;
            sum[0] = sum[0] + w * u.x;
            sum[1] = sum[1] + w * u.y;
            sum[2] = sum[2] + w * u.z;
            if (VAR) sumv = sumv + (w * w) * u.w;
        }
    }
    finish_pixel<LAST>(q, p, sum, sumw, sumv, a_p, c_p.z);
}

// The lattice form: the same level with its taps staged in LDS. At step s a workgroup owns a kLatX x kLatY tile of ONE residue class (x mod s, y mod s):
// in that class's own lattice the 25 taps are dense, so a (kLatX + 4) x (kLatY + 4) window of packed words and colours serves the
// whole tile -- 1.7 loads per pixel and plane instead of 25 -- and the first level's h(c) / m is evaluated once per staged pixel.
// The residue is the fastest-varying part of the block index: the s workgroups whose lanes share cache lines are dispatched together.
// A word outside the image is staged as not live. The sums run in the same order over the same values: the same bits. A lane's
// loads and stores lie s words apart, which is what the form pays: it wins up to step 4 and loses from step 8 on.
constexpr int kLatX = 32, kLatY = 8, kWinX = kLatX + 4, kWinY = kLatY + 4;
constexpr int kLatticeMaxStep = 4;   // the lattice form up to this step, the gather form above it (vrt_launch_filter.hip)

template <class Q, bool FIRST, bool LAST>
__global__ __launch_bounds__(kLatX *kLatY) void filter_level_lattice_kernel(const Q q) {
    constexpr bool VAR = kVar<Q>;
    __shared__ float4 s_n[kWinX * kWinY], s_a[kWinX * kWinY], s_u[kWinX * kWinY];
    const Level &l = level_of(q);
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
                    if (VAR) u.w = l.pack[2 * px + t].w;   // V2's, from filter_variance_kernel
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
    if (!(n_p.w == n_p.w)) return pass_through<LAST>(q, p);
    const float4 a_p = s_a[c], c_p = l.pack[2 * px + p];
    float4 u_p;
    if (VAR) u_p = s_u[c];   // beside a_p and c_p: the schedule follows this order
    const float gx = c_p.x, gy = c_p.y;
    const float zfloor = n_p.w * (1.0f / 256.0f);
    float gs = 0.0f, gv = 0.0f;   // V3's two sums, declared out here: the register assignment follows it
    float sl = 0.0f, y_p = 0.0f;
    if constexpr (VAR) {   // V3: the smoothed variance of the centre's 3 x 3, on the same staged lattice
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
        sl = lum_width(q.sigma_lum, gv, gs);
        y_p = luminance(u_p.x, u_p.y, u_p.z);
    }
    float sumw = 0.0f, sumv = 0.0f, sum[3] = {0.0f, 0.0f, 0.0f};   // plain locals, as in the gather form
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
            float4 u;
            float dl = 0.0f;
            if (VAR) {   // the colour and V3's |Y(u) - Y(u_p)| before the guides' exponent: the schedule follows this order
                u = s_u[i];
                dl = __builtin_fabsf(luminance(u.x, u.y, u.z) - y_p);
            }
            const float w = tap_weight<VAR>(l, n_p, a_p, n_q, s_a[i], gx * (float)(ax * s) + ry_, zfloor, b3(ay) * b3(ax), dl, sl);
            if (!VAR) u = s_u[i];   // the colour after the weight: the schedule follows this order
            sumw = sumw + w;
            sum[0] = sum[0] + w * u.x;
            sum[1] = sum[1] + w * u.y;
            sum[2] = sum[2] + w * u.z;
            if (VAR) sumv = sumv + (w * w) * u.w;
        }
    }
    finish_pixel<LAST>(q, p, sum, sumw, sumv, a_p, c_p.z);
}

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

}  // namespace filter
}  // namespace vrt
