// vrt_upsample.hip.h -- the guided upsampling pass (include/vrt.h vrt_upsample_hdr, points U1-U6): a float image traced at 1 / r of
// the resolution rebuilt at full size from its four bilinear taps, each weighed by how well the tap's LOW guides agree with the
// pixel's HIGH guides, on the albedo-divided image, with a byte per pixel that says where no tap counted.
// One lane per HIGH pixel, one 8 x 8 tile per wave, four tiles side by side per workgroup, as temporal_kernel. The high guides come
// first, then the four taps. r is a kernel argument, the same in every lane.
// The workgroup's window of the low image -- the taps of its 32 x 8 high pixels, (32 / r + 2) x (8 / r + 2) low pixels -- is staged
// in LDS once, as three 16-byte words per low pixel: g() of the guides and u = h(c) / m are evaluated once per low pixel, not once
// per tap (at r = 2 a low pixel is a tap of about sixteen high pixels), and a tap is three LDS reads. fx is monotone in x, so the
// window's corners are the floors of the first and last lane's position. A window larger than kWinX x kWinY (none is, for the r
// and offsets the host admits) sends the whole workgroup down the path that reads every tap from memory, its coverage first, the
// rest only where the tap counts: the same operations on the same values in the same order, the same bits. That path as a kernel
// of its own was measured against this one and lost (profiles/upsample_ab.txt). No scratch (profiles/upsample_resource_usage.txt).
// Every expression is the header's, operation by operation; tests/oracle_upsample.c restates them.
#pragma once
#include "vrt_hdr.hip.h"
#include "vrt_upsample.h"

namespace vrt {
namespace upsample {

constexpr int kTile = 8, kWaves = 4;   // a workgroup: four tiles side by side
// the staged window: x0 of the last lane minus x0 of the first is at most 31 / r + 1, and the taps reach one further
constexpr int kWinX = kTile * kWaves + 2, kWinY = kTile + 2;

// g and m of include/vrt.h vrt_filter_hdr points 1 and 2, as vrt_filter.hip.h has them
VRT_DEV float guide_value(float v) { return v != v ? 0.0f : fmin_c(fmax_c(-accum::kHdrMax, v), accum::kHdrMax); }
VRT_DEV float modulation(float albedo, float coverage) { return fmax_c(albedo + (1.0f - coverage), 1.0f / 255.0f); }

// point 3 on the high planes: the smaller |Z_n - Z_p| over the two neighbours `stride` floats either side of p that exist (lo / hi)
// and are live; 0 if none
VRT_DEV float depth_slope(const Args &q, size_t p, size_t stride, bool lo, bool hi, float zp) {
    float s = 0.0f;
    bool have = false;
    if (lo && guide_value(q.hi_coverage[p - stride]) > 0.0f) {
        s = __builtin_fabsf(guide_value(q.hi_depth[p - stride]) - zp);
        have = true;
    }
    if (hi && guide_value(q.hi_coverage[p + stride]) > 0.0f) {
        const float d = __builtin_fabsf(guide_value(q.hi_depth[p + stride]) - zp);
        s = have ? fmin_c(s, d) : d;
    }
    return s;
}

// A low pixel as a tap reads it: {u, g(coverage)}, {g(normal), g(depth)}, g(albedo). u (U2): h(c) / m with the pixel's own albedo and
// coverage where it is live and the flag is set, else h(c). The guides of a pixel that is not live are never read: zeros.
struct LowPixel {
    float4 c, n, a;
};
VRT_DEV float4 low_colour(const Args &q, size_t t, bool live, float cov, const float4 &a) {
    float4 u = make_float4(accum::hdr_value(q.rgb[t * 3 + 0]), accum::hdr_value(q.rgb[t * 3 + 1]), accum::hdr_value(q.rgb[t * 3 + 2]), cov);
    if (q.demodulate && live) {
        u.x = u.x / modulation(a.x, cov);
        u.y = u.y / modulation(a.y, cov);
        u.z = u.z / modulation(a.z, cov);
    }
    return u;
}
VRT_DEV float4 low_albedo(const Args &q, size_t t) {
    return make_float4(guide_value(q.albedo[t * 4 + 0]), guide_value(q.albedo[t * 4 + 1]), guide_value(q.albedo[t * 4 + 2]),
                       guide_value(q.albedo[t * 4 + 3]));
}
VRT_DEV float4 low_normal_depth(const Args &q, size_t t) {
    return make_float4(guide_value(q.normal[t * 3 + 0]), guide_value(q.normal[t * 3 + 1]), guide_value(q.normal[t * 3 + 2]),
                       guide_value(q.depth[t]));
}

// a tap from memory: the coverage first (the staging loop, and the fallback)
struct FromMemory {
    const Args &q;
    VRT_DEV float coverage(int qx, int qy) const { return guide_value(q.coverage[(size_t)qy * (size_t)q.width + (size_t)qx]); }
    // the rest of a tap whose coverage is cov; guides: whether n and the albedo's alpha are read at all
    VRT_DEV LowPixel rest(int qx, int qy, float cov, bool guides) const {
        const size_t t = (size_t)qy * (size_t)q.width + (size_t)qx;
        const bool live = cov > 0.0f;
        LowPixel l;
        l.a = (live && (guides || q.demodulate)) ? low_albedo(q, t) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        l.n = (live && guides) ? low_normal_depth(q, t) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        l.c = low_colour(q, t, live, cov, l.a);
        return l;
    }
};

// a tap from the workgroup's window
struct FromWindow {
    const float4 *s_c, *s_n, *s_a;
    int wx0, wy0, win_w;
    VRT_DEV int at(int qx, int qy) const { return (qy - wy0) * win_w + (qx - wx0); }
    VRT_DEV float coverage(int qx, int qy) const { return s_c[at(qx, qy)].w; }
    VRT_DEV LowPixel rest(int qx, int qy, float, bool) const {
        const int i = at(qx, qy);
        return LowPixel{s_c[i], s_n[i], s_a[i]};
    }
};

// U1-U6 for the high pixel (x, y) with its taps from `low`
template <class LOW>
VRT_DEV void upsample_pixel(const Args &q, const LOW &low, int x, int y, int hw, int hh) {
    const size_t p = (size_t)y * (size_t)hw + (size_t)x;
    const float rf = (float)q.factor;
    // U1, U2: the high pixel
    const float cov_p = guide_value(q.hi_coverage[p]);
    const bool live_p = cov_p > 0.0f;
    float n_p[3] = {0.0f, 0.0f, 0.0f}, a_p[4] = {0.0f, 0.0f, 0.0f, 0.0f}, z_p = 0.0f, gx = 0.0f, gy = 0.0f;
    float m_p[3] = {1.0f, 1.0f, 1.0f};
    if (live_p) {
#pragma unroll
        for (int k = 0; k < 3; ++k) n_p[k] = guide_value(q.hi_normal[p * 3 + k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) a_p[k] = guide_value(q.hi_albedo[p * 4 + k]);
        z_p = guide_value(q.hi_depth[p]);
        gx = depth_slope(q, p, 1, x > 0, x + 1 < hw, z_p);
        gy = depth_slope(q, p, (size_t)hw, y > 0, y + 1 < hh, z_p);
        if (q.demodulate) {
#pragma unroll
            for (int k = 0; k < 3; ++k) m_p[k] = modulation(a_p[k], cov_p);
        }
    }
    // U3
    const float fx = ((float)x + q.offset_hi_x) / rf - q.offset_lo_x;
    const float fy = ((float)y + q.offset_hi_y) / rf - q.offset_lo_y;
    const float xf = __builtin_floorf(fx), yf = __builtin_floorf(fy);
    const float tx = fx - xf, ty = fy - yf;
    const int x0 = (int)xf, y0 = (int)yf;
    const float zfloor = z_p * (1.0f / 256.0f);
    // U4
    float sumw = 0.0f, sum[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
        if (qx < 0 || qx >= q.width || qy < 0 || qy >= q.height) continue;
        const float cov_q = low.coverage(qx, qy);
        if ((cov_q > 0.0f) != live_p) continue;
        const LowPixel l = low.rest(qx, qy, cov_q, live_p);
        const float b = ((k & 1) ? tx : 1.0f - tx) * ((k >> 1) ? ty : 1.0f - ty);
        float w = b;
        if (live_p) {
            const float dx = l.n.x - n_p[0], dy = l.n.y - n_p[1], dz = l.n.z - n_p[2];
            const float dn2 = (dx * dx + dy * dy) + dz * dz;
            const float a0 = l.a.x - a_p[0], a1 = l.a.y - a_p[1], a2 = l.a.z - a_p[2], a3 = l.a.w - a_p[3];
            const float da2 = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
            const float dzq = __builtin_fabsf(l.n.w - z_p);
            const float ddx = __builtin_fabsf((float)qx - fx) * rf, ddy = __builtin_fabsf((float)qy - fy) * rf;
            const float den = q.sigma_depth * ((gx * ddx + gy * ddy) + zfloor) + 0x1p-20f;
            const float e = (dn2 * q.kn + da2 * q.ka) + dzq / den;
            w = b * det_expf(-e);
        }
        sumw = sumw + w;
        sum[0] = sum[0] + w * l.c.x;
        sum[1] = sum[1] + w * l.c.y;
        sum[2] = sum[2] + w * l.c.z;
    }
    // U5
    float up[3];
    const bool resolved = sumw > q.min_weight;
    if (resolved) {
        up[0] = sum[0] / sumw;
        up[1] = sum[1] / sumw;
        up[2] = sum[2] / sumw;
    } else {   // rare and divergent: the nearest low pixel, whatever its liveness
        int nx = (int)__builtin_floorf(fx + 0.5f), ny = (int)__builtin_floorf(fy + 0.5f);
        nx = nx < 0 ? 0 : (nx > q.width - 1 ? q.width - 1 : nx);
        ny = ny < 0 ? 0 : (ny > q.height - 1 ? q.height - 1 : ny);
        const float4 u = low.rest(nx, ny, low.coverage(nx, ny), false).c;
        up[0] = u.x;
        up[1] = u.y;
        up[2] = u.z;
    }
    // U6
    const float f[3] = {accum::hdr_value(up[0] * m_p[0]), accum::hdr_value(up[1] * m_p[1]), accum::hdr_value(up[2] * m_p[2])};
    if (q.out_rgb) { q.out_rgb[p * 3 + 0] = f[0]; q.out_rgb[p * 3 + 1] = f[1]; q.out_rgb[p * 3 + 2] = f[2]; }
    if (q.out_rgba)
        q.out_rgba[p] = unorm8(accum::tone_map(f[0], q.op, q.exposure)) | (unorm8(accum::tone_map(f[1], q.op, q.exposure)) << 8) |
                        (unorm8(accum::tone_map(f[2], q.op, q.exposure)) << 16) | (255u << 24);
    if (q.out_unresolved) q.out_unresolved[p] = resolved ? (uint8_t)0 : (uint8_t)1;
}

// x0 of U3 for the high coordinate v, clamped into the low image: monotone in v
VRT_DEV int low_coord(int v, float offset_hi, float rf, float offset_lo, int add, int size) {
    const int c = (int)__builtin_floorf(((float)v + offset_hi) / rf - offset_lo) + add;
    return c < 0 ? 0 : (c > size - 1 ? size - 1 : c);
}

__global__ __launch_bounds__(64 * kWaves) void upsample_kernel(const Args q) {
    const int hw = q.width * q.factor, hh = q.height * q.factor;
    const int x = (int)(blockIdx.x * kWaves + threadIdx.y) * kTile + (int)(threadIdx.x & 7u);
    const int y = (int)blockIdx.y * kTile + (int)(threadIdx.x >> 3);
    const bool inside = x < hw && y < hh;
    {
        __shared__ float4 s_c[kWinX * kWinY], s_n[kWinX * kWinY], s_a[kWinX * kWinY];
        // the window: the taps, and the nearest pixels, of the workgroup's first and last pixel inside the frame -- the same in every lane
        const float rf = (float)q.factor;
        const int xa = (int)blockIdx.x * kWaves * kTile, ya = (int)blockIdx.y * kTile;
        const int xb = xa + kWaves * kTile - 1 < hw - 1 ? xa + kWaves * kTile - 1 : hw - 1;
        const int yb = ya + kTile - 1 < hh - 1 ? ya + kTile - 1 : hh - 1;
        const int wx0 = low_coord(xa, q.offset_hi_x, rf, q.offset_lo_x, 0, q.width), wx1 = low_coord(xb, q.offset_hi_x, rf, q.offset_lo_x, 1, q.width);
        const int wy0 = low_coord(ya, q.offset_hi_y, rf, q.offset_lo_y, 0, q.height), wy1 = low_coord(yb, q.offset_hi_y, rf, q.offset_lo_y, 1, q.height);
        const int win_w = wx1 - wx0 + 1, win_h = wy1 - wy0 + 1;
        if (win_w <= kWinX && win_h <= kWinY) {
            for (int i = (int)(threadIdx.y * 64u + threadIdx.x); i < win_w * win_h; i += 64 * kWaves) {
                const int wy = i / win_w, wx = i - wy * win_w;
                const FromMemory m{q};
                const float cov = m.coverage(wx0 + wx, wy0 + wy);
                const LowPixel l = m.rest(wx0 + wx, wy0 + wy, cov, true);
                s_c[i] = l.c;
                s_n[i] = l.n;
                s_a[i] = l.a;
            }
            __syncthreads();
            if (inside) upsample_pixel(q, FromWindow{s_c, s_n, s_a, wx0, wy0, win_w}, x, y, hw, hh);
            return;
        }
    }
    if (inside) upsample_pixel(q, FromMemory{q}, x, y, hw, hh);
}

}  // namespace upsample
}  // namespace vrt
