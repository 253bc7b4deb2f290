// vrt_temporal.hip.h -- the temporal pass (include/vrt.h vrt_temporal_hdr, points T1-T6): the previous frame's integrated colour and
// luminance moments reprojected into this frame through the guide planes, each of the four bilinear taps tested against this
// pixel's normal and the depth the previous camera saw its world point at, blended with this frame's image, and the variance of the
// integrated mean for vrt_filter_hdr_var.
// One lane per pixel, one 8 x 8 tile per wave: a wave's taps fall in a compact window of the previous frame (camera motion moves a
// tile's pixels together), and its stores are rows of eight adjacent 16-byte words. The taps are gathered from memory, 16 bytes a
// load; a tap's guide words (planes 1 and 2) come first and its colour word (plane 0) only where the tap counts, so a wave whose
// taps all fail never loads a colour. No LDS, no barrier, no scratch (profiles/temporal_resource_usage.txt).
// Every expression is the header's, operation by operation; tests/oracle_temporal.c restates them.
// The kernel has two compile-time forms, chosen by its argument type. Args is vrt_temporal_hdr's. ArgsMom is vrt_temporal_hdr_mom's
// (T3s, T7, T6m; tests/oracle_temporal_mom.c): the measured variance V rides in plane 2's fourth float, which every tap's guide load
// brings anyway, and the 3 x 3 search is one rolled loop behind the sw == 0 branch that keeps running sums and no per-tap values.
// Everything the second form adds is behind `if constexpr`: the first compiles to the instructions it had
// (profiles/temporal_mom_codegen.txt).
#pragma once
#include <type_traits>

#include "vrt_hdr.hip.h"
#include "vrt_temporal.h"

namespace vrt {
namespace temporal {

constexpr int kTile = 8, kWaves = 4;   // a workgroup: four tiles side by side

// g, hv and V1 of include/vrt.h vrt_filter_hdr / vrt_filter_hdr_var, as vrt_filter.hip.h has them
VRT_DEV float guide_value(float v) { return v != v ? 0.0f : fmin_c(fmax_c(-accum::kHdrMax, v), accum::kHdrMax); }
constexpr float kVarMax = 65504.0f * 65504.0f;
VRT_DEV float var_value(float v) { return fmin_c(fmax_c(0.0f, v), kVarMax); }
VRT_DEV float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// shader_ray_dir() of vrt_common.hip.h on the pass's own camera block, then primary_ray_dir()'s general form: the direction
// pathTrace marches for a ray through (fx, fy)
VRT_DEV F3 ray_dir(const Args &q, float fx, float fy) {
    const float u = (fx / (float)q.width) * 2.0f - 1.0f;
    const float v = (fy / (float)q.height) * 2.0f - 1.0f;
    float view[4];
    mat_vec(q.inv_proj, u, v, -1.0f, 1.0f, view);
    if (__builtin_fabsf(view[3]) > 1e-6f) { const float w = view[3]; view[0] = view[0] / w; view[1] = view[1] / w; view[2] = view[2] / w; }
    const F3 vd = normalize3(F3{view[0], view[1], view[2]});
    float wd4[4];
    mat_vec(q.inv_view, vd.x, vd.y, vd.z, 0.0f, wd4);
    const F3 d = normalize3(F3{wd4[0], wd4[1], wd4[2]});
    return scale3(d, 1.0f / __builtin_sqrtf(dot3(d, d)));
}

// (sum of w * Xq) / sw of T3 over the counted taps, in tap order
VRT_DEV float previous(const bool ok[4], const float w[4], float x0, float x1, float x2, float x3, float sw) {
    float s = 0.0f;
    if (ok[0]) s = s + w[0] * x0;
    if (ok[1]) s = s + w[1] * x1;
    if (ok[2]) s = s + w[2] * x2;
    if (ok[3]) s = s + w[3] * x3;
    return s / sw;
}

template <class A>
__global__ __launch_bounds__(64 * kWaves) void temporal_kernel(const A q) {
    constexpr bool kMom = std::is_same<A, ArgsMom>::value;
    const int x = (int)(blockIdx.x * kWaves + threadIdx.y) * kTile + (int)(threadIdx.x & 7u);
    const int y = (int)blockIdx.y * kTile + (int)(threadIdx.x >> 3);
    if (x >= q.width || y >= q.height) return;
    const size_t px = (size_t)q.width * (size_t)q.height, p = (size_t)y * (size_t)q.width + (size_t)x;
    const float c[3] = {accum::hdr_value(q.rgb[p * 3 + 0]), accum::hdr_value(q.rgb[p * 3 + 1]), accum::hdr_value(q.rgb[p * 3 + 2])};
    const float cov = guide_value(q.coverage[p]);
    if (!(cov > 0.0f)) {   // not live
        q.history_out[p] = make_float4(c[0], c[1], c[2], 0.0f);
        q.history_out[px + p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        q.history_out[2 * px + p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (q.out_rgb) { q.out_rgb[p * 3 + 0] = c[0]; q.out_rgb[p * 3 + 1] = c[1]; q.out_rgb[p * 3 + 2] = c[2]; }
        if (q.out_variance) q.out_variance[p] = 0.0f;
        return;
    }
    const F3 n_p{guide_value(q.normal[p * 3 + 0]), guide_value(q.normal[p * 3 + 1]), guide_value(q.normal[p * 3 + 2])};
    const float z_p = guide_value(q.depth[p]);

    bool ok[4] = {false, false, false, false};
    float w[4] = {0.0f, 0.0f, 0.0f, 0.0f}, m1q[4] = {0.0f, 0.0f, 0.0f, 0.0f}, m2q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    size_t t[4] = {0, 0, 0, 0};
    float sw = 0.0f;
    [[maybe_unused]] float vq[4] = {0.0f, 0.0f, 0.0f, 0.0f};                       // T7's V of the taps
    [[maybe_unused]] float s_fx = 0.0f, s_fy = 0.0f, s_zexp = 0.0f, s_ztol = 0.0f;   // T2's position, for T3s
    [[maybe_unused]] bool placed = false;
    if (q.history_in) {   // the same in every lane
        // T1
        const F3 d = ray_dir(q, (float)x + q.offset_x, (float)y + q.offset_y);
        const F3 P{q.cam_pos[0] + z_p * d.x, q.cam_pos[1] + z_p * d.y, q.cam_pos[2] + z_p * d.z};
        // T2
        float clip[4];
        mat_vec(q.prev_view_proj, P.x, P.y, P.z, 1.0f, clip);
        if (clip[3] > 1e-6f) {
            const float fx = (((clip[0] / clip[3]) + 1.0f) * 0.5f) * (float)q.width - q.offset_x;
            const float fy = (((clip[1] / clip[3]) + 1.0f) * 0.5f) * (float)q.height - q.offset_y;
            if (fx > -1.0f && fx < (float)q.width && fy > -1.0f && fy < (float)q.height) {
                const float xf = __builtin_floorf(fx), yf = __builtin_floorf(fy);
                const float tx = fx - xf, ty = fy - yf;
                const int x0 = (int)xf, y0 = (int)yf;
                const float zexp = len3(sub3(P, F3{q.prev_cam_pos[0], q.prev_cam_pos[1], q.prev_cam_pos[2]}));
                const float ztol = q.depth_tol * zexp + 0x1p-20f;
                w[0] = (1.0f - tx) * (1.0f - ty);
                w[1] = tx * (1.0f - ty);
                w[2] = (1.0f - tx) * ty;
                w[3] = tx * ty;
                if constexpr (kMom) { s_fx = fx; s_fy = fy; s_zexp = zexp; s_ztol = ztol; placed = true; }
                // T3: the guide words of every tap, then the verdicts
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                    if (qx < 0 || qx >= q.width || qy < 0 || qy >= q.height) continue;
                    t[k] = (size_t)qy * (size_t)q.width + (size_t)qx;
                    float4 g1 = q.history_in[px + t[k]], g2 = q.history_in[2 * px + t[k]];
                    // keeps plane 2's word one 16-byte load: V is used blocks later, and the compiler otherwise gathers it again as a
                    // load of its own, four more gathers a pixel
                    if constexpr (kMom) asm volatile("" : "+v"(g2.x), "+v"(g2.y), "+v"(g2.z), "+v"(g2.w));
                    m1q[k] = accum::hdr_value(g1.x);
                    m2q[k] = var_value(g1.y);
                    const float zq = guide_value(g1.z);
                    const float nd = (guide_value(g2.x) * n_p.x + guide_value(g2.y) * n_p.y) + guide_value(g2.z) * n_p.z;
                    ok[k] = guide_value(g1.w) > 0.0f && nd >= q.normal_min && __builtin_fabsf(zq - zexp) <= ztol;
                    if constexpr (kMom) vq[k] = var_value(g2.w);
                }
            }
        }
    }
    // ... and the colour word of the taps that pass so far: its N decides last
    float4 cq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cq[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (ok[k]) {
            const float4 h0 = q.history_in[t[k]];
            cq[k] = make_float4(accum::hdr_value(h0.x), accum::hdr_value(h0.y), accum::hdr_value(h0.z),
                                fmin_c(fmax_c(0.0f, guide_value(h0.w)), q.max_history));
            ok[k] = cq[k].w >= 1.0f;
        }
        if (ok[k]) sw = sw + w[k];
    }
    float cp[3] = {0.0f, 0.0f, 0.0f}, n_prev = 0.0f, m1p = 0.0f, m2p = 0.0f;
    if (sw > 0.0f) {
        cp[0] = previous(ok, w, cq[0].x, cq[1].x, cq[2].x, cq[3].x, sw);
        cp[1] = previous(ok, w, cq[0].y, cq[1].y, cq[2].y, cq[3].y, sw);
        cp[2] = previous(ok, w, cq[0].z, cq[1].z, cq[2].z, cq[3].z, sw);
        n_prev = previous(ok, w, cq[0].w, cq[1].w, cq[2].w, cq[3].w, sw);
        m1p = previous(ok, w, m1q[0], m1q[1], m1q[2], m1q[3], sw);
        m2p = previous(ok, w, m2q[0], m2q[1], m2q[2], m2q[3], sw);
    }
    [[maybe_unused]] float vp = 0.0f;
    if constexpr (kMom) {
        if (sw > 0.0f) {
            vp = previous(ok, w, vq[0], vq[1], vq[2], vq[3], sw);
        } else if (placed && q.search != 0 && sw == 0.0f) {
            // T3s: rare and divergent, so one rolled loop over the nine taps with running sums -- guide words, then the colour word
            const int xc = (int)__builtin_floorf(s_fx + 0.5f), yc = (int)__builtin_floorf(s_fy + 0.5f);
            float sc0 = 0.0f, sc1 = 0.0f, sc2 = 0.0f, sn = 0.0f, s1 = 0.0f, s2 = 0.0f, sv = 0.0f, ssw = 0.0f;
#pragma unroll 1
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll 1
                for (int dx = -1; dx <= 1; ++dx) {
                    const int qx = xc + dx, qy = yc + dy;
                    if (qx < 0 || qx >= q.width || qy < 0 || qy >= q.height) continue;
                    const size_t tq = (size_t)qy * (size_t)q.width + (size_t)qx;
                    const float4 g1 = q.history_in[px + tq], g2 = q.history_in[2 * px + tq];
                    const float nd = (guide_value(g2.x) * n_p.x + guide_value(g2.y) * n_p.y) + guide_value(g2.z) * n_p.z;
                    if (!(guide_value(g1.w) > 0.0f && nd >= q.normal_min && __builtin_fabsf(guide_value(g1.z) - s_zexp) <= s_ztol)) continue;
                    const float4 h0 = q.history_in[tq];
                    const float nq = fmin_c(fmax_c(0.0f, guide_value(h0.w)), q.max_history);
                    if (!(nq >= 1.0f)) continue;
                    ssw = ssw + 1.0f;
                    sc0 = sc0 + accum::hdr_value(h0.x);
                    sc1 = sc1 + accum::hdr_value(h0.y);
                    sc2 = sc2 + accum::hdr_value(h0.z);
                    sn = sn + nq;
                    s1 = s1 + accum::hdr_value(g1.x);
                    s2 = s2 + var_value(g1.y);
                    sv = sv + var_value(g2.w);
                }
            }
            if (ssw > 0.0f) {
                cp[0] = sc0 / ssw; cp[1] = sc1 / ssw; cp[2] = sc2 / ssw;
                n_prev = sn / ssw; m1p = s1 / ssw; m2p = s2 / ssw; vp = sv / ssw;
            }
        }
    }
    // T4
    const float n_new = fmin_c(n_prev + 1.0f, q.max_history);
    const float a = fmax_c(1.0f / n_new, q.alpha_min), am = fmax_c(1.0f / n_new, q.alpha_moments_min);
    // T5
    const float r[3] = {cp[0] + a * (c[0] - cp[0]), cp[1] + a * (c[1] - cp[1]), cp[2] + a * (c[2] - cp[2])};
    const float yl = luminance(c[0], c[1], c[2]);
    const float m1 = m1p + am * (yl - m1p), m2 = m2p + am * (yl * yl - m2p);
    // T7
    [[maybe_unused]] float v_new = 0.0f;
    if constexpr (kMom) {
        const float v = q.variance_in ? var_value(q.variance_in[p]) : kVarMax;
        const float om = 1.0f - a;
        v_new = var_value((om * om) * vp + (a * a) * v);
    }
    // T6, T6m
    q.history_out[p] = make_float4(r[0], r[1], r[2], n_new);
    q.history_out[px + p] = make_float4(m1, m2, z_p, cov);
    q.history_out[2 * px + p] = make_float4(n_p.x, n_p.y, n_p.z, v_new);
    if (q.out_rgb) { q.out_rgb[p * 3 + 0] = r[0]; q.out_rgb[p * 3 + 1] = r[1]; q.out_rgb[p * 3 + 2] = r[2]; }
    if (q.out_variance) {
        const float spread = n_new >= 2.0f ? var_value(fmax_c(0.0f, m2 - m1 * m1) / (n_new - 1.0f)) : kVarMax;
        if constexpr (kMom) q.out_variance[p] = n_new < q.measured_below ? v_new : spread;
        else q.out_variance[p] = spread;
    }
}

}  // namespace temporal
}  // namespace vrt
