/* tests/oracle_bloom.c -- TEST INFRASTRUCTURE ONLY: bloom (include/vrt.h vrt_bloom_hdr, points B0-B8) restated in scalar C, written
 * from the header and from nothing of the product's code. tests/oracle_hdr.c, included unchanged, brings h = o_hdr_value, the min and
 * max of the unorm8 store and the store itself. Every operation rounded on its own (built with oracle/Makefile's flags: no
 * contraction, no fast-math).
 * plant: 0 the rule; 1 far and near swapped in B5's lerp; 2 the tent evaluated as a multiply by 3; 3 the KARIS weight left in at
 * level 2 (level 1 stores the weighted sums, level 2 divides); 4 the threshold compared against Y instead of Ye; 5 invL left out. */
#include "oracle_hdr.c"

#include <stdlib.h>

typedef struct { int32_t levels; uint32_t flags; float threshold, knee, intensity; } o_bloom;
typedef struct { float exposure, metered; uint32_t window, frames; } o_bloom_record;

#define O_BLOOM_MAX_LEVELS 8
#define O_F32_MAX 3.402823466e38f

/* E1 */
static float o_bloom_lum(const float *c) {
    return (0.2126f * o_hdr_value(c[0]) + 0.7152f * o_hdr_value(c[1])) + 0.0722f * o_hdr_value(c[2]);
}

static int o_bloom_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

/* B0 */
void o_bloom_sizes(int W, int H, int levels, int *w, int *h) {
    w[0] = W;
    h[0] = H;
    for (int l = 1; l <= levels; l++) {
        w[l] = (w[l - 1] + 1) >> 1;
        h[l] = (h[l - 1] + 1) >> 1;
    }
}

/* B2, B3: the input pixel c -> out[4] */
static void o_bloom_bright(const float *c, float eb, const o_bloom *b, int plant, float *out) {
    const float y = o_bloom_lum(c);
    const float ye = fmin_c(y * eb, O_F32_MAX);
    const float d = (plant == 4 ? y : ye) - b->threshold;
    float soft = 0.0f;
    if (b->knee > 0.0f) {
        const float s = fmin_c(fmax_c(d + b->knee, 0.0f), b->knee + b->knee);
        soft = (s * s) / (4.0f * b->knee);
    }
    const float a = fmax_c(fmax_c(soft, d), 0.0f);
    const float g = fmin_c(a / fmax_c(ye, 0x1p-16f), 1.0f);
    for (int k = 0; k < 3; k++) out[k] = o_hdr_value(c[k]) * g;
    out[3] = 1.0f;
    if (b->flags & 1u) {
        const float w = 1.0f / (1.0f + o_bloom_lum(out));
        for (int k = 0; k < 3; k++) out[k] = out[k] * w;
        out[3] = w;
    }
}

/* B4's T */
static float o_bloom_tent(float a0, float a1, float a2, float a3, int plant) {
    if (plant == 2) return (a0 + 3.0f * a1) + (3.0f * a2 + a3);
    const float p0 = a0 + a1, p1 = a1 + a2, p2 = a2 + a3;
    return (p0 + p1) + (p1 + p2);
}

/* B4: src (sw x sh, 4 floats per pixel) -> dst (dw x dh); divide: store v.ch / v.w and w = 1 */
static void o_bloom_down(const float *src, int sw, int sh, float *dst, int dw, int dh, int divide, int plant) {
    for (int Y = 0; Y < dh; Y++)
        for (int X = 0; X < dw; X++) {
            float v[4];
            for (int k = 0; k < 4; k++) {
                float r[4];
                for (int j = 0; j < 4; j++) {
                    const float *row = src + (size_t)o_bloom_clamp(2 * Y - 1 + j, sh - 1) * (size_t)sw * 4;
                    float a[4];
                    for (int o = 0; o < 4; o++) a[o] = row[(size_t)o_bloom_clamp(2 * X - 1 + o, sw - 1) * 4 + k];
                    r[j] = o_bloom_tent(a[0], a[1], a[2], a[3], plant);
                }
                v[k] = o_bloom_tent(r[0], r[1], r[2], r[3], plant) * 0.015625f;
            }
            float *d = dst + ((size_t)Y * (size_t)dw + (size_t)X) * 4;
            if (divide) {
                d[0] = v[0] / v[3];
                d[1] = v[1] / v[3];
                d[2] = v[2] / v[3];
                d[3] = 1.0f;
            } else {
                for (int k = 0; k < 4; k++) d[k] = v[k];
            }
        }
}

/* B5 */
static float o_bloom_lerp(float far_, float near_, int plant) {
    if (plant == 1) { const float t = far_; far_ = near_; near_ = t; }
    return ((far_ + near_) + (near_ + near_)) * 0.25f;
}
static float o_bloom_up(const float *s, int sw, int sh, int x, int y, int k, int plant) {
    const int nx = x >> 1, ny = y >> 1;
    const int fx = o_bloom_clamp(nx + ((x & 1) ? 1 : -1), sw - 1), fy = o_bloom_clamp(ny + ((y & 1) ? 1 : -1), sh - 1);
    const float tf = o_bloom_lerp(s[((size_t)fy * sw + fx) * 4 + k], s[((size_t)fy * sw + nx) * 4 + k], plant);
    const float tn = o_bloom_lerp(s[((size_t)ny * sw + fx) * 4 + k], s[((size_t)ny * sw + nx) * 4 + k], plant);
    return o_bloom_lerp(tf, tn, plant);
}

/* B0-B8. rec == NULL: no record. out_rgb (W*H*3), out_rgba8 (W*H*4), out_levels (every D_l of l = 1..L one after the other, 4 floats
 * per pixel, as B4 leaves them) and out_glow (B of B7, W*H*3) may each be NULL. Returns 0, or -1 where memory ran out. */
int o_bloom_run(const float *rgb, int W, int H, const o_bloom *b, int op, float tm_exposure, const o_bloom_record *rec, int plant,
                float *out_rgb, uint8_t *out_rgba8, float *out_levels, float *out_glow) {
    const int L = b->levels;
    int w[O_BLOOM_MAX_LEVELS + 1], h[O_BLOOM_MAX_LEVELS + 1];
    o_bloom_sizes(W, H, L, w, h);
    float e = tm_exposure;
    if (rec) e = fmin_c(tm_exposure * rec->exposure, O_F32_MAX);   /* B1 = E9's e */
    float *lev[O_BLOOM_MAX_LEVELS + 1] = {0};
    for (int l = 0; l <= L; l++) {
        lev[l] = (float *)malloc((size_t)w[l] * (size_t)h[l] * 4 * sizeof(float));
        if (!lev[l]) {
            for (int i = 0; i < l; i++) free(lev[i]);
            return -1;
        }
    }
    const size_t px = (size_t)W * (size_t)H;
    for (size_t p = 0; p < px; p++) o_bloom_bright(rgb + p * 3, e, b, plant, lev[0] + p * 4);
    const int karis = (b->flags & 1u) != 0;
    for (int l = 1; l <= L; l++) o_bloom_down(lev[l - 1], w[l - 1], h[l - 1], lev[l], w[l], h[l], karis && l == (plant == 3 ? 2 : 1), plant);
    if (out_levels) {
        size_t at = 0;
        for (int l = 1; l <= L; l++) {
            const size_t n = (size_t)w[l] * (size_t)h[l] * 4;
            memcpy(out_levels + at, lev[l], n * sizeof(float));
            at += n;
        }
    }
    /* B6 */
    for (int l = L - 1; l >= 1; l--)
        for (int y = 0; y < h[l]; y++)
            for (int x = 0; x < w[l]; x++)
                for (int k = 0; k < 4; k++) {
                    float *d = lev[l] + ((size_t)y * w[l] + x) * 4 + k;
                    *d = *d + o_bloom_up(lev[l + 1], w[l + 1], h[l + 1], x, y, k, plant);
                }
    /* B7, B8 */
    const float inv_l = plant == 5 ? 1.0f : 1.0f / (float)L;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * (size_t)W + (size_t)x;
            for (int k = 0; k < 3; k++) {
                const float glow = o_bloom_up(lev[1], w[1], h[1], x, y, k, plant) * inv_l;
                const float f = o_hdr_value(o_hdr_value(rgb[p * 3 + k]) + b->intensity * glow);
                if (out_glow) out_glow[p * 3 + k] = glow;
                if (out_rgb) out_rgb[p * 3 + k] = f;
                if (out_rgba8) {
                    const float xe = e * f;
                    const float t = op == 1 ? xe / (1.0f + xe) : xe;
                    out_rgba8[p * 4 + k] = t != t ? 0 : unorm8(t);
                }
            }
            if (out_rgba8) out_rgba8[p * 4 + 3] = 255;
        }
    for (int l = 0; l <= L; l++) free(lev[l]);
    return 0;
}
