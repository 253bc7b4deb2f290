/* tests/oracle_filter_var.c -- TEST INFRASTRUCTURE ONLY: the variance-guided filter (include/vrt.h vrt_filter_hdr_var, V1-V4 beside
 * points 1-5) restated in scalar C, one pixel at a time, whole images between the levels.
 *
 * tests/oracle_filter_hdr.c, included unchanged, brings points 1-3 (o_filter_guide, modulation, slope), the guide-only filter this
 * one must reproduce where the luminance term is dropped, and everything that file includes. Every operation rounded on its own:
 * built by tests/oracle_filter_var.py with oracle/Makefile's flags (no contraction).
 *
 * plant != 0 changes the rule:
 *   1  the weight not squared in sumv                 2  the 3 x 3 of vbar at spacing 1 instead of s
 *   3  Ym forgotten in V2 (a caller's plane)          4  dl of the remodulated colour u * m instead of u
 * are PLANTED MISREADINGS the closed forms of tests/test_filter_var.py must catch;
 *   5  dl / sl dropped from e
 * is no misreading but the reduction to points 1-5: the colours are then o_filter_hdr's, bit for bit. */
#include "oracle_filter_hdr.c"

typedef struct o_filter_var { int32_t levels; uint32_t flags; float sigma_normal, sigma_albedo, sigma_depth, sigma_lum; } o_filter_var_t;

/* V1 */
static float lum(const float *u) { return (0.2126f * u[0] + 0.7152f * u[1]) + 0.0722f * u[2]; }

/* hv of V2 and V4 */
float o_filter_var_value(float v) { return fmin_c(fmax_c(0.0f, v), 65504.0f * 65504.0f); }

/* point 4's e of tap q = p + (tx - x, ty - y), the offsets counted as (ax, ay) pixels */
static float guide_e(const float *N, const float *A, const float *Z, const float *G, size_t p, size_t q, int ax, int ay, float kn, float ka,
                     float sigma_depth) {
    float dx = N[q * 3] - N[p * 3], dy = N[q * 3 + 1] - N[p * 3 + 1], dz = N[q * 3 + 2] - N[p * 3 + 2];
    float dn2 = (dx * dx + dy * dy) + dz * dz;
    float a0 = A[q * 4] - A[p * 4], a1 = A[q * 4 + 1] - A[p * 4 + 1], a2 = A[q * 4 + 2] - A[p * 4 + 2], a3 = A[q * 4 + 3] - A[p * 4 + 3];
    float da2 = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
    float dzq = fabsf(Z[q] - Z[p]);
    float den = sigma_depth * ((G[p * 2] * (float)ax + G[p * 2 + 1] * (float)ay) + Z[p] * (1.0f / 256.0f)) + 0x1p-20f;
    return (dn2 * kn + da2 * ka) + dzq / den;
}

/* The planes as o_filter_hdr takes them; variance [H][W] or NULL (the spatial estimate). out_rgb [H][W][3], out_rgba8 [H][W][4],
 * out_var [H][W], v0_out [H][W] (V2's result; 0 where not live): any may be NULL. level_out (may be NULL): [levels][H][W][4], u and v
 * after each level (zeros where the pixel is not live). Returns 0, or -1 where memory runs out. */
int o_filter_var(const float *rgb, const float *normal, const float *albedo, const float *depth, const float *coverage, const float *variance,
                 int W, int H, const o_filter_var_t *f, int op, float e, int plant, float *out_rgb, uint8_t *out_rgba8, float *out_var,
                 float *level_out, float *v0_out) {
    const size_t px = (size_t)W * (size_t)H;
    const int demod = (f->flags & 1u) != 0;
    const float kn = 1.0f / (f->sigma_normal * f->sigma_normal), ka = 1.0f / (f->sigma_albedo * f->sigma_albedo);
    static const float B[3] = {0.375f, 0.25f, 0.0625f};
    float *N = malloc(px * 3 * sizeof(float)), *A = malloc(px * 4 * sizeof(float)), *Z = malloc(px * sizeof(float));
    float *C = malloc(px * sizeof(float)), *M = malloc(px * 3 * sizeof(float)), *G = malloc(px * 2 * sizeof(float));
    float *u = malloc(px * 3 * sizeof(float)), *un = malloc(px * 3 * sizeof(float));
    float *v = malloc(px * sizeof(float)), *vn = malloc(px * sizeof(float)), *Ym2 = malloc(px * sizeof(float));
    uint8_t *live = malloc(px);
    int rc = -1;
    if (!N || !A || !Z || !C || !M || !G || !u || !un || !v || !vn || !Ym2 || !live) goto done;
    for (size_t p = 0; p < px; p++) {                                                  /* points 1 and 2 */
        for (int k = 0; k < 3; k++) N[p * 3 + k] = o_filter_guide(normal[p * 3 + k]);
        for (int k = 0; k < 4; k++) A[p * 4 + k] = o_filter_guide(albedo[p * 4 + k]);
        Z[p] = o_filter_guide(depth[p]);
        C[p] = o_filter_guide(coverage[p]);
        live[p] = C[p] > 0.0f;
        for (int k = 0; k < 3; k++) {
            M[p * 3 + k] = demod ? modulation(A[p * 4 + k], C[p]) : 1.0f;
            u[p * 3 + k] = o_hdr_value(rgb[p * 3 + k]) / M[p * 3 + k];
        }
        float ym = demod ? lum(M + p * 3) : 1.0f;
        Ym2[p] = ym * ym;
    }
    for (int y = 0; y < H; y++)                                                        /* point 3 */
        for (int x = 0; x < W; x++) {
            size_t p = (size_t)y * W + x;
            G[p * 2 + 0] = live[p] ? slope(Z, live, p, 1, x > 0, x + 1 < W, 0) : 0.0f;
            G[p * 2 + 1] = live[p] ? slope(Z, live, p, (size_t)W, y > 0, y + 1 < H, 0) : 0.0f;
        }
    for (int y = 0; y < H; y++)                                                        /* V2 */
        for (int x = 0; x < W; x++) {
            size_t p = (size_t)y * W + x;
            if (!live[p]) { v[p] = 0.0f; continue; }
            if (variance) {
                v[p] = plant == 3 ? o_filter_var_value(variance[p]) : o_filter_var_value(variance[p]) / Ym2[p];
                continue;
            }
            float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int oy = -3; oy <= 3; oy++)
                for (int ox = -3; ox <= 3; ox++) {
                    int tx = x + ox, ty = y + oy;
                    if (tx < 0 || tx >= W || ty < 0 || ty >= H) continue;
                    size_t q = (size_t)ty * W + tx;
                    if (!live[q]) continue;
                    float w = o_det_expf(-guide_e(N, A, Z, G, p, q, abs(ox), abs(oy), kn, ka, f->sigma_depth));
                    float l = lum(u + q * 3);
                    sw = sw + w;
                    s1 = s1 + w * l;
                    s2 = s2 + w * (l * l);
                }
            float m1 = s1 / sw, m2 = s2 / sw;
            v[p] = fmax_c(0.0f, m2 - m1 * m1);
        }
    if (v0_out) memcpy(v0_out, v, px * sizeof(float));
    for (int i = 0; i < f->levels; i++) {                                              /* V3 */
        const int s = 1 << i, s3 = plant == 2 ? 1 : s;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                size_t p = (size_t)y * W + x;
                if (!live[p]) { un[p * 3] = un[p * 3 + 1] = un[p * 3 + 2] = 0.0f; vn[p] = 0.0f; continue; }
                float gs = 0.0f, gv = 0.0f;
                for (int oy = -1; oy <= 1; oy++)
                    for (int ox = -1; ox <= 1; ox++) {
                        int tx = x + s3 * ox, ty = y + s3 * oy;
                        if (tx < 0 || tx >= W || ty < 0 || ty >= H) continue;
                        size_t q = (size_t)ty * W + tx;
                        if (!live[q]) continue;
                        float g = (ox == 0 && oy == 0) ? 0.25f : ((ox == 0 || oy == 0) ? 0.125f : 0.0625f);
                        gs = gs + g;
                        gv = gv + g * v[q];
                    }
                float vbar = gv / gs;
                float sl = f->sigma_lum * sqrtf(vbar) + 0x1p-20f;
                float rp[3] = {u[p * 3] * M[p * 3], u[p * 3 + 1] * M[p * 3 + 1], u[p * 3 + 2] * M[p * 3 + 2]};
                float yp = plant == 4 ? lum(rp) : lum(u + p * 3);
                float sumw = 0.0f, sumv = 0.0f, sum[3] = {0.0f, 0.0f, 0.0f};
                for (int oy = -2; oy <= 2; oy++)
                    for (int ox = -2; ox <= 2; ox++) {
                        int tx = x + s * ox, ty = y + s * oy;
                        if (tx < 0 || tx >= W || ty < 0 || ty >= H) continue;
                        size_t q = (size_t)ty * W + tx;
                        if (!live[q]) continue;
                        int ax = abs(ox), ay = abs(oy);
                        float rq[3] = {u[q * 3] * M[q * 3], u[q * 3 + 1] * M[q * 3 + 1], u[q * 3 + 2] * M[q * 3 + 2]};
                        float dl = fabsf((plant == 4 ? lum(rq) : lum(u + q * 3)) - yp);
                        float ee = guide_e(N, A, Z, G, p, q, ax * s, ay * s, kn, ka, f->sigma_depth);
                        if (plant != 5) ee = ee + dl / sl;
                        float w = (B[ay] * B[ax]) * o_det_expf(-ee);
                        sumw = sumw + w;
                        for (int k = 0; k < 3; k++) sum[k] = sum[k] + w * u[q * 3 + k];
                        sumv = sumv + (plant == 1 ? w : w * w) * v[q];
                    }
                for (int k = 0; k < 3; k++) un[p * 3 + k] = sum[k] / sumw;
                vn[p] = sumv / (sumw * sumw);
            }
        float *t = u; u = un; un = t;
        t = v; v = vn; vn = t;
        if (level_out)
            for (size_t p = 0; p < px; p++) {
                float *o = level_out + ((size_t)i * px + p) * 4;
                o[0] = u[p * 3]; o[1] = u[p * 3 + 1]; o[2] = u[p * 3 + 2]; o[3] = v[p];
            }
    }
    for (size_t p = 0; p < px; p++) {                                                  /* V4 */
        float fo[3];
        for (int k = 0; k < 3; k++) fo[k] = live[p] ? o_hdr_value(u[p * 3 + k] * M[p * 3 + k]) : o_hdr_value(rgb[p * 3 + k]);
        if (out_rgb) memcpy(out_rgb + p * 3, fo, sizeof fo);
        if (out_rgba8) o_hdr_tonemap(fo, 1, op, e, out_rgba8 + p * 4);
        if (out_var) out_var[p] = live[p] ? o_filter_var_value(v[p] * Ym2[p]) : 0.0f;
    }
    rc = 0;
done:
    free(N); free(A); free(Z); free(C); free(M); free(G); free(u); free(un); free(v); free(vn); free(Ym2); free(live);
    return rc;
}
