/* tests/oracle_filter_hdr.c -- TEST INFRASTRUCTURE ONLY: the guided filter (include/vrt.h vrt_filter_hdr, points 1-5) restated in
 * scalar C, one pixel at a time, whole images between the levels.
 *
 * tests/oracle_denoise_hdr.c, included unchanged, brings tests/oracle_hdr.c (h = o_hdr_value, the tone map and unorm8 =
 * o_hdr_tonemap, the samples' float colours) and the ID-aware blur the quality test compares with; o_det_expf is the exp of
 * oracle/rt_oracle.c. Every operation rounded on its own: built by tests/oracle_filter_hdr.py with oracle/Makefile's flags (no
 * contraction).
 *
 * plant != 0 is a PLANTED MISREADING the closed forms of tests/test_filter_hdr.py must catch:
 *   1  the depth slopes as the two-sided maximum      2  alpha left out of da2
 *   3  dead taps included                             4  the step not applied to the offsets in den */
#include "oracle_denoise_hdr.c"

#include <stdlib.h>

typedef struct o_filter { int32_t levels; uint32_t flags; float sigma_normal, sigma_albedo, sigma_depth; } o_filter;

/* point 1: g(v) */
float o_filter_guide(float v) { return v != v ? 0.0f : fmin_c(fmax_c(-65504.0f, v), 65504.0f); }

/* point 2: m of one channel */
static float modulation(float albedo, float coverage) { return fmax_c(albedo + (1.0f - coverage), 1.0f / 255.0f); }

/* point 3: over the two neighbours `stride` pixels either side of p that exist (lo / hi) and are live */
static float slope(const float *Z, const uint8_t *live, size_t p, size_t stride, int lo, int hi, int plant) {
    float s = 0.0f;
    int have = 0;
    if (lo && live[p - stride]) { s = fabsf(Z[p - stride] - Z[p]); have = 1; }
    if (hi && live[p + stride]) {
        float d = fabsf(Z[p + stride] - Z[p]);
        s = have ? (plant == 1 ? fmax_c(s, d) : fmin_c(s, d)) : d;
    }
    return s;
}

/* rgb [H][W][3], normal [H][W][3], albedo [H][W][4], depth [H][W], coverage [H][W]; out_rgb [H][W][3] and out_rgba8 [H][W][4],
 * either may be NULL. level_out (may be NULL): [levels][H][W][3], u after each level (what the next one reads; zeros where the
 * pixel is not live). Returns 0, or -1 where memory runs out. */
int o_filter_hdr(const float *rgb, const float *normal, const float *albedo, const float *depth, const float *coverage, int W, int H,
                 const o_filter *f, int op, float e, int plant, float *out_rgb, uint8_t *out_rgba8, float *level_out) {
    const size_t px = (size_t)W * (size_t)H;
    const int demod = (f->flags & 1u) != 0;
    const float kn = 1.0f / (f->sigma_normal * f->sigma_normal), ka = 1.0f / (f->sigma_albedo * f->sigma_albedo);
    static const float B[3] = {0.375f, 0.25f, 0.0625f};
    float *N = malloc(px * 3 * sizeof(float)), *A = malloc(px * 4 * sizeof(float)), *Z = malloc(px * sizeof(float));
    float *C = malloc(px * sizeof(float)), *M = malloc(px * 3 * sizeof(float)), *G = malloc(px * 2 * sizeof(float));
    float *u = malloc(px * 3 * sizeof(float)), *v = malloc(px * 3 * sizeof(float));
    uint8_t *live = malloc(px);
    int rc = -1;
    if (!N || !A || !Z || !C || !M || !G || !u || !v || !live) goto done;
    for (size_t p = 0; p < px; p++) {                                                  /* points 1 and 2 */
        for (int k = 0; k < 3; k++) N[p * 3 + k] = o_filter_guide(normal[p * 3 + k]);
        for (int k = 0; k < 4; k++) A[p * 4 + k] = o_filter_guide(albedo[p * 4 + k]);
        Z[p] = o_filter_guide(depth[p]);
        C[p] = o_filter_guide(coverage[p]);
        live[p] = C[p] > 0.0f;
        for (int k = 0; k < 3; k++) {
            M[p * 3 + k] = demod ? modulation(A[p * 4 + k], C[p]) : 1.0f;
            u[p * 3 + k] = o_hdr_value(rgb[p * 3 + k]) / M[p * 3 + k];   /* read where the pixel is live (and by plant 3) */
        }
    }
    for (int y = 0; y < H; y++)                                                        /* point 3 */
        for (int x = 0; x < W; x++) {
            size_t p = (size_t)y * W + x;
            G[p * 2 + 0] = live[p] ? slope(Z, live, p, 1, x > 0, x + 1 < W, plant) : 0.0f;
            G[p * 2 + 1] = live[p] ? slope(Z, live, p, (size_t)W, y > 0, y + 1 < H, plant) : 0.0f;
        }
    for (int i = 0; i < f->levels; i++) {                                              /* point 4 */
        const int s = 1 << i;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                size_t p = (size_t)y * W + x;
                if (!live[p]) { v[p * 3] = v[p * 3 + 1] = v[p * 3 + 2] = 0.0f; continue; }
                float sumw = 0.0f, sum[3] = {0.0f, 0.0f, 0.0f};
                for (int oy = -2; oy <= 2; oy++)
                    for (int ox = -2; ox <= 2; ox++) {
                        int tx = x + s * ox, ty = y + s * oy;
                        if (tx < 0 || tx >= W || ty < 0 || ty >= H) continue;
                        size_t q = (size_t)ty * W + tx;
                        if (!live[q] && plant != 3) continue;
                        int ax = abs(ox), ay = abs(oy), sd = plant == 4 ? 1 : s;
                        float dx = N[q * 3] - N[p * 3], dy = N[q * 3 + 1] - N[p * 3 + 1], dz = N[q * 3 + 2] - N[p * 3 + 2];
                        float dn2 = (dx * dx + dy * dy) + dz * dz;
                        float a0 = A[q * 4] - A[p * 4], a1 = A[q * 4 + 1] - A[p * 4 + 1], a2 = A[q * 4 + 2] - A[p * 4 + 2],
                              a3 = plant == 2 ? 0.0f : A[q * 4 + 3] - A[p * 4 + 3];
                        float da2 = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
                        float dzq = fabsf(Z[q] - Z[p]);
                        float den = f->sigma_depth * ((G[p * 2] * (float)(ax * sd) + G[p * 2 + 1] * (float)(ay * sd)) + Z[p] * (1.0f / 256.0f)) + 0x1p-20f;
                        float ee = (dn2 * kn + da2 * ka) + dzq / den;
                        float w = (B[ay] * B[ax]) * o_det_expf(-ee);
                        sumw = sumw + w;
                        for (int k = 0; k < 3; k++) sum[k] = sum[k] + w * u[q * 3 + k];
                    }
                for (int k = 0; k < 3; k++) v[p * 3 + k] = sum[k] / sumw;
            }
        float *t = u; u = v; v = t;
        if (level_out) memcpy(level_out + (size_t)i * px * 3, u, px * 3 * sizeof(float));
    }
    for (size_t p = 0; p < px; p++) {                                                  /* point 5 */
        float fo[3];
        for (int k = 0; k < 3; k++) fo[k] = live[p] ? o_hdr_value(u[p * 3 + k] * M[p * 3 + k]) : o_hdr_value(rgb[p * 3 + k]);
        if (out_rgb) memcpy(out_rgb + p * 3, fo, sizeof fo);
        if (out_rgba8) o_hdr_tonemap(fo, 1, op, e, out_rgba8 + p * 4);
    }
    rc = 0;
done:
    free(N); free(A); free(Z); free(C); free(M); free(G); free(u); free(v); free(live);
    return rc;
}
