/* tests/oracle_hdr.c -- TEST INFRASTRUCTURE ONLY: the oracle's FLOAT colour at any sample of the progressive accumulation, and the
 * HDR accumulation's arithmetic (include/vrt.h vrt_accum_keep_hdr) restated in plain C.
 *
 * tests/oracle_lens.c, included unchanged (and with it oracle/rt_oracle.c), makes the ray of any sample -- the corner's
 * (aperture 0, no jitter), the jittered one, the thin lens's. o_render_hdr is its o_render_lens with the three floats path_trace
 * returns stored as they are instead of through unorm8: unorm8 of them is o_render_lens's frame byte for byte
 * (tests/test_accum_hdr.py checks that). Then h(c), the sequential float64 sum, the mean and the two tone maps, every operation
 * rounded on its own. Built by tests/oracle_hdr.py with the oracle's own flags (no contraction) together with the other three
 * oracle sources. */
#include "oracle_lens.c"

void o_render_hdr(const o_scene *s, int W, int H, int row0, int row1, int mode, uint32_t sample, int jitter, float aperture,
                  float focus, float *rgb_out) {
    ctx_t c;
    memset(&c, 0, sizeof c);
    c.s = s;
    for (int py = row0; py < row1; py++) {
        for (int px = 0; px < W; px++) {
            c.px_fetches = 0;
            c.px_index = (uint32_t)(py * W + px);
            init_rng(&c, px, py, (int)sample);
            float o[3], d[3];
            (void)o_lens_ray(s, W, H, px, py, sample, jitter, aperture, focus, o, d);
            v3 ro = {o[0], o[1], o[2]}, wd = {d[0], d[1], d[2]};
            float rgb[3];
            int32_t vid, dist;
            path_trace(&c, ro, wd, mode, rgb, &vid, &dist);
            size_t p = (size_t)py * (size_t)W + (size_t)px;
            rgb_out[p * 3 + 0] = rgb[0]; rgb_out[p * 3 + 1] = rgb[1]; rgb_out[p * 3 + 2] = rgb[2];
        }
    }
}

/* the unorm8 store of n floats (NaN stores 0, as the device's conversion does) */
void o_hdr_unorm8(const float *v, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) out[i] = v[i] != v[i] ? 0 : unorm8(v[i]);
}

/* point 1: h(c) = min(max(0, c), 65504) in the store's min / max conventions, the zero first: NaN -> +0 */
float o_hdr_value(float c) { return fmin_c(fmax_c(0.0f, c), 65504.0f); }

/* point 2: sums[i] = sums[i] + (double)h(c[i]) for the entries with take[i] != 0 (take == NULL: all) */
void o_hdr_add(double *sums, const float *c, const uint8_t *take, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!take || take[i]) sums[i] = sums[i] + (double)o_hdr_value(c[i]);
}

/* k sequential adds of h(c) to +0.0 */
double o_hdr_sum_repeat(float c, uint32_t k) {
    double s = 0.0;
    const double v = (double)o_hdr_value(c);
    for (uint32_t i = 0; i < k; i++) s = s + v;
    return s;
}

/* ... and the product that stands for them */
double o_hdr_product(float c, uint32_t k) { return (double)o_hdr_value(c) * (double)k; }

/* point 3: mean[i] = (float)(sums[i] / (double)counts[i / 3]) */
void o_hdr_mean(const double *sums, const uint32_t *counts, size_t pixels, float *mean) {
    for (size_t p = 0; p < pixels; p++)
        for (int k = 0; k < 3; k++) mean[p * 3 + k] = (float)(sums[p * 3 + k] / (double)counts[p]);
}

/* point 4: op 0 clamp (y = e * x), op 1 Reinhard (x' = e * x; y = x' / (1 + x')); rgba8 = unorm8(y), alpha 255 */
void o_hdr_tonemap(const float *mean, size_t pixels, int op, float e, uint8_t *rgba8) {
    for (size_t p = 0; p < pixels; p++) {
        for (int k = 0; k < 3; k++) {
            const float xe = e * mean[p * 3 + k];
            const float y = op == 1 ? xe / (1.0f + xe) : xe;
            rgba8[p * 4 + k] = y != y ? 0 : unorm8(y);
        }
        rgba8[p * 4 + 3] = 255;
    }
}
