/* tests/oracle_moments.c -- TEST INFRASTRUCTURE ONLY: the luminance moments of an HDR accumulation (include/vrt.h
 * vrt_accum_keep_moments, points M1-M3) restated in scalar C.
 *
 * tests/oracle_hdr.c, included unchanged, gives the float colour of any sample and h(c). Here: a sample's luminance and its float32
 * square (M1), the two sequential float64 sums (M2) with the product that stands for k equal samples, and the resolve to the
 * variance of the mean's luminance (M3), every operation rounded on its own. `plant` puts one deliberate misreading of the rule
 * in (tests/oracle_moments.py PLANT), for the tests that show the checker tells them apart. Built by tests/oracle_moments.py with
 * the oracle's own flags (no contraction). */
#include "oracle_hdr.c"

enum { PLANT_NONE = 0, PLANT_DIVISOR_N = 1, PLANT_SQUARE_IN_DOUBLE = 2, PLANT_Y_OF_BYTES = 3 };

/* M1: y = Y(h(c)) with V1's Y and its association */
float o_mom_luminance(const float *c, int plant) {
    float h[3];
    for (int k = 0; k < 3; k++) {
        h[k] = o_hdr_value(c[k]);
        if (plant == PLANT_Y_OF_BYTES) h[k] = (float)unorm8(h[k]) / 255.0f;
    }
    return (0.2126f * h[0] + 0.7152f * h[1]) + 0.0722f * h[2];
}

/* M2: s[p] = {S1, S2}; one add each for the pixels with take[p] != 0 (take == NULL: all), c: 3 floats per pixel */
void o_mom_add(double *s, const float *c, const uint8_t *take, size_t pixels, int plant) {
    for (size_t p = 0; p < pixels; p++) {
        if (take && !take[p]) continue;
        const float y = o_mom_luminance(c + p * 3, plant);
        const float q = y * y;
        s[p * 2 + 0] = s[p * 2 + 0] + (double)y;
        s[p * 2 + 1] = s[p * 2 + 1] + (double)q;
    }
}

/* k sequential adds of one colour to {+0.0, +0.0} ... */
void o_mom_sum_repeat(const float *c, uint32_t k, double *s) {
    s[0] = s[1] = 0.0;
    for (uint32_t i = 0; i < k; i++) o_mom_add(s, c, NULL, 1, PLANT_NONE);
}

/* ... and the products that stand for them: s = s + (double)y * k, s = s + (double)q * k */
void o_mom_add_product(const float *c, uint32_t k, double *s) {
    const float y = o_mom_luminance(c, PLANT_NONE);
    const float q = y * y;
    s[0] = s[0] + (double)y * (double)k;
    s[1] = s[1] + (double)q * (double)k;
}

/* hv of V2: NaN, -0 and everything negative -> +0, else at most 65504^2 */
static float o_mom_hv(float v) { return fmin_c(fmax_c(0.0f, v), 65504.0f * 65504.0f); }

/* M3: the variance of the mean's luminance by each pixel's own count */
void o_mom_variance(const double *s, const uint32_t *counts, size_t pixels, int plant, float *out) {
    for (size_t p = 0; p < pixels; p++) {
        const uint32_t n = counts[p];
        if (n < 2u) {
            out[p] = 65504.0f * 65504.0f;
            continue;
        }
        const double m1 = s[p * 2 + 0] / (double)n;
        const double m2 = s[p * 2 + 1] / (double)n;
        const float m1f = (float)m1;
        const float sq = m1f * m1f;
        double d = m2 - (double)sq;
        if (plant == PLANT_SQUARE_IN_DOUBLE) d = m2 - m1 * m1;
        const double d0 = 0.0 < d ? d : 0.0; /* max(0, d), the zero first: NaN -> +0 */
        const double div = plant == PLANT_DIVISOR_N ? (double)n : (double)(n - 1u);
        out[p] = o_mom_hv((float)(d0 / div));
    }
}
