/* tests/oracle_temporal_mom.c -- TEST INFRASTRUCTURE ONLY: the temporal pass with measured variances and a 3 x 3 search (include/vrt.h
 * vrt_temporal_hdr_mom: T1, T2, T3, T3s, T4, T5, T7, T6m) restated in scalar C, one pixel at a time.
 *
 * tests/oracle_temporal.c, included unchanged, brings o_temporal_t, temporal_ray (T1) and everything it includes itself. Every
 * operation rounded on its own: built by tests/oracle_temporal_mom.py with oracle/Makefile's flags (no contraction).
 *
 * plant != 0 is a PLANTED MISREADING the closed forms of tests/test_temporal_mom.py must catch:
 *   1  V' = a * a * v, the (1 - a)^2 * Vp term dropped        2  bilinear weights about (fx, fy) kept in the search (the taps
 *      that carry any have just failed: it finds nothing)
 *   3  the search's centre by floorf(fx), not floorf(fx + 0.5f) 4  the switch of T6m on Nprev in place of N' */
#include "oracle_temporal.c"

typedef struct o_temporal_mom {
    o_temporal_t t;
    int32_t measured_below, search;
} o_temporal_mom_t;

/* T3's tests of one tap (qx, qy); where it counts, its seven quantities h(r), h(g), h(b), N, h(m1), hv(m2), hv(V) into xq */
static int mom_tap(const float *hist_in, int W, int H, int qx, int qy, const float *np_, float Zexp, const o_temporal_t *t, float *xq) {
    if (qx < 0 || qx >= W || qy < 0 || qy >= H) return 0;
    const size_t px = (size_t)W * (size_t)H, q = (size_t)qy * W + qx;
    const float *q0 = hist_in + q * 4, *q1 = hist_in + (px + q) * 4, *q2 = hist_in + (2 * px + q) * 4;
    const float Nq = fmin_c(fmax_c(0.0f, o_filter_guide(q0[3])), (float)t->max_history);
    const float Zq = o_filter_guide(q1[2]), Cq = o_filter_guide(q1[3]);
    const float nq[3] = {o_filter_guide(q2[0]), o_filter_guide(q2[1]), o_filter_guide(q2[2])};
    const float nd = (nq[0] * np_[0] + nq[1] * np_[1]) + nq[2] * np_[2];
    if (!(Cq > 0.0f) || !(Nq >= 1.0f) || !(nd >= t->normal_min)) return 0;
    if (!(fabsf(Zq - Zexp) <= t->depth_tol * Zexp + 0x1p-20f)) return 0;
    xq[0] = o_hdr_value(q0[0]); xq[1] = o_hdr_value(q0[1]); xq[2] = o_hdr_value(q0[2]);
    xq[3] = Nq;
    xq[4] = o_hdr_value(q1[0]);
    xq[5] = o_filter_var_value(q1[1]);
    xq[6] = o_filter_var_value(q2[3]);
    return 1;
}

/* o_temporal's arguments with var_in [H][W] or NULL before hist_in and an o_temporal_mom_t; details [H][W][10] = o_temporal's eight
 * (sw: T3's), then whether the search ran (1 or 0) and how many of its taps counted. */
void o_temporal_mom(const float *inv_proj, const float *inv_view, const float *cam_pos, const float *rgb, const float *normal,
                    const float *depth, const float *coverage, const float *var_in, const float *hist_in, int W, int H,
                    const o_temporal_mom_t *tm, int plant, float *hist_out, float *out_rgb, float *out_var, float *details) {
    const o_temporal_t *t = &tm->t;
    const size_t px = (size_t)W * (size_t)H;
    const float nmax = (float)t->max_history, unknown = 65504.0f * 65504.0f;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            float *h0 = hist_out + p * 4, *h1 = hist_out + (px + p) * 4, *h2 = hist_out + (2 * px + p) * 4;
            float c[3], det[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int k = 0; k < 3; k++) c[k] = o_hdr_value(rgb[p * 3 + k]);
            const float cov = o_filter_guide(coverage[p]);
            if (!(cov > 0.0f)) {
                h0[0] = c[0]; h0[1] = c[1]; h0[2] = c[2]; h0[3] = 0.0f;
                for (int k = 0; k < 4; k++) h1[k] = h2[k] = 0.0f;
                if (out_rgb) memcpy(out_rgb + p * 3, c, sizeof c);
                if (out_var) out_var[p] = 0.0f;
                if (details) memcpy(details + p * 10, det, sizeof det);
                continue;
            }
            const float np_[3] = {o_filter_guide(normal[p * 3]), o_filter_guide(normal[p * 3 + 1]), o_filter_guide(normal[p * 3 + 2])};
            const float Zp = o_filter_guide(depth[p]);
            float sw = 0.0f, s[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, xq[7];
            if (hist_in) {
                v3 d = temporal_ray(inv_proj, inv_view, W, H, (float)x + t->offset_x, (float)y + t->offset_y);   /* T1 */
                v3 P = {cam_pos[0] + Zp * d.x, cam_pos[1] + Zp * d.y, cam_pos[2] + Zp * d.z};
                float clip[4];                                                                                  /* T2 */
                mat_vec(t->prev_view_proj, P.x, P.y, P.z, 1.0f, clip);
                if (clip[3] > 1e-6f) {
                    const float fx = (((clip[0] / clip[3]) + 1.0f) * 0.5f) * (float)W - t->offset_x;
                    const float fy = (((clip[1] / clip[3]) + 1.0f) * 0.5f) * (float)H - t->offset_y;
                    v3 from = {t->prev_camera_pos[0], t->prev_camera_pos[1], t->prev_camera_pos[2]};
                    v3 dp = sub3(P, from);
                    const float Zexp = sqrtf((dp.x * dp.x + dp.y * dp.y) + dp.z * dp.z);
                    det[0] = fx; det[1] = fy; det[2] = Zexp;
                    if (fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H) {
                        const float x0f = floorf(fx), y0f = floorf(fy), tx = fx - x0f, ty = fy - y0f;
                        const int x0 = (int)x0f, y0 = (int)y0f;
                        const float wt[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
                        for (int k = 0; k < 4; k++) {                                                          /* T3 */
                            if (!mom_tap(hist_in, W, H, x0 + (k & 1), y0 + (k >> 1), np_, Zexp, t, xq)) continue;
                            det[3 + k] = 1.0f;
                            sw = sw + wt[k];
                            for (int j = 0; j < 7; j++) s[j] = s[j] + wt[k] * xq[j];
                        }
                        det[7] = sw;
                        if (tm->search == 1 && sw == 0.0f) {                                                   /* T3s */
                            const int xc = (int)floorf(plant == 3 ? fx : fx + 0.5f), yc = (int)floorf(plant == 3 ? fy : fy + 0.5f);
                            det[8] = 1.0f;
                            for (int j = 0; j < 7; j++) s[j] = 0.0f;
                            for (int dy = -1; dy <= 1; dy++)
                                for (int dx = -1; dx <= 1; dx++) {
                                    if (!mom_tap(hist_in, W, H, xc + dx, yc + dy, np_, Zexp, t, xq)) continue;
                                    float wq = 1.0f;
                                    if (plant == 2) wq = fmax_c(0.0f, 1.0f - fabsf((float)(xc + dx) - fx)) * fmax_c(0.0f, 1.0f - fabsf((float)(yc + dy) - fy));
                                    det[9] = det[9] + 1.0f;
                                    sw = sw + wq;
                                    for (int j = 0; j < 7; j++) s[j] = s[j] + (plant == 2 ? wq * xq[j] : xq[j]);
                                }
                        }
                    }
                }
            }
            float prev[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (sw > 0.0f)
                for (int j = 0; j < 7; j++) prev[j] = s[j] / sw;
            const float Nprev = prev[3], m1p = prev[4], m2p = prev[5], Vp = prev[6];
            const float Nn = fmin_c(Nprev + 1.0f, nmax);                                                        /* T4 */
            const float a = fmax_c(1.0f / Nn, t->alpha_min), am = fmax_c(1.0f / Nn, t->alpha_moments_min);
            float cn[3];                                                                                        /* T5 */
            for (int j = 0; j < 3; j++) cn[j] = prev[j] + a * (c[j] - prev[j]);
            const float Y = lum(c);
            const float m1 = m1p + am * (Y - m1p), m2 = m2p + am * (Y * Y - m2p);
            const float v = var_in ? o_filter_var_value(var_in[p]) : unknown;                                   /* T7 */
            const float om = 1.0f - a;
            const float Vn = o_filter_var_value(plant == 1 ? (a * a) * v : (om * om) * Vp + (a * a) * v);
            h0[0] = cn[0]; h0[1] = cn[1]; h0[2] = cn[2]; h0[3] = Nn;                                            /* T6m */
            h1[0] = m1; h1[1] = m2; h1[2] = Zp; h1[3] = cov;
            h2[0] = np_[0]; h2[1] = np_[1]; h2[2] = np_[2]; h2[3] = Vn;
            if (out_rgb) memcpy(out_rgb + p * 3, cn, sizeof cn);
            if (out_var) {
                const float spread = fmax_c(0.0f, m2 - m1 * m1);
                const float t6 = Nn >= 2.0f ? o_filter_var_value(spread / (Nn - 1.0f)) : unknown;
                out_var[p] = (plant == 4 ? Nprev : Nn) < (float)tm->measured_below ? Vn : t6;
            }
            if (details) memcpy(details + p * 10, det, sizeof det);
        }
}
