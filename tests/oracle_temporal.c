/* tests/oracle_temporal.c -- TEST INFRASTRUCTURE ONLY: the temporal pass (include/vrt.h vrt_temporal_hdr, points T1-T6) restated in
 * scalar C, one pixel at a time.
 *
 * tests/oracle_filter_var.c, included unchanged, brings the variance-guided filter the accumulation forms chain the pass with
 * (o_filter_var), g = o_filter_guide, hv = o_filter_var_value, V1's lum, h = o_hdr_value, and through oracle/rt_oracle.c mat_vec,
 * normalize3 and the min / max conventions. Every operation rounded on its own: built by tests/oracle_temporal.py with
 * oracle/Makefile's flags (no contraction).
 *
 * plant != 0 is a PLANTED MISREADING the closed forms of tests/test_temporal.py must catch:
 *   1  the offset not subtracted from fx, fy          2  the previous quantities not divided by sw
 *   3  Zexp taken from the current eye                4  the variance not divided by N' - 1 */
#include "oracle_filter_var.c"

typedef struct o_temporal {
    float prev_view_proj[16], prev_camera_pos[4];
    float offset_x, offset_y;
    int32_t max_history;
    float alpha_min, alpha_moments_min, normal_min, depth_tol;
} o_temporal_t;

/* T1: the ray pathTrace marches through (fx, fy): main()'s ray generation (comp:624-641), then pathTrace's own normalisation */
static v3 temporal_ray(const float *inv_proj, const float *inv_view, int W, int H, float fx, float fy) {
    float u = (fx / (float)W) * 2.0f - 1.0f;
    float v = (fy / (float)H) * 2.0f - 1.0f;
    float view[4];
    mat_vec(inv_proj, u, v, -1.0f, 1.0f, view);
    if (fabsf(view[3]) > 1e-6f) { float w = view[3]; view[0] /= w; view[1] /= w; view[2] /= w; view[3] /= w; }
    v3 vd = {view[0], view[1], view[2]};
    vd = normalize3(vd);
    float wd4[4];
    mat_vec(inv_view, vd.x, vd.y, vd.z, 0.0f, wd4);
    v3 wd = {wd4[0], wd4[1], wd4[2]};
    wd = normalize3(wd);
    return scale3(wd, 1.0f / sqrtf(dot3(wd, wd)));
}

/* The camera block in vrt_set_camera's shapes, the planes as o_filter_var takes them (no albedo), hist_in [3][H][W][4] or NULL (the
 * first frame); hist_out [3][H][W][4]; out_rgb [H][W][3], out_var [H][W] and details [H][W][8] = fx, fy, Zexp, the four tap
 * verdicts (1 or 0) and sw (zeros where T2 was not reached) may be NULL. */
void o_temporal(const float *inv_proj, const float *inv_view, const float *cam_pos, const float *rgb, const float *normal, const float *depth,
                const float *coverage, const float *hist_in, int W, int H, const o_temporal_t *t, int plant, float *hist_out, float *out_rgb,
                float *out_var, float *details) {
    const size_t px = (size_t)W * (size_t)H;
    const float nmax = (float)t->max_history;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            float *h0 = hist_out + p * 4, *h1 = hist_out + (px + p) * 4, *h2 = hist_out + (2 * px + p) * 4;
            float c[3], det[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int k = 0; k < 3; k++) c[k] = o_hdr_value(rgb[p * 3 + k]);
            const float cov = o_filter_guide(coverage[p]);
            if (!(cov > 0.0f)) {
                h0[0] = c[0]; h0[1] = c[1]; h0[2] = c[2]; h0[3] = 0.0f;
                for (int k = 0; k < 4; k++) h1[k] = h2[k] = 0.0f;
                if (out_rgb) memcpy(out_rgb + p * 3, c, sizeof c);
                if (out_var) out_var[p] = 0.0f;
                if (details) memcpy(details + p * 8, det, sizeof det);
                continue;
            }
            const float np_[3] = {o_filter_guide(normal[p * 3]), o_filter_guide(normal[p * 3 + 1]), o_filter_guide(normal[p * 3 + 2])};
            const float Zp = o_filter_guide(depth[p]);
            float sw = 0.0f, sc[3] = {0.0f, 0.0f, 0.0f}, sn = 0.0f, s1 = 0.0f, s2 = 0.0f;
            if (hist_in) {
                v3 d = temporal_ray(inv_proj, inv_view, W, H, (float)x + t->offset_x, (float)y + t->offset_y);   /* T1 */
                v3 P = {cam_pos[0] + Zp * d.x, cam_pos[1] + Zp * d.y, cam_pos[2] + Zp * d.z};
                float clip[4];                                                                                  /* T2 */
                mat_vec(t->prev_view_proj, P.x, P.y, P.z, 1.0f, clip);
                if (clip[3] > 1e-6f) {
                    float fx = (((clip[0] / clip[3]) + 1.0f) * 0.5f) * (float)W, fy = (((clip[1] / clip[3]) + 1.0f) * 0.5f) * (float)H;
                    if (plant != 1) { fx = fx - t->offset_x; fy = fy - t->offset_y; }
                    v3 from = {t->prev_camera_pos[0], t->prev_camera_pos[1], t->prev_camera_pos[2]};
                    if (plant == 3) { from.x = cam_pos[0]; from.y = cam_pos[1]; from.z = cam_pos[2]; }
                    v3 dp = sub3(P, from);
                    const float Zexp = sqrtf((dp.x * dp.x + dp.y * dp.y) + dp.z * dp.z);
                    det[0] = fx; det[1] = fy; det[2] = Zexp;
                    if (fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H) {
                        const float x0f = floorf(fx), y0f = floorf(fy), tx = fx - x0f, ty = fy - y0f;
                        const int x0 = (int)x0f, y0 = (int)y0f;
                        const float wt[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
                        for (int k = 0; k < 4; k++) {                                                          /* T3 */
                            const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                            const size_t q = (size_t)qy * W + qx;
                            const float *q0 = hist_in + q * 4, *q1 = hist_in + (px + q) * 4, *q2 = hist_in + (2 * px + q) * 4;
                            const float Nq = fmin_c(fmax_c(0.0f, o_filter_guide(q0[3])), nmax);
                            const float Zq = o_filter_guide(q1[2]), Cq = o_filter_guide(q1[3]);
                            const float nq[3] = {o_filter_guide(q2[0]), o_filter_guide(q2[1]), o_filter_guide(q2[2])};
                            const float nd = (nq[0] * np_[0] + nq[1] * np_[1]) + nq[2] * np_[2];
                            if (!(Cq > 0.0f) || !(Nq >= 1.0f) || !(nd >= t->normal_min)) continue;
                            if (!(fabsf(Zq - Zexp) <= t->depth_tol * Zexp + 0x1p-20f)) continue;
                            det[3 + k] = 1.0f;
                            sw = sw + wt[k];
                            for (int j = 0; j < 3; j++) sc[j] = sc[j] + wt[k] * o_hdr_value(q0[j]);
                            sn = sn + wt[k] * Nq;
                            s1 = s1 + wt[k] * o_hdr_value(q1[0]);
                            s2 = s2 + wt[k] * o_filter_var_value(q1[1]);
                        }
                        det[7] = sw;
                    }
                }
            }
            float cp[3] = {0.0f, 0.0f, 0.0f}, Nprev = 0.0f, m1p = 0.0f, m2p = 0.0f;
            if (sw > 0.0f) {
                const float div = plant == 2 ? 1.0f : sw;
                for (int j = 0; j < 3; j++) cp[j] = sc[j] / div;
                Nprev = sn / div; m1p = s1 / div; m2p = s2 / div;
            }
            const float Nn = fmin_c(Nprev + 1.0f, nmax);                                                        /* T4 */
            const float a = fmax_c(1.0f / Nn, t->alpha_min), am = fmax_c(1.0f / Nn, t->alpha_moments_min);
            float cn[3];                                                                                        /* T5 */
            for (int j = 0; j < 3; j++) cn[j] = cp[j] + a * (c[j] - cp[j]);
            const float Y = lum(c);
            const float m1 = m1p + am * (Y - m1p), m2 = m2p + am * (Y * Y - m2p);
            h0[0] = cn[0]; h0[1] = cn[1]; h0[2] = cn[2]; h0[3] = Nn;                                            /* T6 */
            h1[0] = m1; h1[1] = m2; h1[2] = Zp; h1[3] = cov;
            h2[0] = np_[0]; h2[1] = np_[1]; h2[2] = np_[2]; h2[3] = 0.0f;
            if (out_rgb) memcpy(out_rgb + p * 3, cn, sizeof cn);
            if (out_var) {
                const float spread = fmax_c(0.0f, m2 - m1 * m1);
                out_var[p] = Nn >= 2.0f ? o_filter_var_value(plant == 4 ? spread : spread / (Nn - 1.0f)) : 65504.0f * 65504.0f;
            }
            if (details) memcpy(details + p * 8, det, sizeof det);
        }
}
