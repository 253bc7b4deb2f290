/* tests/oracle_upsample.c -- TEST INFRASTRUCTURE ONLY: the guided upsampling pass (include/vrt.h vrt_upsample_hdr, points U1-U6)
 * restated in scalar C, one high pixel at a time.
 *
 * tests/oracle_filter_hdr.c, included unchanged, brings the guided filter (o_filter_hdr: the r = 1 identity's other side), g =
 * o_filter_guide, point 2's modulation and point 3's slope, h = o_hdr_value, the tone map and o_det_expf. Every operation rounded on
 * its own: built by tests/oracle_upsample.py with oracle/Makefile's flags (no contraction).
 *
 * plant != 0 is a PLANTED MISREADING the closed forms of tests/test_upsample.py must catch:
 *   1  the offsets swapped                            2  the output modulated by the nearest low pixel's albedo
 *   3  liveness ignored                               4  ddx, ddy not scaled by r */
#include "oracle_filter_hdr.c"

typedef struct o_upsample {
    int32_t factor;
    uint32_t flags;
    float sigma_normal, sigma_albedo, sigma_depth, min_weight;
    float offset_lo_x, offset_lo_y, offset_hi_x, offset_hi_y;
} o_upsample_t;

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* U2 for the low pixel q: u = h(c) / m, m from its own planes where it is live and the flag is set */
static void low_colour(const float *rgb, const float *albedo, const float *coverage, size_t q, int demod, float u[3], float m[3]) {
    const float cov = o_filter_guide(coverage[q]);
    for (int k = 0; k < 3; k++) {
        m[k] = (demod && cov > 0.0f) ? modulation(o_filter_guide(albedo[q * 4 + k]), cov) : 1.0f;
        u[k] = o_hdr_value(rgb[q * 3 + k]) / m[k];
    }
}

/* The LOW image and planes [h][w][..], the HIGH planes [r h][r w][..]; out_rgb [H][W][3], out_rgba8 [H][W][4], out_unresolved [H][W]
 * and details [H][W][8] = fx, fy, the four tap weights w (0 where the tap was skipped), sumw, 0 -- any may be NULL. Returns 0, or -1
 * where memory runs out. */
int o_upsample(const float *rgb, const float *normal, const float *albedo, const float *depth, const float *coverage, const float *hi_normal,
               const float *hi_albedo, const float *hi_depth, const float *hi_coverage, int w, int h, const o_upsample_t *u, int op, float e,
               int plant, float *out_rgb, uint8_t *out_rgba8, uint8_t *out_unresolved, float *details) {
    const int r = u->factor, W = r * w, H = r * h;
    const size_t hpx = (size_t)W * (size_t)H;
    const int demod = (u->flags & 1u) != 0;
    const float kn = 1.0f / (u->sigma_normal * u->sigma_normal), ka = 1.0f / (u->sigma_albedo * u->sigma_albedo);
    const float rf = (float)r;
    float ohx = u->offset_hi_x, ohy = u->offset_hi_y, olx = u->offset_lo_x, oly = u->offset_lo_y;
    if (plant == 1) { ohx = u->offset_lo_x; ohy = u->offset_lo_y; olx = u->offset_hi_x; oly = u->offset_hi_y; }
    float *Z = malloc(hpx * sizeof(float));
    uint8_t *live = malloc(hpx);
    if (!Z || !live) { free(Z); free(live); return -1; }
    for (size_t p = 0; p < hpx; p++) {                                                 /* U1 on the high planes */
        Z[p] = o_filter_guide(hi_depth[p]);
        live[p] = o_filter_guide(hi_coverage[p]) > 0.0f;
    }
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            const float cov_p = o_filter_guide(hi_coverage[p]);
            const int live_p = cov_p > 0.0f;
            float np_[3], ap[4], mp[3] = {1.0f, 1.0f, 1.0f}, det[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int k = 0; k < 3; k++) np_[k] = o_filter_guide(hi_normal[p * 3 + k]);
            for (int k = 0; k < 4; k++) ap[k] = o_filter_guide(hi_albedo[p * 4 + k]);
            if (demod && live_p)                                                       /* U2 */
                for (int k = 0; k < 3; k++) mp[k] = modulation(ap[k], cov_p);
            const float gx = live_p ? slope(Z, live, p, 1, x > 0, x + 1 < W, 0) : 0.0f;
            const float gy = live_p ? slope(Z, live, p, (size_t)W, y > 0, y + 1 < H, 0) : 0.0f;
            const float fx = ((float)x + ohx) / rf - olx, fy = ((float)y + ohy) / rf - oly;            /* U3 */
            const float x0f = floorf(fx), y0f = floorf(fy), tx = fx - x0f, ty = fy - y0f;
            const int x0 = (int)x0f, y0 = (int)y0f;
            const float b[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
            float sumw = 0.0f, sum[3] = {0.0f, 0.0f, 0.0f};
            for (int k = 0; k < 4; k++) {                                              /* U4 */
                const int X = x0 + (k & 1), Y = y0 + (k >> 1);
                if (X < 0 || X >= w || Y < 0 || Y >= h) continue;
                const size_t q = (size_t)Y * w + X;
                const int live_q = o_filter_guide(coverage[q]) > 0.0f;
                if (live_q != live_p && plant != 3) continue;
                float wt = b[k];
                if (live_p) {
                    const float dx = o_filter_guide(normal[q * 3]) - np_[0], dy = o_filter_guide(normal[q * 3 + 1]) - np_[1],
                                dz = o_filter_guide(normal[q * 3 + 2]) - np_[2];
                    const float dn2 = (dx * dx + dy * dy) + dz * dz;
                    const float a0 = o_filter_guide(albedo[q * 4]) - ap[0], a1 = o_filter_guide(albedo[q * 4 + 1]) - ap[1],
                                a2 = o_filter_guide(albedo[q * 4 + 2]) - ap[2], a3 = o_filter_guide(albedo[q * 4 + 3]) - ap[3];
                    const float da2 = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
                    const float dzq = fabsf(o_filter_guide(depth[q]) - Z[p]);
                    const float sc = plant == 4 ? 1.0f : rf;
                    const float ddx = fabsf((float)X - fx) * sc, ddy = fabsf((float)Y - fy) * sc;
                    const float den = u->sigma_depth * ((gx * ddx + gy * ddy) + Z[p] * (1.0f / 256.0f)) + 0x1p-20f;
                    const float ee = (dn2 * kn + da2 * ka) + dzq / den;
                    wt = b[k] * o_det_expf(-ee);
                }
                float uq[3], mq[3];
                low_colour(rgb, albedo, coverage, q, demod, uq, mq);
                det[2 + k] = wt;
                sumw = sumw + wt;
                for (int j = 0; j < 3; j++) sum[j] = sum[j] + wt * uq[j];
            }
            det[0] = fx; det[1] = fy; det[6] = sumw;
            float up[3], mn[3];                                                        /* U5 */
            const size_t nq = (size_t)clampi((int)floorf(fy + 0.5f), 0, h - 1) * w + (size_t)clampi((int)floorf(fx + 0.5f), 0, w - 1);
            const int resolved = sumw > u->min_weight;
            if (resolved) {
                for (int j = 0; j < 3; j++) up[j] = sum[j] / sumw;
                if (plant == 2) low_colour(rgb, albedo, coverage, nq, demod, mn, mp);
            } else {
                low_colour(rgb, albedo, coverage, nq, demod, up, mn);
                if (plant == 2) memcpy(mp, mn, sizeof mn);
            }
            float fo[3];                                                               /* U6 */
            for (int j = 0; j < 3; j++) fo[j] = o_hdr_value(up[j] * mp[j]);
            if (out_rgb) memcpy(out_rgb + p * 3, fo, sizeof fo);
            if (out_rgba8) o_hdr_tonemap(fo, 1, op, e, out_rgba8 + p * 4);
            if (out_unresolved) out_unresolved[p] = resolved ? 0 : 1;
            if (details) memcpy(details + p * 8, det, sizeof det);
        }
    free(Z); free(live);
    return 0;
}
