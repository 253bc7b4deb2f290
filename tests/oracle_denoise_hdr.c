/* tests/oracle_denoise_hdr.c -- TEST INFRASTRUCTURE ONLY: the HDR display pass (include/vrt.h vrt_denoise_hdr, points 1-3) restated
 * in scalar C: quad.frag:22-83 on a float image, every float through h(c), then the tone map.
 *
 * tests/oracle_hdr.c, included unchanged, supplies h (o_hdr_value), the tone map and unorm8 (o_hdr_tonemap); o_denoise of
 * oracle/rt_oracle.c is the byte pass this one must equal on byte / 255.0f images. Every operation rounded on its own: built by
 * tests/oracle_denoise_hdr.py with tests/oracle_hdr.py's flags (no contraction). */
#include "oracle_hdr.c"

/* rgb [H][W][3] floats, id_dist [H][W][2]; out_rgb [H][W][3] and out_rgba8 [H][W][4], either may be NULL */
void o_denoise_hdr(const float *rgb, const int32_t *id_dist, int W, int H, int op, float e, float *out_rgb, uint8_t *out_rgba8) {
    for (int py = 0; py < H; py++)
        for (int px = 0; px < W; px++) {
            size_t p = (size_t)py * W + px;
            int center_id = id_dist[p * 2], center_dist = id_dist[p * 2 + 1];
            float f[3];
            if (center_id == 0) {                                                                 /* quad.frag:36-39 */
                for (int k = 0; k < 3; k++) f[k] = o_hdr_value(rgb[p * 3 + k]);
            } else {
                float radius_f = 200.0f / sqrtf((float)(center_dist > 1 ? center_dist : 1));       /* :45 */
                int R = (int)radius_f;
                R = R < 1 ? 1 : (R > 20 ? 20 : R);                                                    /* :48 */
                float sum[3] = {0.0f, 0.0f, 0.0f}, count = 0.0f;
                for (int y = -R; y <= R; y++)
                    for (int x = -R; x <= R; x++) {
                        int nx = px + x, ny = py + y;
                        if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;                         /* :60-63 */
                        size_t q = (size_t)ny * W + nx;
                        if (id_dist[q * 2] == center_id) {                                            /* :67-73 */
                            sum[0] = sum[0] + o_hdr_value(rgb[q * 3 + 0]);
                            sum[1] = sum[1] + o_hdr_value(rgb[q * 3 + 1]);
                            sum[2] = sum[2] + o_hdr_value(rgb[q * 3 + 2]);
                            count = count + 1.0f;
                        }
                    }
                float d = fmax_c(count, 1.0f);                                                        /* :78 */
                for (int k = 0; k < 3; k++) f[k] = sum[k] / d;
            }
            if (out_rgb)
                for (int k = 0; k < 3; k++) out_rgb[p * 3 + k] = f[k];
            if (out_rgba8) o_hdr_tonemap(f, 1, op, e, out_rgba8 + p * 4);
        }
}
