/* tests/oracle_rays_hdr.c -- TEST INFRASTRUCTURE ONLY: the oracle's FLOAT colour for rays of the caller's own (include/vrt.h
 * vrt_shade_rays_hdr).
 *
 * o_shade_rays_hdr is tests/oracle_rays.c's o_shade_rays with the three floats path_trace returns stored as they are instead of
 * through unorm8 (unorm8 of them is o_shade_rays's bytes: tests/test_shade_rays_hdr.py checks that). h(c), the sequential float64
 * sum, the product that stands for it, the mean and the tone maps are tests/oracle_hdr.c's, included unchanged (and with it
 * oracle/rt_oracle.c) -- nothing of the arithmetic is restated here. Built by tests/oracle_rays_hdr.py with the oracle's own
 * flags (no contraction) together with the other three oracle sources. */
#include "oracle_hdr.c"

void o_shade_rays_hdr(const o_scene *s, size_t n, const float *origins, int stride, const float *dirs, int width, int mode, int sample,
                      float *rgb_out, int32_t *id_dist) {
    ctx_t c;
    memset(&c, 0, sizeof c);
    c.s = s;
    for (size_t i = 0; i < n; i++) {
        c.px_fetches = 0;
        c.px_index = (uint32_t)i;
        init_rng(&c, (int)(i % (size_t)width), (int)(i / (size_t)width), sample);
        const float *o = origins + (stride ? i * 3 : 0), *d = dirs + i * 3;
        v3 ro = {o[0], o[1], o[2]}, wd = {d[0], d[1], d[2]};
        float rgb[3];
        int32_t vid, dist;
        path_trace(&c, ro, wd, mode, rgb, &vid, &dist);
        if (rgb_out) { rgb_out[i * 3 + 0] = rgb[0]; rgb_out[i * 3 + 1] = rgb[1]; rgb_out[i * 3 + 2] = rgb[2]; }
        if (id_dist) { id_dist[i * 2 + 0] = vid; id_dist[i * 2 + 1] = dist; }
    }
}
