/* tests/oracle_samples.c -- TEST INFRASTRUCTURE ONLY: the oracle's VRT_MODE_FULL frame at any initRNG sample index.
 *
 * oracle/rt_oracle.c, included unchanged, renders sample 0 (o_render: init_rng(&c, px, py, 0), as raytracing.comp:629 does).
 * o_render_sample is o_render's loop with the sample index as a parameter and nothing else changed, so its sample 0 is
 * o_render's frame byte for byte (tests/test_accumulate.py checks that). Built by tests/oracle_samples.py with the oracle's own
 * flags together with the other three oracle sources. */
#include "../oracle/rt_oracle.c"

void o_render_sample(const o_scene *s, int W, int H, int row0, int row1, int mode, int sample, uint8_t *rgba8, int32_t *id_dist) {
    ctx_t c;
    memset(&c, 0, sizeof c);
    c.s = s;
    for (int py = row0; py < row1; py++) {
        for (int px = 0; px < W; px++) {
            c.px_fetches = 0;
            c.px_index = (uint32_t)(py * W + px);
            init_rng(&c, px, py, sample);
            float u = ((float)px / (float)W) * 2.0f - 1.0f;
            float v = ((float)py / (float)H) * 2.0f - 1.0f;
            float view[4];
            mat_vec(s->inv_proj, u, v, -1.0f, 1.0f, view);
            if (fabsf(view[3]) > 1e-6f) { float w = view[3]; view[0] /= w; view[1] /= w; view[2] /= w; view[3] /= w; }
            v3 vd = {view[0], view[1], view[2]};
            vd = normalize3(vd);
            float wd4[4];
            mat_vec(s->inv_view, vd.x, vd.y, vd.z, 0.0f, wd4);
            v3 wd = {wd4[0], wd4[1], wd4[2]};
            wd = normalize3(wd);
            v3 ro = {s->cam_pos[0], s->cam_pos[1], s->cam_pos[2]};
            float rgb[3];
            int32_t vid, dist;
            path_trace(&c, ro, wd, mode, rgb, &vid, &dist);
            size_t p = (size_t)py * (size_t)W + (size_t)px;
            if (rgba8) { rgba8[p * 4 + 0] = unorm8(rgb[0]); rgba8[p * 4 + 1] = unorm8(rgb[1]); rgba8[p * 4 + 2] = unorm8(rgb[2]); rgba8[p * 4 + 3] = 255; }
            if (id_dist) { id_dist[p * 2 + 0] = vid; id_dist[p * 2 + 1] = dist; }
        }
    }
}
