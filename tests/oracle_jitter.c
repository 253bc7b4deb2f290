/* tests/oracle_jitter.c -- TEST INFRASTRUCTURE ONLY: the oracle's frame at any jittered sample of the progressive accumulation.
 *
 * oracle/rt_oracle.c, included unchanged, renders the frame (o_render: the ray through the pixel's corner, init_rng(&c, px, py, 0)).
 * o_render_jittered is o_render's loop with two additions and nothing else changed: init_rng takes the sample index, and with
 * `jitter` the pixel's float(px) and float(py) become float(px) + jx(sample) and float(py) + jy(sample) (include/vrt.h
 * VRT_ACCUM_JITTER). Its sample 0 is o_render's frame byte for byte (tests/test_accum_jitter.py checks that). Built by
 * tests/oracle_jitter.py with the oracle's own flags (no contraction) together with the other three oracle sources. */
#include "../oracle/rt_oracle.c"

static uint32_t bitreverse32(uint32_t x) {
    uint32_t r = 0;
    for (int i = 0; i < 32; i++, x >>= 1) r = (r << 1) | (x & 1u);
    return r;
}

static uint32_t sobol2(uint32_t k) {
    uint32_t y = 0, v = 1u << 31;
    for (uint32_t i = k; i; i >>= 1, v ^= v >> 1)
        if (i & 1u) y ^= v;
    return y;
}

void o_jitter_offsets(uint32_t k, float *jx, float *jy) {
    *jx = (float)(bitreverse32(k) >> 8) * 0x1p-24f;
    *jy = (float)(sobol2(k) >> 8) * 0x1p-24f;
}

void o_render_jittered(const o_scene *s, int W, int H, int row0, int row1, int mode, uint32_t sample, int jitter, uint8_t *rgba8,
                       int32_t *id_dist) {
    ctx_t c;
    memset(&c, 0, sizeof c);
    c.s = s;
    float jx = 0.0f, jy = 0.0f;
    if (jitter) o_jitter_offsets(sample, &jx, &jy);
    for (int py = row0; py < row1; py++) {
        for (int px = 0; px < W; px++) {
            c.px_fetches = 0;
            c.px_index = (uint32_t)(py * W + px);
            init_rng(&c, px, py, (int)sample);
            const float fx = jitter ? (float)px + jx : (float)px;
            const float fy = jitter ? (float)py + jy : (float)py;
            float u = (fx / (float)W) * 2.0f - 1.0f;
            float v = (fy / (float)H) * 2.0f - 1.0f;
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
