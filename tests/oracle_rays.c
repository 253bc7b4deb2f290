/* tests/oracle_rays.c -- TEST INFRASTRUCTURE ONLY: the oracle's pathTrace for rays of the caller's own (include/vrt.h
 * vrt_shade_rays).
 *
 * oracle/rt_oracle.c, included unchanged, already traces any ray: path_trace(ctx, origin, dir, mode, ...) looks the medium up at
 * floor(origin * u_voxelScale) and normalises the direction itself. o_shade_rays seeds init_rng(i % width, i / width, sample) per
 * ray, as the entry point specifies, and calls it; o_frame_rays hands back the origin and the direction o_render gives path_trace
 * for every pixel, row-major, so that o_shade_rays on them is o_render's frame (tests/test_shade_rays.py checks that). Built by
 * tests/oracle_rays.py with the oracle's own flags together with the other three oracle sources. */
#include "../oracle/rt_oracle.c"

void o_shade_rays(const o_scene *s, size_t n, const float *origins, int stride, const float *dirs, int width, int mode, int sample,
                  uint8_t *rgba8, int32_t *id_dist) {
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
        if (rgba8) { rgba8[i * 4 + 0] = unorm8(rgb[0]); rgba8[i * 4 + 1] = unorm8(rgb[1]); rgba8[i * 4 + 2] = unorm8(rgb[2]); rgba8[i * 4 + 3] = 255; }
        if (id_dist) { id_dist[i * 2 + 0] = vid; id_dist[i * 2 + 1] = dist; }
    }
}

/* o_render's ray generation (comp:624-641), one operation at a time as it has it */
void o_frame_rays(const o_scene *s, int W, int H, float *origins_out, float *dirs_out) {
    for (int py = 0; py < H; py++) {
        for (int px = 0; px < W; px++) {
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
            size_t p = (size_t)py * (size_t)W + (size_t)px;
            origins_out[p * 3 + 0] = s->cam_pos[0]; origins_out[p * 3 + 1] = s->cam_pos[1]; origins_out[p * 3 + 2] = s->cam_pos[2];
            dirs_out[p * 3 + 0] = wd.x; dirs_out[p * 3 + 1] = wd.y; dirs_out[p * 3 + 2] = wd.z;
        }
    }
}
