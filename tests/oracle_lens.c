/* tests/oracle_lens.c -- TEST INFRASTRUCTURE ONLY: the oracle's frame at any thin-lens sample of the progressive accumulation.
 *
 * oracle/rt_oracle.c, included unchanged, renders the frame (o_render: the ray through the pixel's corner from the eye).
 * o_render_lens is o_render's loop (as tests/oracle_jitter.c has it: init_rng with the sample index, optional sub-pixel
 * jitter) with the ray moved to the lens sample of include/vrt.h vrt_set_lens: origin o on the lens, direction through the
 * point where the pinhole ray meets the plane of focus. path_trace takes the origin and looks the medium up there itself
 * (rt_oracle.c path_trace: octree_find at floor(o * u_voxelScale)). Its sample 0, and every sample at aperture 0, is
 * oracle_jitter.c's sample byte for byte (tests/test_accum_lens.py checks that). Built by tests/oracle_lens.py with the
 * oracle's own flags (no contraction) together with the other three oracle sources. */
#include "../oracle/rt_oracle.c"

static uint32_t lbitreverse32(uint32_t x) {
    uint32_t r = 0;
    for (int i = 0; i < 32; i++, x >>= 1) r = (r << 1) | (x & 1u);
    return r;
}

static uint32_t lsobol2(uint32_t k) {
    uint32_t y = 0, v = 1u << 31;
    for (uint32_t i = k; i; i >>= 1, v ^= v >> 1)
        if (i & 1u) y ^= v;
    return y;
}

/* include/vrt.h vrt_set_lens, point 2: poly 1 is x^3+x+1, poly 2 is x^3+x^2+1 */
static void lens_dirs(uint32_t poly, const uint32_t m[3], uint32_t v[32]) {
    for (int i = 0; i < 3; i++) v[i] = m[i] << (31 - i);
    for (int i = 3; i < 32; i++) {
        uint32_t x = v[i - 3] ^ (v[i - 3] >> 3);
        if (poly & 2u) x ^= v[i - 1];
        if (poly & 1u) x ^= v[i - 2];
        v[i] = x;
    }
}

static uint32_t gmul(const uint32_t D[32], uint32_t k) {
    uint32_t y = 0;
    for (int i = 0; k; i++, k >>= 1)
        if (k & 1u) y ^= D[i];
    return y;
}

/* (lu, lv) of sample k in [0,1)^2 */
void o_lens_uv(uint32_t k, float *lu, float *lv) {
    static const uint32_t mu[3] = {1, 1, 5}, mv[3] = {1, 3, 1};
    uint32_t U[32], V[32];
    lens_dirs(1, mu, U);
    lens_dirs(2, mv, V);
    *lu = (float)((gmul(U, k) >> 8) ^ 0x800000u) * 0x1p-24f;
    *lv = (float)((gmul(V, k) >> 8) ^ 0x800000u) * 0x1p-24f;
}

/* point 3: the concentric map of (lu, lv) to the unit disc */
void o_lens_point(uint32_t k, float *lx, float *ly) {
    float lu, lv;
    o_lens_uv(k, &lu, &lv);
    const float a = 2.0f * lu - 1.0f, b = 2.0f * lv - 1.0f;
    *lx = *ly = 0.0f;
    if (a == 0.0f && b == 0.0f) return;
    float r, phi;
    if (fabsf(a) > fabsf(b)) { r = a; phi = 0.785398163f * (b / a); }
    else { r = b; phi = 1.57079633f - 0.785398163f * (a / b); }
    float s, c;
    det_sincos(phi, &s, &c);
    *lx = r * c;
    *ly = r * s;
}

/* points 1, 4, 5: the ray of pixel (px, py) at sample k; o[3], dir[3] out. Returns 1 when the lens moved it, 0 for the pinhole ray. */
int o_lens_ray(const o_scene *s, int W, int H, int px, int py, uint32_t sample, int jitter, float aperture, float focus, float *o,
               float *dir) {
    float jx = 0.0f, jy = 0.0f;
    if (jitter) {
        jx = (float)(lbitreverse32(sample) >> 8) * 0x1p-24f;
        jy = (float)(lsobol2(sample) >> 8) * 0x1p-24f;
    }
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
    v3 d = {wd4[0], wd4[1], wd4[2]};
    d = normalize3(d);
    const v3 e = {s->cam_pos[0], s->cam_pos[1], s->cam_pos[2]};
    o[0] = e.x; o[1] = e.y; o[2] = e.z;
    dir[0] = d.x; dir[1] = d.y; dir[2] = d.z;
    float lx, ly;
    o_lens_point(sample, &lx, &ly);
    const float *iv = s->inv_view;
    const v3 R = {iv[0], iv[1], iv[2]}, U = {iv[4], iv[5], iv[6]}, Z = {iv[8], iv[9], iv[10]};
    const float cosd = -((d.x * Z.x + d.y * Z.y) + d.z * Z.z);
    if (aperture == 0.0f || (lx == 0.0f && ly == 0.0f) || !(cosd > 0.0f)) return 0;
    const float sx = aperture * lx, sy = aperture * ly;
    const v3 oo = {(e.x + sx * R.x) + sy * U.x, (e.y + sx * R.y) + sy * U.y, (e.z + sx * R.z) + sy * U.z};
    const float t = focus / cosd;
    const v3 p = {e.x + t * d.x, e.y + t * d.y, e.z + t * d.z};
    const v3 nd = normalize3(sub3(p, oo));
    o[0] = oo.x; o[1] = oo.y; o[2] = oo.z;
    dir[0] = nd.x; dir[1] = nd.y; dir[2] = nd.z;
    return 1;
}

void o_render_lens(const o_scene *s, int W, int H, int row0, int row1, int mode, uint32_t sample, int jitter, float aperture,
                   float focus, uint8_t *rgba8, int32_t *id_dist) {
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
            if (rgba8) { rgba8[p * 4 + 0] = unorm8(rgb[0]); rgba8[p * 4 + 1] = unorm8(rgb[1]); rgba8[p * 4 + 2] = unorm8(rgb[2]); rgba8[p * 4 + 3] = 255; }
            if (id_dist) { id_dist[p * 2 + 0] = vid; id_dist[p * 2 + 1] = dist; }
        }
    }
}
