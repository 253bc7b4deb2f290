/* tests/oracle_guides.c -- TEST INFRASTRUCTURE ONLY: the guide planes (include/vrt.h vrt_accum_guides, vrt_guide_rays) restated on
 * the oracle's own march.
 *
 * tests/oracle_lens.c, included unchanged (and with it oracle/rt_oracle.c), makes the ray of any sample of an accumulation -- the
 * corner's (aperture 0, no jitter), the jittered one, the thin lens's. guide_of_ray is pathTrace's prologue and its depth-0
 * hitMarching (rt_oracle.c path_trace up to comp:478) and then only what names the surface: the normal before the flip
 * (comp:497), the four bytes of surfaceColor (comp:505-507) with the highlighted voxel's inversion (comp:518-520), and the
 * distance from the ray's origin to the hit point, every operation a float32 one. Then the sums and the resolve of the header,
 * every division in float64. Built by tests/oracle_guides.py with the oracle's own flags (no contraction) together with the other
 * three oracle sources.
 *
 * plant: a misreading planted on purpose, so that the tests can show the comparison fails -- 1: the normal's sign flipped, 2: the
 * depth measured from the eye (cameraPos) instead of the sample's own origin. */
#include "oracle_lens.c"

typedef struct {
    int hit;
    int32_t n[3];       /* +1 / -1 on one axis */
    uint8_t a[4];       /* R, G, B, A bytes */
    float depth;        /* h(distance), world units */
    int32_t cell[3];    /* hitMapPos */
} guide_t;

static float g_hdr_value(float c) { return fmin_c(fmax_c(0.0f, c), 65504.0f); }

static guide_t guide_of_ray(ctx_t *c, v3 ray_origin, v3 ray_dir, int plant) {
    const o_scene *s = c->s;
    guide_t g;
    memset(&g, 0, sizeof g);
    int32_t cur = 0;
    i3 nmin = {s->bounds_min[0], s->bounds_min[1], s->bounds_min[2]};
    i3 nmax = {s->bounds_max[0], s->bounds_max[1], s->bounds_max[2]};
    v3 gro = scale3(ray_origin, s->voxel_scale);
    vox_t tv = octree_find(c, floor_i3(gro), &nmin, &nmax, &cur);
    float start_iof = (tv.props[0] > 0.0f && tv.props[0] < 3.0f) ? tv.props[0] : 1.0f;
    float inv_len = 1.0f / sqrtf(dot3(ray_dir, ray_dir));
    ray_dir = scale3(ray_dir, inv_len);
    i3 mp = {0, 0, 0};
    v3 hp = {0, 0, 0}, hn = {0, 0, 0};
    vox_t last, hv;
    if (!hit_marching(c, gro, ray_dir, start_iof, &mp, &hp, &hn, &last, &hv)) return g;
    g.hit = 1;
    v3 normal = hn;
    if (!(len3(hn) > 0.0f)) { normal.x = 0.0f; normal.y = 1.0f; normal.z = 0.0f; }
    if (plant == 1) { normal.x = -normal.x; normal.y = -normal.y; normal.z = -normal.z; }
    g.n[0] = (int32_t)normal.x; g.n[1] = (int32_t)normal.y; g.n[2] = (int32_t)normal.z;
    v3 hpw = hp;
    if (s->voxel_scale != 1.0f) { hpw.x = hp.x / s->voxel_scale; hpw.y = hp.y / s->voxel_scale; hpw.z = hp.z / s->voxel_scale; }
    v3 from = ray_origin;
    if (plant == 2) { from.x = s->cam_pos[0]; from.y = s->cam_pos[1]; from.z = s->cam_pos[2]; }
    g.depth = g_hdr_value(len3(sub3(hpw, from)));
    const float *sc = hv.color[3] > 0.0f ? hv.color : last.color;
    for (int k = 0; k < 4; k++) g.a[k] = unorm8(sc[k]);   /* the leaf's own byte: unorm8(b / 255.0f) == b */
    if (mp.x == s->highlighted[0] && mp.y == s->highlighted[1] && mp.z == s->highlighted[2]) {
        for (int k = 0; k < 3; k++) g.a[k] = (uint8_t)(255 - g.a[k]);
        g.a[3] = 255;
    }
    g.cell[0] = mp.x; g.cell[1] = mp.y; g.cell[2] = mp.z;
    return g;
}

static void put(const guide_t *g, size_t p, int8_t *normal, uint8_t *albedo, float *depth, uint8_t *hit, int32_t *cell) {
    for (int k = 0; k < 3; k++) normal[p * 3 + k] = (int8_t)g->n[k];
    for (int k = 0; k < 4; k++) albedo[p * 4 + k] = g->a[k];
    depth[p] = g->depth;
    hit[p] = (uint8_t)g->hit;
    if (cell) for (int k = 0; k < 3; k++) cell[p * 3 + k] = g->cell[k];
}

/* the guide of sample `sample` of every pixel: normal int8 [H][W][3], albedo uint8 [H][W][4], depth float [H][W], hit uint8 [H][W],
 * cell int32 [H][W][3] (may be NULL) */
void o_guide_sample(const o_scene *s, int W, int H, uint32_t sample, int jitter, float aperture, float focus, int plant, int8_t *normal,
                    uint8_t *albedo, float *depth, uint8_t *hit, int32_t *cell) {
    ctx_t c;
    memset(&c, 0, sizeof c);
    c.s = s;
    for (int py = 0; py < H; py++) {
        for (int px = 0; px < W; px++) {
            float o[3], d[3];
            (void)o_lens_ray(s, W, H, px, py, sample, jitter, aperture, focus, o, d);
            v3 ro = {o[0], o[1], o[2]}, wd = {d[0], d[1], d[2]};
            const guide_t g = guide_of_ray(&c, ro, wd, plant);
            put(&g, (size_t)py * (size_t)W + (size_t)px, normal, albedo, depth, hit, cell);
        }
    }
}

/* ... and of n rays of the caller's own */
void o_guide_rays(const o_scene *s, size_t n, const float *origins, int stride, const float *dirs, int8_t *normal, uint8_t *albedo,
                  float *depth, uint8_t *hit, int32_t *cell) {
    ctx_t c;
    memset(&c, 0, sizeof c);
    c.s = s;
    for (size_t i = 0; i < n; i++) {
        const float *o = origins + (stride ? i * 3 : 0), *d = dirs + i * 3;
        v3 ro = {o[0], o[1], o[2]}, wd = {d[0], d[1], d[2]};
        const guide_t g = guide_of_ray(&c, ro, wd, 0);
        put(&g, i, normal, albedo, depth, hit, cell);
    }
}

/* one sample's guides into the state of `pixels` pixels: asum uint32 [.][4], nsum int32 [.][3], hits uint32 [.], dsum double [.];
 * a miss adds nothing */
void o_guide_add(size_t pixels, const int8_t *normal, const uint8_t *albedo, const float *depth, const uint8_t *hit, uint32_t *asum,
                 int32_t *nsum, uint32_t *hits, double *dsum) {
    for (size_t p = 0; p < pixels; p++) {
        if (!hit[p]) continue;
        for (int k = 0; k < 4; k++) asum[p * 4 + k] += albedo[p * 4 + k];
        for (int k = 0; k < 3; k++) nsum[p * 3 + k] += normal[p * 3 + k];
        hits[p] += 1u;
        dsum[p] = dsum[p] + (double)g_hdr_value(depth[p]);
    }
}

/* the planes of n samples: every division in float64, one rounding to float32 */
void o_guide_resolve(size_t pixels, uint32_t n, const uint32_t *asum, const int32_t *nsum, const uint32_t *hits, const double *dsum,
                     float *normal, float *albedo, float *depth, float *coverage) {
    for (size_t p = 0; p < pixels; p++) {
        for (int k = 0; k < 3; k++) normal[p * 3 + k] = (float)((double)nsum[p * 3 + k] / (double)n);
        for (int k = 0; k < 4; k++) albedo[p * 4 + k] = (float)((double)asum[p * 4 + k] / (255.0 * (double)n));
        coverage[p] = (float)((double)hits[p] / (double)n);
        depth[p] = hits[p] ? (float)(dsum[p] / (double)hits[p]) : 0.0f;
    }
}
