/* tests/oracle_guides_glass.c -- TEST INFRASTRUCTURE ONLY: guides past glass (include/vrt.h vrt_set_guide_glass, rule G0-G6) restated
 * on the oracle's own march.
 *
 * tests/oracle_guides.c, included unchanged, names the surface of one march. guide_past_glass chains such marches: after a
 * translucent hit it restates comp:547-572 as rt_oracle.c path_trace has it (lines 456-516) on the oracle's own hit_marching,
 * refract3 and o_det_powf -- the alpha-0 rules, n1 and n2, the flip, the refracted direction, Fresnel's shares, the "spawns nothing"
 * test -- without the ray stack, and starts the next segment 1e-4 behind the surface in medium n2. The sums and the resolve are
 * oracle_guides.c's. Built by tests/oracle_guides_glass.py with the oracle's own flags (no contraction).
 *
 * plant: a misreading planted on purpose, so that the tests can show a comparison fails -- 1: n2 / n1 for the ratio, 2: the depth
 * taken as the straight distance from the sample's origin to the final point, 3: A taken from the final surface, 4: the 1e-4 nudge
 * applied along +normal. */
#include "oracle_guides.c"
#include "../include/vrt.h"

typedef struct {
    guide_t g;
    int32_t surfaces;   /* S: the surfaces the chain took (0: segment 0 missed) */
    int32_t vid;        /* the final surface as the shader's voxel ID: linear cell * 6 + getFaceIndex(hitNormal) */
} glass_t;

static glass_t guide_past_glass(ctx_t *c, v3 ray_origin, v3 ray_dir, int plant) {
    const o_scene *s = c->s;
    glass_t out;
    memset(&out, 0, sizeof out);
    /* G0 */
    int32_t cur = 0;
    i3 nmin = {s->bounds_min[0], s->bounds_min[1], s->bounds_min[2]};
    i3 nmax = {s->bounds_max[0], s->bounds_max[1], s->bounds_max[2]};
    v3 gro = scale3(ray_origin, s->voxel_scale);
    vox_t tv = octree_find(c, floor_i3(gro), &nmin, &nmax, &cur);
    float iof = (tv.props[0] > 0.0f && tv.props[0] < 3.0f) ? tv.props[0] : 1.0f;
    float inv_len = 1.0f / sqrtf(dot3(ray_dir, ray_dir));
    v3 dir = scale3(ray_dir, inv_len);
    v3 ow = ray_origin;
    float L = 0.0f;
    uint8_t a0 = 0;
    int S = 0;
    for (;;) {
        i3 mp = {0, 0, 0};
        v3 hp = {0, 0, 0}, hn = {0, 0, 0};
        vox_t last, hv;
        /* G1 */
        if (!hit_marching(c, gro, dir, iof, &mp, &hp, &hn, &last, &hv)) { out.surfaces = S; return out; }
        /* G2 */
        v3 normal = hn;
        if (!(len3(hn) > 0.0f)) { normal.x = 0.0f; normal.y = 1.0f; normal.z = 0.0f; }
        const v3 named = normal;   /* before the flip */
        v3 hpw = hp;
        if (s->voxel_scale != 1.0f) { hpw.x = hp.x / s->voxel_scale; hpw.y = hp.y / s->voxel_scale; hpw.z = hp.z / s->voxel_scale; }
        L = L + len3(sub3(hpw, ow));
        float sc[4];
        memcpy(sc, hv.color[3] > 0.0f ? hv.color : last.color, 16);
        if (mp.x == s->highlighted[0] && mp.y == s->highlighted[1] && mp.z == s->highlighted[2]) {
            sc[0] = 1.0f - sc[0]; sc[1] = 1.0f - sc[1]; sc[2] = 1.0f - sc[2]; sc[3] = 1.0f;
        }
        if (S == 0) a0 = unorm8(sc[3]);
        S = S + 1;
        /* G3, G4 */
        int ends = sc[3] >= 1.0f || S == VRT_GUIDE_MAX_SURFACES;
        v3 refr_dir = {0, 0, 0};
        float n2 = 1.0f;
        if (!ends) { /* G5: rt_oracle.c:460-499 */
            if (hv.color[3] <= 0.0f) { hv.props[0] = 1.0f; hv.props[1] = 0.0f; hv.props[2] = 0.0f; }
            if (last.color[3] <= 0.0f) {
                if (iof > 0.0f) { last.props[0] = last.props[1] = last.props[2] = 0.0f; }
                else { last.props[0] = 1.0f; last.props[1] = 0.0f; last.props[2] = 0.0f; }
            }
            n2 = hv.props[0] > 0.0f ? hv.props[0] : 1.0f;
            float n1 = last.props[0] > 0.0f ? last.props[0] : 1.0f;
            v3 inc = dir;
            float cosi = dot3(inc, normal);
            if (cosi > 0.0f) { normal.x = -normal.x; normal.y = -normal.y; normal.z = -normal.z; float t = n1; n1 = n2; n2 = t; }
            refr_dir = refract3(inc, normal, plant == 1 ? n2 / n1 : n1 / n2);
            float R0 = (n1 - n2) / (n1 + n2) * (n1 - n2) / (n1 + n2);
            v3 ninc = {-inc.x, -inc.y, -inc.z};
            float cos_t = fmax_c(0.0f, dot3(ninc, normal));
            float fres = R0 + (1.0f - R0) * o_det_powf(1.0f - cos_t, 5.0f);
            fres = fmin_c(fmax_c(fres, 0.0f), 1.0f);
            int has_tir = len3(refr_dir) < 0.001f;
            float reflect_i = fres;
            float refract_i = has_tir ? 0.0f : (1.0f - fres);
            ends = reflect_i <= 0.001f || refract_i <= 0.001f;
        }
        if (ends) { /* G6 */
            guide_t *g = &out.g;
            g->hit = 1;
            g->n[0] = (int32_t)named.x; g->n[1] = (int32_t)named.y; g->n[2] = (int32_t)named.z;
            for (int k = 0; k < 3; k++) g->a[k] = unorm8(sc[k]);
            g->a[3] = plant == 3 ? unorm8(sc[3]) : a0;
            g->depth = g_hdr_value(plant == 2 ? len3(sub3(hpw, ray_origin)) : L);
            g->cell[0] = mp.x; g->cell[1] = mp.y; g->cell[2] = mp.z;
            out.surfaces = S;
            out.vid = (mp.x + s->tex_dim * (mp.y + s->tex_dim * mp.z)) * 6 + face_index(hn);
            return out;
        }
        gro = plant == 4 ? add3(hp, scale3(normal, 1e-4f)) : sub3(hp, scale3(normal, 1e-4f));
        ow = gro;
        if (s->voxel_scale != 1.0f) { ow.x = gro.x / s->voxel_scale; ow.y = gro.y / s->voxel_scale; ow.z = gro.z / s->voxel_scale; }
        dir = refr_dir;
        iof = n2;
    }
}

/* o_guide_sample's outputs and, per pixel, the surface count S (int32 [H][W]) and the final surface's voxel ID (int32 [H][W], may be
 * NULL) */
void o_glass_sample(const o_scene *s, int W, int H, uint32_t sample, int jitter, float aperture, float focus, int plant, int8_t *normal,
                    uint8_t *albedo, float *depth, uint8_t *hit, int32_t *cell, int32_t *surfaces, int32_t *vid) {
    ctx_t c;
    memset(&c, 0, sizeof c);
    c.s = s;
    for (int py = 0; py < H; py++) {
        for (int px = 0; px < W; px++) {
            float o[3], d[3];
            (void)o_lens_ray(s, W, H, px, py, sample, jitter, aperture, focus, o, d);
            v3 ro = {o[0], o[1], o[2]}, wd = {d[0], d[1], d[2]};
            const glass_t g = guide_past_glass(&c, ro, wd, plant);
            const size_t p = (size_t)py * (size_t)W + (size_t)px;
            put(&g.g, p, normal, albedo, depth, hit, cell);
            surfaces[p] = g.surfaces;
            if (vid) vid[p] = g.vid;
        }
    }
}

/* ... and of n rays of the caller's own */
void o_glass_rays(const o_scene *s, size_t n, const float *origins, int stride, const float *dirs, int plant, int8_t *normal,
                  uint8_t *albedo, float *depth, uint8_t *hit, int32_t *cell, int32_t *surfaces, int32_t *vid) {
    ctx_t c;
    memset(&c, 0, sizeof c);
    c.s = s;
    for (size_t i = 0; i < n; i++) {
        const float *o = origins + (stride ? i * 3 : 0), *d = dirs + i * 3;
        v3 ro = {o[0], o[1], o[2]}, wd = {d[0], d[1], d[2]};
        const glass_t g = guide_past_glass(&c, ro, wd, plant);
        put(&g.g, i, normal, albedo, depth, hit, cell);
        surfaces[i] = g.surfaces;
        if (vid) vid[i] = g.vid;
    }
}
