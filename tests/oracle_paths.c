/* tests/oracle_paths.c -- TEST INFRASTRUCTURE ONLY: the one checker of the five path rules of VRT_MODE_FULL (include/vrt.h).
 *
 * oracle/rt_oracle.c is included unchanged. path_trace_paths() is its path_trace loop with each rule at its one place, and
 * o_shade_rays_paths is the one entry point. The rules, and the arguments that switch each one off:
 *
 * 1. Path depth (vrt_set_path_depth), `depth` D in 1 .. 8: depth 0 and the inner vertices 1 <= d < D take the depth-0 operations,
 *    d == D the shader's terminal branch. Off at D = 1: the oracle's own loop.
 * 2. Sun disc (vrt_set_sun_disc), `tan_radius` > 0: a shadowing vertex first draws its own light direction (two draws, the
 *    concentric map, the basis). Off at tan_radius 0: nothing is drawn and the shadow ray goes towards lightDir.
 * 3. Emitter sampling (vrt_set_emitter_sampling), `n_emit` > 0: after the sun's direct term a shadowing vertex spends four draws on
 *    a connection to the list -- emitter, face, point -- and adds E * g with g = cs * cl * (n * 6 * size^2) / (PI * r2); a ray of
 *    depth >= 1 that hits an emissive voxel adds nothing. Off at n_emit 0: nothing is drawn, and neither rule below is read.
 * 4. Emitter importance (vrt_set_emitter_importance), `mode` 1 (VRT_EMIT_POWER): the vertex picks emitter j by the thresholds T --
 *    which o_shade_rays_paths computes from the weights itself, in exact integers; it never sees the product's table -- and the face
 *    among the m faces turned towards x = hitPoint + normal * 1e-1; m == 0 ends the vertex's sampling with the four draws spent. From
 *    q on the steps are rule 3's; the weight is g = cs * cl * (m * size^2) / (PI * r2 * p). Off at mode 0 (VRT_EMIT_UNIFORM): the
 *    weights are not read.
 * 5. Emitter MIS (vrt_set_emitter_mis), `mis` 1 at mode 1: the connection that would add E * g adds (E * g) * wn with wn = pl /
 *    (pl + pb), nothing where !(pl > 0), and a ray of depth >= 1 that hits an emissive voxel adds its emissive term times wb = pb /
 *    (pl + pb), 1 where !(pl > 0). mis_density() is the header's emit_mis_density: it is given the hit alone -- point, axis, cell and
 *    the voxel's colour and illumination bytes -- and inv_power, which o_shade_rays_paths computes from the weights itself. Off at
 *    mis 0, and at mode 0.
 *
 * `flaw` plants one misreading of a rule, for the tests that show that an expectation test can tell. O_FLAW_NONE is the rule; every
 * other value names one flaw, of rule 4's g or of rule 5's bounce side (the enum below).
 *
 * The log has one record type, o_path_vertex: the loop's fields, then those each rule added, in the order of the rules. What a rule
 * draws and computes is zero where the rule is off; the fields that describe the loop itself (lp, rx, ry, normal, shadow_steps; x
 * with a list) are filled at every setting. For a DIRECT vertex the density's fields are those of its connection (zero where no
 * connection reached `g`), for an EMIT record those of the bounce ray's hit. Built by tests/oracle_paths.py with the oracle's own
 * flags together with the other three oracle sources. */
#include "../oracle/rt_oracle.c"
#include <stdlib.h>

enum {
    O_FLAW_NONE = 0,
    O_FLAW_POWER_SIX_FACES = 1,   /* importance: 6 in m's place in g                                  */
    O_FLAW_POWER_NO_P = 2,        /* importance: g without p                                          */
    O_FLAW_MIS_BOUNCE_FULL = 3,   /* MIS: the bounce side keeps weight 1 (light is counted twice)     */
    O_FLAW_MIS_BOUNCE_NONE = 4    /* MIS: the bounce side adds nothing                                */
};

enum {
    O_PD_SKY0 = 0,      /* miss at depth 0:        gl * sky * tc * w                         */
    O_PD_SKY = 1,       /* miss at depth > 0:      tc * sky * sun * w / PI                   */
    O_PD_GLASS = 2,     /* glass fallback:         tc * (sc * (gl * ndotl)) * w              */
    O_PD_EMIT0 = 3,     /* emissive at depth 0:    tc * sc * extra * w                       */
    O_PD_EMIT = 4,      /* emissive at depth > 0:  tc * sc * extra * w / PI                  */
    O_PD_DIRECT = 5,    /* depth 0 or inner:       gl * lit * ndotl * sc * tc * w / PI       */
    O_PD_AMBIENT = 6    /* terminal:               extra * sc * tc * w / PI                  */
};

typedef struct {
    uint32_t ray;       /* index of the ray in the batch */
    int32_t kind, depth, chain, lit;
    float ndotl, sc[3], tc[3], weight, extra;   /* extra: the emission (kinds 3, 4) or the ambient factor (kind 6) */
    /* DIRECT vertices only (zero elsewhere): the two draws of the sun disc, their concentric map, L'; then the two draws of the bounce
     * direction, the (flipped) normal and the steps the shadow march took (64: it ended by the cap). At tan_radius 0: u1 = u2 = dx =
     * dy = 0 (nothing is drawn) and lp = lightDir. */
    float u1, u2, dx, dy, lp[3], rx, ry, normal[3];
    int32_t shadow_steps;
    /* DIRECT vertices with a list that is not empty (zero elsewhere): the four draws, the emitter and face they pick, the point on it;
     * cs, cl and r2 of the connection (cs = cl = 0 where r2 is not > 0); whether its ray hit anything, whether that hit lies in the
     * emitter's cube, the steps its march took (0: nothing was marched); g and the emissive term E (0 where nothing was added) */
    float u0, uf, ua, ub;
    int32_t j, f;
    float q[3], cs, cl, r2;
    int32_t conn_hit, in_box, conn_steps;
    float g, E[3];
    /* mode 1 only: the tick t = min((uint32)(u0 * 2^24), 2^24 - 1), the ticks emitter j holds, the number of faces x sees */
    int32_t t, ticks, m;
    float x[3];   /* both modes: the connection's origin, hitPoint + normal * 1e-1 */
    /* mis 1 only (zero elsewhere), DIRECT vertices whose connection reached g and EMIT records: the inputs of the density -- x, dir, cs,
     * the hit's point, axis (-1: the hit has no normal), cell, colour word (R | G << 8 | B << 16) and illumination byte -- then m, w,
     * pl, pb and the weight applied (wn or wb); has_mis says that these fields are filled */
    int32_t has_mis;
    float mx[3], mdir[3], mcs, mpoint[3];
    int32_t maxis, mcell[3], mrgb, millum, mm, mw;
    float pl, pb, wt;
} o_path_vertex;

/* include/vrt.h vrt_set_emitter_mis, emit_mis_density: every operation float32, rounded on its own */
typedef struct { int32_t axis, cell[3], rgb, illum, m, w; float point[3], pl, pb; } mis_t;
static int byte_of(float unorm) { return (int)rintf(unorm * 255.0f); }
static mis_t mis_density(v3 x, v3 dir, float cs, v3 point, v3 hn, i3 cell, const vox_t *hv, float inv_power) {
    mis_t d;
    d.axis = hn.x != 0.0f ? 0 : (hn.y != 0.0f ? 1 : (hn.z != 0.0f ? 2 : -1));   /* no normal: the direction is 0 on the hit's axis */
    d.cell[0] = cell.x; d.cell[1] = cell.y; d.cell[2] = cell.z;
    d.point[0] = point.x; d.point[1] = point.y; d.point[2] = point.z;
    const int R = byte_of(hv->color[0]), G = byte_of(hv->color[1]), B = byte_of(hv->color[2]);
    d.rgb = R | (G << 8) | (B << 16);
    d.illum = byte_of(hv->props[1]);
    const v3 v = sub3(point, x);
    const float r2 = dot3(v, v);
    const float cl = d.axis < 0 ? 0.0f : fabsf(vget(dir, d.axis));
    d.m = 0;
    for (int k = 0; k < 3; k++) {
        const float xk = vget(x, k);
        if (xk < (float)d.cell[k] || xk > (float)d.cell[k] + 1.0f) d.m++;
    }
    d.w = d.illum * (R + G + B);
    d.pl = (d.m == 0 || !(cl > 0.0f)) ? 0.0f : ((((float)d.w * inv_power) * r2) / ((float)d.m * cl));
    d.pb = (cs > 0.0f ? cs : 0.0f) / kPI;
    return d;
}

/* the basis of include/vrt.h vrt_set_sun_disc, step 1, with the oracle's own normalize3 / len3 / cross3 */
typedef struct { float s, ll; v3 Ln, T, B; } sun_t;
static sun_t sun_basis(const float *light_dir, float tan_radius) {
    sun_t b;
    v3 L = {light_dir[0], light_dir[1], light_dir[2]};
    b.s = tan_radius;
    b.ll = len3(L);
    b.Ln = normalize3(L);
    v3 up;
    if (fabsf(b.Ln.z) < 0.999f) { up.x = 0.0f; up.y = 0.0f; up.z = 1.0f; } else { up.x = 1.0f; up.y = 0.0f; up.z = 0.0f; }
    b.T = normalize3(cross3(up, b.Ln));
    b.B = cross3(b.Ln, b.T);
    return b;
}

/* the concentric map of include/vrt.h vrt_set_lens, step 3 (tests/oracle_lens.c o_lens_point has it for the lens sequence) */
void o_sun_disc_map(float lu, float lv, float *lx, float *ly) {
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

/* the basis as the checker makes it, for the tests: out[11] = tan_radius, ll, Ln, T, B */
void o_sun_basis(const float *light_dir, float tan_radius, float *out) {
    sun_t b = sun_basis(light_dir, tan_radius);
    out[0] = b.s; out[1] = b.ll;
    out[2] = b.Ln.x; out[3] = b.Ln.y; out[4] = b.Ln.z;
    out[5] = b.T.x; out[6] = b.T.y; out[7] = b.T.z;
    out[8] = b.B.x; out[9] = b.B.y; out[10] = b.B.z;
}

typedef struct {
    o_path_vertex *buf;
    size_t cap, n;
    uint32_t ray;
} pd_log;

/* the record pd_put() wrote last, or NULL where it was not kept */
static o_path_vertex *pd_last(pd_log *lg) { return (lg && lg->n >= 1 && lg->n <= lg->cap) ? &lg->buf[lg->n - 1] : NULL; }

static void pd_mis(o_path_vertex *v, v3 x, v3 dir, float cs, const mis_t *d, float wt) {
    if (!v) return;
    v->has_mis = 1;
    v->mx[0] = x.x; v->mx[1] = x.y; v->mx[2] = x.z;
    v->mdir[0] = dir.x; v->mdir[1] = dir.y; v->mdir[2] = dir.z;
    v->mcs = cs;
    for (int k = 0; k < 3; k++) { v->mpoint[k] = d->point[k]; v->mcell[k] = d->cell[k]; }
    v->maxis = d->axis; v->mrgb = d->rgb; v->millum = d->illum; v->mm = d->m; v->mw = d->w;
    v->pl = d->pl; v->pb = d->pb; v->wt = wt;
}

static void pd_put(pd_log *lg, int kind, int depth, int chain, int lit, float ndotl, const float *sc, const float *tc, float w, float extra) {
    if (!lg) return;
    if (lg->n < lg->cap) {
        o_path_vertex *v = &lg->buf[lg->n];
        v->ray = lg->ray; v->kind = kind; v->depth = depth; v->chain = chain; v->lit = lit;
        v->ndotl = ndotl;
        for (int k = 0; k < 3; k++) { v->sc[k] = sc ? sc[k] : 0.0f; v->tc[k] = tc[k]; }
        v->weight = w; v->extra = extra;
        v->u1 = v->u2 = v->dx = v->dy = v->rx = v->ry = 0.0f;
        for (int k = 0; k < 3; k++) v->lp[k] = v->normal[k] = 0.0f;
        v->shadow_steps = 0;
        v->u0 = v->uf = v->ua = v->ub = v->cs = v->cl = v->r2 = v->g = 0.0f;
        v->j = v->f = v->conn_hit = v->in_box = v->conn_steps = 0;
        for (int k = 0; k < 3; k++) v->q[k] = v->E[k] = 0.0f;
        v->t = v->ticks = v->m = 0;
        v->x[0] = v->x[1] = v->x[2] = 0.0f;
        v->has_mis = 0;
        for (int k = 0; k < 3; k++) { v->mx[k] = v->mdir[k] = v->mpoint[k] = 0.0f; v->mcell[k] = 0; }
        v->mcs = v->pl = v->pb = v->wt = 0.0f;
        v->maxis = v->mrgb = v->millum = v->mm = v->mw = 0;
    }
    lg->n++;   /* counts past the capacity: the caller sees that the log was cut */
}

/* comp:435-622 pathTrace in O_MODE_FULL with the path depth `D` (1 .. 8), the sun disc `sun`, the emitter list (n_emit entries), its
 * thresholds, the mode and -- read at mode 1 with n_emit > 0 only -- the MIS flag with inv_power = 1 / Wtot */
static void path_trace_paths(ctx_t *c, v3 ray_origin, v3 ray_dir, int D, const sun_t *sun, const int32_t *emit, int n_emit, const uint32_t *cdf, int mode, int mis, float inv_power, int flaw, float out_rgb[3], int32_t *voxel_id, int32_t *pixel_dist, pd_log *lg) {
    const o_scene *s = c->s;
    int32_t cur = 0;
    i3 nmin = {s->bounds_min[0], s->bounds_min[1], s->bounds_min[2]};
    i3 nmax = {s->bounds_max[0], s->bounds_max[1], s->bounds_max[2]};
    *voxel_id = 0;
    *pixel_dist = s->bounds_max[0] - s->bounds_min[0];
    v3 gro = scale3(ray_origin, s->voxel_scale);
    i3 this_mp = floor_i3(gro);
    vox_t tv = octree_find(c, this_mp, &nmin, &nmax, &cur);
    float start_iof = (tv.props[0] > 0.0f && tv.props[0] < 3.0f) ? tv.props[0] : 1.0f;

    ray_t stack[MAX_RAYS];
    int chain_of[MAX_RAYS];   /* the log's chain of each waiting ray (0: the depth-0 rays) */
    for (int i = 0; i < MAX_RAYS; i++) { stack[i].defined = 0; chain_of[i] = 0; }
    float inv_len = 1.0f / sqrtf(dot3(ray_dir, ray_dir));
    ray_dir = scale3(ray_dir, inv_len);
    const float ones[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    stack[0] = make_ray(gro, ray_dir, start_iof, 1.0f, s->global_light, 0.0f,
                        tv.color[3] > 0.0f ? tv.color : ones, tv.color[3] * 5.0f, 0);
    int sp = 1;
    int chains = 0;
    float fc[3] = {0.0f, 0.0f, 0.0f};
    const float *gl = s->global_light;
    v3 light = {s->light_dir[0], s->light_dir[1], s->light_dir[2]};

    const int use_mis = mis && mode == 1 && n_emit > 0;
    float cb = 0.0f;   /* the cosine of the bounce ray in flight at its vertex: a ray of depth >= 1 is popped right after its push */
    while (sp > 0) {
        ray_t r = stack[--sp];
        const int chain = chain_of[sp];
        stack[sp].defined = 0;
        if (!r.defined) continue;
        i3 mp = {0, 0, 0};
        v3 hp = {0, 0, 0}, hn = {0, 0, 0};
        vox_t last, hv;
        int hit = hit_marching(c, r.origin, r.dir, r.iof, &mp, &hp, &hn, &last, &hv);
        float tc[4] = {r.tint[0], r.tint[1], r.tint[2], r.tint[3]};
        if (!hit && r.depth <= 0) {
            if (r.dist_in_medium > 1e-6f && r.medium_density > 0.0f) absorb(tc, r.medium_density, r.dist_in_medium, r.medium_color);
            for (int k = 0; k < 3; k++) fc[k] = fc[k] + gl[k] * kSky[k] * tc[k] * r.weight;
            pd_put(lg, O_PD_SKY0, r.depth, chain, 0, 0.0f, NULL, tc, r.weight, 0.0f);
            continue;
        } else if (!hit) {
            for (int k = 0; k < 3; k++) fc[k] = fc[k] + tc[k] * kSky[k] * kSun * r.weight / kPI;
            pd_put(lg, O_PD_SKY, r.depth, chain, 0, 0.0f, NULL, tc, r.weight, 0.0f);
            continue;
        }
        v3 normal = hn;
        if (!(len3(hn) > 0.0f)) { normal.x = 0.0f; normal.y = 1.0f; normal.z = 0.0f; }
        v3 hpw = {hp.x / s->voxel_scale, hp.y / s->voxel_scale, hp.z / s->voxel_scale};
        r.dist_in_medium = r.dist_in_medium + len3(sub3(hpw, r.origin)) / s->voxel_scale;
        if (hv.color[3] <= 0.0f) { hv.props[0] = 1.0f; hv.props[1] = 0.0f; hv.props[2] = 0.0f; }
        if (last.color[3] <= 0.0f) {
            if (r.iof > 0.0f) { last.props[0] = last.props[1] = last.props[2] = 0.0f; }
            else { last.props[0] = 1.0f; last.props[1] = 0.0f; last.props[2] = 0.0f; }
        }
        float sc[4];
        memcpy(sc, hv.color[3] > 0.0f ? hv.color : last.color, 16);
        float n2 = hv.props[0] > 0.0f ? hv.props[0] : 1.0f;
        float n1 = last.props[0] > 0.0f ? last.props[0] : 1.0f;
        v3 inc = r.dir;
        if (r.dist_in_medium > 1e-6f && r.medium_density > 0.0f) absorb(tc, r.medium_density, r.dist_in_medium, r.medium_color);
        if (mp.x == s->highlighted[0] && mp.y == s->highlighted[1] && mp.z == s->highlighted[2]) {
            sc[0] = 1.0f - sc[0]; sc[1] = 1.0f - sc[1]; sc[2] = 1.0f - sc[2]; sc[3] = 1.0f;
        }
        float cosi = dot3(inc, normal);
        if (cosi > 0.0f) { normal.x = -normal.x; normal.y = -normal.y; normal.z = -normal.z; float t = n1; n1 = n2; n2 = t; }
        float ndotl = fmax_c(dot3(normal, light), 0.0f);

        if (r.depth == 0 && *voxel_id == 0 && sc[3] >= 1.0f) { /* comp:539-544 */
            int32_t lin = mp.x + s->tex_dim * (mp.y + s->tex_dim * mp.z);
            *voxel_id = lin * 6 + face_index(hn);
            *pixel_dist = (int32_t)len3(sub3(hpw, ray_origin));
        }

        if (r.depth <= 0 && sc[3] < 1.0f) { /* translucent, comp:547-572: unchanged */
            v3 refr_dir = refract3(inc, normal, n1 / n2);
            float R0 = (n1 - n2) / (n1 + n2) * (n1 - n2) / (n1 + n2);
            v3 ninc = {-inc.x, -inc.y, -inc.z};
            float cos_t = fmax_c(0.0f, dot3(ninc, normal));
            float fres = R0 + (1.0f - R0) * o_det_powf(1.0f - cos_t, 5.0f);
            fres = fmin_c(fmax_c(fres, 0.0f), 1.0f);
            int has_tir = len3(refr_dir) < 0.001f;
            float reflect_i = fres;
            float refract_i = has_tir ? 0.0f : (1.0f - fres);
            if (sp == MAX_RAYS || reflect_i <= 0.001f || refract_i <= 0.001f) {
                for (int k = 0; k < 3; k++) {
                    float direct = gl[k] * ndotl;
                    float lit = sc[k] * direct;
                    fc[k] = fc[k] + tc[k] * lit * r.weight;
                }
                pd_put(lg, O_PD_GLASS, r.depth, chain, 1, ndotl, sc, tc, r.weight, 0.0f);
                continue;
            }
            if (reflect_i > 0.001f && sp < MAX_RAYS) {
                float rw = r.weight * reflect_i;
                if (rw > 1e-4f) {
                    chain_of[sp] = chain;
                    stack[sp++] = make_ray(add3(hp, scale3(normal, 1e-4f)), reflect3(inc, normal), n1, rw, tc,
                                           r.dist_in_medium, last.color, last.color[3] * 5.0f, r.depth);
                }
            }
            if (refract_i > 0.001f && sp < MAX_RAYS && !has_tir) {
                chain_of[sp] = chain;
                stack[sp++] = make_ray(sub3(hp, scale3(normal, 1e-4f)), refr_dir, n2, r.weight * refract_i, tc,
                                       0.0f, hv.color, hv.color[3] * 5.0f, r.depth);
            }
        } else { /* opaque, comp:573-618 */
            float emission = hv.props[1] * 10.0f;
            if (emission > 0.0f && r.depth == 0) {
                for (int k = 0; k < 3; k++) fc[k] = fc[k] + tc[k] * sc[k] * emission * r.weight;
                pd_put(lg, O_PD_EMIT0, r.depth, chain, 0, ndotl, sc, tc, r.weight, emission);
                continue;
            } else if (emission > 0.0f) {
                if (use_mis) {   /* EMITTER MIS, the bounce: the complementary share of the balance heuristic */
                    const mis_t d = mis_density(r.origin, r.dir, cb, hp, hn, mp, &hv, inv_power);
                    float wb = !(d.pl > 0.0f) ? 1.0f : d.pb / (d.pl + d.pb);
                    if (flaw == O_FLAW_MIS_BOUNCE_FULL) wb = 1.0f;
                    if (flaw != O_FLAW_MIS_BOUNCE_NONE)
                        for (int k = 0; k < 3; k++) fc[k] = fc[k] + (tc[k] * sc[k] * emission * r.weight / kPI) * wb;
                    pd_put(lg, O_PD_EMIT, r.depth, chain, 0, ndotl, sc, tc, r.weight, emission);
                    pd_mis(pd_last(lg), r.origin, r.dir, cb, &d, flaw == O_FLAW_MIS_BOUNCE_NONE ? 0.0f : wb);
                    continue;
                }
                if (n_emit > 0) continue;   /* EMITTER SAMPLING (7): the vertex before has sampled the emitters itself */
                for (int k = 0; k < 3; k++) fc[k] = fc[k] + tc[k] * sc[k] * emission * r.weight / kPI;
                pd_put(lg, O_PD_EMIT, r.depth, chain, 0, ndotl, sc, tc, r.weight, emission);
                continue;
            }
            o_path_vertex *direct_rec = NULL;
            if (r.depth < D) {   /* THE RULE: depth 0, and the inner vertices 1 <= d < D, take the depth-0 operations */
                /* THE SUN DISC: at tan_radius > 0 this vertex draws its own light direction first */
                float u1 = 0.0f, u2 = 0.0f, dx = 0.0f, dy = 0.0f;
                v3 lp = light;
                float nl = ndotl;
                if (sun->s > 0.0f) {
                    u1 = rand_f(c);
                    u2 = rand_f(c);
                    o_sun_disc_map(u1, u2, &dx, &dy);
                    const float sx = sun->s * dx, sy = sun->s * dy;
                    v3 v = {(sun->Ln.x + sx * sun->T.x) + sy * sun->B.x, (sun->Ln.y + sx * sun->T.y) + sy * sun->B.y,
                            (sun->Ln.z + sx * sun->T.z) + sy * sun->B.z};
                    lp = scale3(normalize3(v), sun->ll);
                    nl = fmax_c(dot3(normal, lp), 0.0f);
                }
                const uint64_t steps0 = c->st.steps;
                int lit = not_in_shadow(c, add3(hp, scale3(normal, 2e-3f)), lp);
                const int32_t shadow_steps = (int32_t)(c->st.steps - steps0);
                for (int k = 0; k < 3; k++) {
                    float direct = gl[k] * (float)lit * nl;
                    fc[k] = fc[k] + direct * sc[k] * tc[k] * r.weight / kPI;
                }
                pd_put(lg, O_PD_DIRECT, r.depth, r.depth == 0 ? chains + 1 : chain, lit, nl, sc, tc, r.weight, 0.0f);
                direct_rec = pd_last(lg);
                if (direct_rec) {
                    direct_rec->u1 = u1; direct_rec->u2 = u2; direct_rec->dx = dx; direct_rec->dy = dy;
                    direct_rec->lp[0] = lp.x; direct_rec->lp[1] = lp.y; direct_rec->lp[2] = lp.z;
                    direct_rec->normal[0] = normal.x; direct_rec->normal[1] = normal.y; direct_rec->normal[2] = normal.z;
                    direct_rec->shadow_steps = shadow_steps;
                }
                /* EMITTER SAMPLING (1-6): after the sun's direct term, before the bounce's two draws */
                if (n_emit > 0) {
                    const float u0 = rand_f(c), uf = rand_f(c), ua = rand_f(c), ub = rand_f(c);
                    const v3 x = add3(hp, scale3(normal, 1e-1f));
                    int j, f = 0, m = 0;
                    uint32_t t = 0, ticks = 0;
                    float p = 0.0f;
                    if (mode == 1) {   /* VRT_EMIT_POWER (1): the emitter by the thresholds */
                        t = (uint32_t)(u0 * 16777216.0f);
                        if (t > 16777215u) t = 16777215u;
                        int lo_i = 0, hi_i = n_emit - 1;   /* the smallest j with T_j > t; T_{n-1} = 2^24 > t */
                        while (lo_i < hi_i) {
                            const int mid = lo_i + (hi_i - lo_i) / 2;
                            if (cdf[mid] > t) hi_i = mid; else lo_i = mid + 1;
                        }
                        j = lo_i;
                        ticks = cdf[j] - (j > 0 ? cdf[j - 1] : 0u);
                        p = (float)ticks * 0x1p-24f;
                    } else {
                        j = (int)(u0 * (float)n_emit);
                        if (j > n_emit - 1) j = n_emit - 1;
                    }
                    const int32_t *e = emit + 4 * (size_t)j;
                    const float sz = (float)e[3];
                    if (mode == 1) {   /* (2): the face among those x sees, in axis order */
                        int faces[3];
                        for (int k = 0; k < 3; k++) {
                            const float xk = vget(x, k);
                            if (xk < (float)e[k]) faces[m++] = 2 * k;
                            else if (xk > (float)e[k] + sz) faces[m++] = 2 * k + 1;
                        }
                        if (m > 0) {
                            int i = (int)(uf * (float)m);
                            if (i > m - 1) i = m - 1;
                            f = faces[i];
                        }
                    } else {
                        f = (int)(uf * 6.0f);
                        if (f > 5) f = 5;
                    }
                    const int ax = f >> 1, side = f & 1, a1 = (ax + 1) % 3, a2 = (ax + 2) % 3;
                    float q[3] = {0.0f, 0.0f, 0.0f};
                    float r2 = 0.0f;
                    v3 w = {0.0f, 0.0f, 0.0f};
                    if (mode != 1 || m > 0) {   /* m == 0: nothing more happens, the four draws stay spent */
                        q[ax] = (float)e[ax] + (side ? sz : 0.0f);
                        q[a1] = (float)e[a1] + ua * sz;
                        q[a2] = (float)e[a2] + ub * sz;
                        const v3 qv = {q[0], q[1], q[2]};
                        w = sub3(qv, x);
                        r2 = dot3(w, w);
                    }
                    float cs = 0.0f, cl = 0.0f, g = 0.0f, E[3] = {0.0f, 0.0f, 0.0f};
                    int conn_hit = 0, in_box = 0;
                    int32_t conn_steps = 0;
                    if (r2 > 0.0f) {
                        const v3 dir = scale3(w, 1.0f / sqrtf(r2));
                        cs = dot3(normal, dir);
                        cl = side ? -vget(dir, ax) : vget(dir, ax);
                        if (cs > 0.0f && cl > 0.0f) {
                            const float ctint[4] = {tc[0] * sc[0], tc[1] * sc[1], tc[2] * sc[2], tc[3] * sc[3]};
                            ray_t cr = make_ray(x, dir, n1, r.weight / (float)INDIRECT_SAMPLES, ctint, 0.0f, last.color, last.color[3] * 5.0f, r.depth + 1);
                            i3 mp2 = {0, 0, 0};
                            v3 hp2 = {0, 0, 0}, hn2 = {0, 0, 0};
                            vox_t last2, hv2;
                            const uint64_t csteps0 = c->st.steps;
                            conn_hit = hit_marching(c, cr.origin, cr.dir, cr.iof, &mp2, &hp2, &hn2, &last2, &hv2);
                            conn_steps = (int32_t)(c->st.steps - csteps0);
                            in_box = conn_hit && mp2.x >= e[0] && mp2.x < e[0] + e[3] && mp2.y >= e[1] && mp2.y < e[1] + e[3] &&
                                     mp2.z >= e[2] && mp2.z < e[2] + e[3];
                            if (in_box) {   /* the hit of a ray of depth >= 1, up to the emissive test */
                                float tc2[4] = {cr.tint[0], cr.tint[1], cr.tint[2], cr.tint[3]};
                                v3 hpw2 = {hp2.x / s->voxel_scale, hp2.y / s->voxel_scale, hp2.z / s->voxel_scale};
                                cr.dist_in_medium = cr.dist_in_medium + len3(sub3(hpw2, cr.origin)) / s->voxel_scale;
                                if (hv2.color[3] <= 0.0f) { hv2.props[0] = 1.0f; hv2.props[1] = 0.0f; hv2.props[2] = 0.0f; }
                                float sc2[4];
                                memcpy(sc2, hv2.color[3] > 0.0f ? hv2.color : last2.color, 16);
                                if (cr.dist_in_medium > 1e-6f && cr.medium_density > 0.0f) absorb(tc2, cr.medium_density, cr.dist_in_medium, cr.medium_color);
                                if (mp2.x == s->highlighted[0] && mp2.y == s->highlighted[1] && mp2.z == s->highlighted[2]) {
                                    sc2[0] = 1.0f - sc2[0]; sc2[1] = 1.0f - sc2[1]; sc2[2] = 1.0f - sc2[2]; sc2[3] = 1.0f;
                                }
                                const float emission2 = hv2.props[1] * 10.0f;
                                if (emission2 > 0.0f) {
                                    if (mode == 1) {
                                        const float mg = flaw == O_FLAW_POWER_SIX_FACES ? 6.0f : (float)m;
                                        if (flaw == O_FLAW_POWER_NO_P) g = ((cs * cl) * (mg * (sz * sz))) / (kPI * r2);
                                        else g = ((cs * cl) * (mg * (sz * sz))) / ((kPI * r2) * p);
                                    } else {
                                        const float area = ((float)n_emit * 6.0f) * (sz * sz);
                                        g = ((cs * cl) * area) / (kPI * r2);
                                    }
                                    if (use_mis) {   /* EMITTER MIS, the connection: its share of the balance heuristic */
                                        const mis_t d = mis_density(x, dir, cs, hp2, hn2, mp2, &hv2, inv_power);
                                        const float wn = d.pl > 0.0f ? d.pl / (d.pl + d.pb) : 0.0f;
                                        for (int k = 0; k < 3; k++) {
                                            E[k] = tc2[k] * sc2[k] * emission2 * cr.weight / kPI;
                                            if (d.pl > 0.0f) fc[k] = fc[k] + (E[k] * g) * wn;
                                        }
                                        pd_mis(direct_rec, x, dir, cs, &d, wn);
                                    } else {
                                        for (int k = 0; k < 3; k++) {
                                            E[k] = tc2[k] * sc2[k] * emission2 * cr.weight / kPI;
                                            fc[k] = fc[k] + E[k] * g;
                                        }
                                    }
                                }
                            }
                        }
                    }
                    if (direct_rec) {
                        direct_rec->u0 = u0; direct_rec->uf = uf; direct_rec->ua = ua; direct_rec->ub = ub;
                        direct_rec->j = j; direct_rec->f = f;
                        for (int k = 0; k < 3; k++) { direct_rec->q[k] = q[k]; direct_rec->E[k] = E[k]; }
                        direct_rec->cs = cs; direct_rec->cl = cl; direct_rec->r2 = r2;
                        direct_rec->conn_hit = conn_hit; direct_rec->in_box = in_box; direct_rec->conn_steps = conn_steps;
                        direct_rec->g = g;
                        direct_rec->t = (int32_t)t; direct_rec->ticks = (int32_t)ticks; direct_rec->m = m;
                        direct_rec->x[0] = x.x; direct_rec->x[1] = x.y; direct_rec->x[2] = x.z;
                    }
                }
            } else {             /* d == D: the shader's terminal branch */
                float amb = fmax_c(1.0f - o_det_expf(-r.dist_in_medium / 512.0f), 0.01f);
                for (int k = 0; k < 3; k++) fc[k] = fc[k] + amb * sc[k] * tc[k] * r.weight / kPI;
                pd_put(lg, O_PD_AMBIENT, r.depth, chain, 0, ndotl, sc, tc, r.weight, amb);
                continue;
            }
            for (int i = 0; i < INDIRECT_SAMPLES && sp < MAX_RAYS && r.depth < D; i++) {
                float rx = rand_f(c), ry = rand_f(c);
                if (direct_rec) { direct_rec->rx = rx; direct_rec->ry = ry; }
                v3 bd = cosine_hemisphere(normal, rx, ry);
                cb = dot3(normal, bd);
                float nw = r.weight / (float)INDIRECT_SAMPLES;
                float tint[4] = {tc[0] * sc[0], tc[1] * sc[1], tc[2] * sc[2], tc[3] * sc[3]};
                chain_of[sp] = r.depth == 0 ? ++chains : chain;
                stack[sp++] = make_ray(add3(hp, scale3(normal, 1e-1f)), bd, n1, nw, tint, 0.0f,
                                       last.color, last.color[3] * 5.0f, r.depth + 1);
            }
        }
    }
    out_rgb[0] = fc[0]; out_rgb[1] = fc[1]; out_rgb[2] = fc[2];
}

/* The thresholds of the header, in exact integers: out[n] from the weights[n] */
void o_emit_thresholds(const uint64_t *weights, int n, uint32_t *out) {
    uint64_t total = 0, cum = 0;
    for (int j = 0; j < n; j++) total += weights[j];
    for (int j = 0; j < n; j++) {
        cum += weights[j];
        if (total > 0) out[j] = (uint32_t)((uint64_t)(j + 1) + (uint64_t)((unsigned __int128)cum * (uint64_t)((1u << 24) - (uint32_t)n) / total));
        else out[j] = (uint32_t)((((uint64_t)j + 1) << 24) / (uint64_t)n);
    }
}

/* Every output but the scene and the rays may be NULL. Returns the number of log records the batch produced (more than log_cap:
 * the log holds the first log_cap of them). */
size_t o_shade_rays_paths(const o_scene *s, size_t n, const float *origins, int stride, const float *dirs, int width, int depth, float tan_radius,
                          const int32_t *emit, const uint64_t *weights, int n_emit, int mode, int mis, int flaw, int sample, uint8_t *rgba8, int32_t *id_dist, float *rgb_out, o_path_vertex *log, size_t log_cap) {
    ctx_t c;
    memset(&c, 0, sizeof c);
    c.s = s;
    pd_log lg = {log, log_cap, 0, 0};
    const sun_t sun = sun_basis(s->light_dir, tan_radius);
    uint32_t *cdf = NULL;
    if (n_emit > 0 && mode == 1) {
        cdf = (uint32_t *)malloc((size_t)n_emit * sizeof *cdf);
        if (!cdf) return 0;
        o_emit_thresholds(weights, n_emit, cdf);
    }
    /* per launch: inv_power = 1 / Wtot, rounded once from the float64 quotient; 0 for a list without power */
    uint64_t wtot = 0;
    if (n_emit > 0 && mode == 1)
        for (int j = 0; j < n_emit; j++) wtot += weights[j];
    const float inv_power = wtot > 0 ? (float)(1.0 / (double)wtot) : 0.0f;
    for (size_t i = 0; i < n; i++) {
        c.px_fetches = 0;
        c.px_index = (uint32_t)i;
        init_rng(&c, (int)(i % (size_t)width), (int)(i / (size_t)width), sample);
        const float *o = origins + (stride ? i * 3 : 0), *d = dirs + i * 3;
        v3 ro = {o[0], o[1], o[2]}, wd = {d[0], d[1], d[2]};
        float rgb[3];
        int32_t vid, dist;
        lg.ray = (uint32_t)i;
        path_trace_paths(&c, ro, wd, depth, &sun, emit, n_emit, cdf, mode, mis, inv_power, flaw, rgb, &vid, &dist, log ? &lg : NULL);
        if (rgba8) { rgba8[i * 4 + 0] = unorm8(rgb[0]); rgba8[i * 4 + 1] = unorm8(rgb[1]); rgba8[i * 4 + 2] = unorm8(rgb[2]); rgba8[i * 4 + 3] = 255; }
        if (id_dist) { id_dist[i * 2 + 0] = vid; id_dist[i * 2 + 1] = dist; }
        if (rgb_out) { rgb_out[i * 3 + 0] = rgb[0]; rgb_out[i * 3 + 1] = rgb[1]; rgb_out[i * 3 + 2] = rgb[2]; }
    }
    free(cdf);
    return lg.n;
}
