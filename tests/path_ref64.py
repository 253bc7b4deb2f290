"""A float64 restatement of pathTrace (shaders/raytracing.comp:435-622) in VRT_MODE_FULL, the whole ray tree (test helper,
not a test).

It reuses tests/shader_ref64.py's decoded grid, node-to-node step, floor rule and notInShadow, and follows the same
independence rules: numpy and shader_ref64 only, nothing under oracle/ and nothing of the product's tracing
(tests/test_shader_reference64.py enforces that for both modules).

What is restated, from the GLSL:
  * The ray stack (comp:451-470): a real LIFO of MAX_RAYS = 8 entries per pixel. Every pass pops the top ray of every
    pixel whose stack is not empty and marches those rays together; pushes go on top, reflected ray before refracted.
  * The initial ray (comp:443-462): the grid origin cameraPos * voxelScale, startIOF (the eye voxel's refraction when it is
    in (0, 3), else 1), the eye voxel's colour and density a*5 as the medium (colour 1 when a == 0), colorTint =
    globalLight, weight 1, depth 0.
  * hitMarching (comp:248-330) from any origin with the ray's own rayIOF as the "air" refraction of the start.
  * A miss (comp:480-495): at depth <= 0 the in-medium absorption exp(-density * distanceInMedium * (1 - mediumColor))
    when distanceInMedium > 1e-6 and density > 0, then sky * globalLight; at depth > 0 sky * sunIntensity (3) / PI.
  * A hit (comp:497-544): distanceInMedium += length(hitPoint / voxelScale - origin) / voxelScale (a world-space point
    minus a grid-space origin, divided once more), the property overrides for a <= 0 (comp:503-504), surfaceColor,
    n1 / n2, the absorption, the highlight inversion (alpha 1), the exit-side flip and swap when cosi > 0, GLSL refract
    and reflect, Fresnel with a true pow, TIR as |refractDir| < 0.001, ndotl; the voxel ID and dist of the first
    depth-0 hit with surfaceColor.a >= 1 while primaryVoxelID is still 0 (an ID-0 hit -- the origin voxel's +X face --
    leaves it re-enterable), dist = int(length(hitPointWorld - cameraPos)).
  * Glass (comp:546-572): the directly lit fall-back when the stack is full or an intensity is <= 0.001; otherwise the
    reflected ray (hitPoint + N*1e-4, n1, weight*R if > 1e-4, the parent's distanceInMedium, the last voxel as medium)
    and the refracted one (hitPoint - N*1e-4, n2, weight*(1-R), distance 0, the hit voxel as medium).
  * Opaque (comp:573-618), also glass at depth > 0: emission * 10 at depth 0 and / PI deeper; at depth 0 the direct
    term through notInShadow(hitPoint + N*2e-3); at depth > 0 ambient max(1 - exp(-distanceInMedium / 512), 0.01) / PI;
    the bounce from hitPoint + N*0.1 with rayIOF n1, tint colorTint * surfaceColor, the last voxel as medium.
  * initRNG / rand (comp:381-395) in exact uint32 arithmetic, seed x + y*1920 + 123456 + sampleIndex*78901 (mod 2^32);
    rand() keeps its float32 conversion float(state) / 2^32 (it is part of the shader's definition, and may give 1.0).
    cosineSampleHemisphere (comp:402-417) after it -- phi, sqrt, sin / cos, cross, normalize -- is float64.

Two facts of the GLSL that the restatement shows rather than assumes: hitMarching's normal is -sign(d) on the axis
crossed, so cosi = dot(d, normal) = -|d[axis]| < 0 at every hit and the exit-side flip and n1 / n2 swap (comp:522-526)
never run -- n1 is the medium left and n2 the medium entered on both sides of glass already. And the swap test
stackSize == MAX_RAYS (comp:548) follows a pop, so it is never true either; a full stack shows as a refracted ray that is
not pushed (comp:565) after the reflected one took the last slot.

Error model (the undecided rule of shader_ref64 carried into every ray of the tree; a pixel is undecided when any ray of
its tree is, and decided pixels must match exactly: rgb bytes, ID and dist):
  * Position. Each ray carries a per-axis bound on the float32 error of its position. A march adds shader_ref64's step
    error plus dir_err * t. The coordinate a step crosses is computed, not carried: the float32 landing is
    pos + d * ((P - pos) * (1 / d)), within 4u * (|P - pos| + err) of the node plane P before two roundings, whatever
    pos's own error was, so the crossed coordinate's bound drops to that when no other coordinate is near a plane (the
    axis is the same in float32); when 8u * (|P - pos| + err) is below half the float32 spacing at P the landing is P
    itself and the pushed coordinate is exactly float32(P + s*1e-4), error 0. The bounds never drop below the ray's line
    error lo3: its origin's bound, which the line keeps however often a coordinate lands on a plane.
    A ray spawned at a hit starts at hitPoint + N * offset with the hit's error plus the rounding of the offset (u times
    the coordinate). The reflected ray's origin along N is P + s*1e-4 - s*1e-4: within float32 rounding of the plane.
    It is evaluated in float32 for every float32 landing within the error bound of P. When they all floor alike the
    start voxel is decided and the spread of those origins is the error along N. When they do not, the start is either
    the last voxel (A) or the hit voxel (B); B's first step goes back across P and is pushed 1e-4 into the last voxel,
    and if that is no change of medium (comp:318-321 with rayIOF n1: a reflection inside glass off its face to air)
    B is A's ray moved 1e-4 along N, so the ray is traced as A with 1e-4 more error along N; otherwise the ray is
    undecided (a reflection seen from air after an approach step too long for the landing to be decided). A start
    on the near side of P is locked there: the coordinate moves away from P monotonically, so that plane is not tested
    again. The error along N shows in the other coordinates where the line crosses planes of N's axis, scaled by
    |d_k / d_N|; the reflected ray's line error holds that.
  * Direction. dir_err bounds the absolute error of each unit direction component beyond the primary ray's ~6u (which
    shader_ref64's step error already holds): reflect is exact for an axis normal (the error stays the parent's);
    refract adds 8u + 4u(1 + eta^2) / sqrt(k) and scales the parent's by eta + eta^2 |cos| / sqrt(k); a bounce has
    E_SINCOS + 2*pi*u (phi's rounding) + 6u (sqrt, products, normalize). Components within max(DIR_MARGIN, 2 * dir_err)
    of 0 are undecided.
  * Colour. Each ray carries a relative error bound of weight * colorTint. A contribution adds the factors it multiplies
    (<= 6u), E_EXP and the exponent's error (|arg| * 5u + density * (1 - mediumColor) * dist_err) where it absorbs, the
    ambient's error (E_EXP * e + e * dist_err / 512 + 2u over its value), and a spawned ray adds Fresnel's absolute error
    e_F (R0 * (8u + 4u(n1 + n2)/|n1 - n2|), E_POW * pow, 5 (1 - cos)^4 (dir_err + 8u)) over the intensity it takes.
    The byte is undecided within EPS_COLOR + 255 * (sum of |contribution| * rel + (contributions + 1) * u * colour) of a
    .5 tie. dist_err grows by the two endpoints' position errors and 4u of the coordinates per hit (over voxelScale).
  * Thresholds a float32 run could land on the other side of: reflect / refract intensity within e_F of 0.001, the
    reflected weight within its error of 1e-4, k within 6u(1 + eta^2) + 2 eta^2 |cos| dir_err of 0 (TIR: refract then
    returns 0 and the < 0.001 length test follows it), |cosi| within dir_err + DIR_MARGIN of 0, distanceInMedium within
    its error of 1e-6 where a medium absorbs, the primary cap (shader_ref64's 1000 of 1024 steps) for every ray and the
    shadow cap (64) as in shader_ref64. The ambient's 0.01 kink is continuous (max is 1-Lipschitz), so it takes the same
    value bound as the rest of the ambient.
  * The det_* routines that stand in for exp, pow, sin and cos are held to these measured bounds on the shader's domains
    (tests/test_path_reference64.py measures them on the oracle, tests/test_gpu_path_reference64.py on the device):
    det_expf on [-87, 0]: relative 7.85e-8 (E_EXP = 1.2e-7; below -87 it returns 0, off by < 1.7e-38);
    det_powf(x, 5) on [0, 1]: relative 8.66e-6 where x^5 >= 1.7e-38 (E_POW = 1.2e-5; absolute < 1.7e-38 below);
    det_sinf / det_cosf on [0, 2 pi): absolute 6.82e-8 / 7.61e-8 (E_SINCOS = 1.2e-7).

Ray batches (PathTrace.rays; the camera constructor is a thin caller of the same entry). shader_ref64's docstring has the
per-ray rules; here they enter as: the primary ray's origin gro = float32(origin * voxelScale) with the per-axis rounding
of that product as err3 and lo3 (zero when exact); startIOF, medium colour and density from the voxel at floor(gro);
dist from the ray's own world-space origin; dir_err = 4.5u (R.GIVEN_DIR_ERR, the float32 normalisation, derived there)
for a given direction, whose components below DIR_MARGIN are decided by the shader's own rule because their error is
relative; initRNG((i % width, i // width), sample); origins outside the world in `outside`, never traced or compared.
  * Radiance. bound() = cerr + (ncon + 1) * u * |fc| + EPS_COLOR / 255 is the one colour bound: frame()'s tie test is
    255 * bound() and radiance() returns (h(fc), bound(), decided).
  * What the float comparison found missing: a hit point's error ACROSS the ray. The crossed coordinate is computed
    (above), but the float32 run follows its own line o + (d + delta) s, and where that line meets the plane of axis b
    after a path s, coordinate a differs by s (delta_a - delta_b d_a / d_b) <= s (dir_err + 6u) (1 + |d_a / d_b|),
    whatever planes were crossed on the way. The per-axis bounds reset at every crossing and lost this; on a ray from
    480 voxels away into glass the entry point moved by 3e-5 and the distance in the medium by 6.5e-5, 1.06 times the
    bound then stated. march() now returns it (m.line) and it enters distanceInMedium's error (edim) at the hit and at
    the origin of every ray spawned there. The floor margins keep the per-axis bounds: every decided ray of every
    frame and batch agrees exactly with them, and they are doubled by DELTA_SAFETY.

Jittered and thin-lens samples of the accumulation enter through PathTrace.lens: tests/lens_ref64.py restates their rays
in float64 with a per-ray origin bound (err3 / lo3) and direction bound (dir_err), and _run carries both as it does a
batch's.

Path depth, sun disc, emitter sampling, emitter importance and emitter MIS (include/vrt.h under those titles; depth=,
tan_radius=, emit= and mis= of the three constructors; the defaults give the shader, bit for bit what this module gave
before it took them). Restated from the header's text alone -- not from the kernels, not from the C checkers; tests/deep_ref64.py
holds the sun's basis and direction, the emitter list, weights and thresholds, and the discrete choices.
  * Path depth. The opaque, non-emissive branch of a ray of depth d: d < D casts the shadow ray, adds the direct term, takes
    its draws and pushes the bounce of depth d + 1 with distanceInMedium 0; it adds no ambient term. d >= D (d >= 1 at D = 1)
    takes the terminal ambient branch. Translucent surfaces below depth 0 are diffuse (they were already), so a chain is
    linear: a pop precedes every push. err3, lo3, edim and the relative colour error pass from vertex to vertex as they did
    from depth 0 to depth 1.
  * The order of a vertex's draws: u1, u2 of the sun (if its radius is > 0), then u0, uf, ua, ub of the connection (if
    sampling is on and the list is not empty), then the bounce's two.
  * Sun disc. L' from deep_ref64.sun_dirs; notInShadow from hitPoint + normal * 2e-3 along L' with the per-ray direction bound
    deep_ref64.sun_dir_err (derived there; R.not_in_shadow adds dir_err * t per step and leaves a ray with a component within
    the direction margin of 0 undecided); ndotl' = max(dot(normal, L'), 0) is continuous: its absolute error, the same bound,
    goes into the colour bound (cerr += the term at ndotl' = 1 times the bound). The translucent branch keeps ndotl from L.
  * Emitter connections (_connect). x = hitPoint + normal * 1e-1 with the bounce origin's per-axis bound ex3. j, f, t, i, p in
    exact float32 (deep_ref64). q: the face coordinate is an exact integer, the other two lo + u * sz round twice (u * sz and
    the sum): u (u sz) + u |q|. w = q - x has e3 = ex3 + xe3 (below) + eq + u |w| per axis; r2 and dir = w / |w| in float64;
    dir's bound is R.GIVEN_DIR_ERR (the float32 normalisation, relative, <= absolute for a unit vector) + |e3|_2 / r: the
    projection (I - n n^T) dw / r does not lengthen dw. cs > 0, cl > 0 and r2 > 0 are undecided within that bound of 0; the
    visible-face tests x[k] < lo[k], x[k] > lo[k] + sz within ex3[k] + xe3[k] of the plane. The connection is marched with march() from
    x with ex3 + xe3 and that direction bound, rayIOF n1; the in-cube test is undecided where a coordinate of the hit other
    than the crossed one lies within the floor margin of a face of the cube. The hit is evaluated as a deeper ray's
    (distanceInMedium from x, the absorption in the last voxel's medium, the highlight inversion, emission = props[1] * 10).
    g's relative error, dir_err / cs + dir_err / cl + 2 |e3|_2 / r + 14u (its products, quotients and E_k's), joins the ray's
    colour bound. Rule 7 is a branch: with sampling on a deeper ray that finds an emitter adds nothing.
  * MIS (_mis_density). pl and pb in float64 from x, dir, cs and the hit: m of the hit CELL, w of the hit voxel's words,
    inv_power the float32 of 1.0 / Wtot. The visible-axis tests are undecided within ex3 + xe3 of their planes, !(pl > 0) where cl
    lies within dir's bound of 0 (m and w are integers), and pb's bound is relative, so cs within it of 0 is undecided too.
    rel(pl) = 2 |e_v|_2 / r + dir_err / cl + 8u with e_v the bound of hit.point - x, rel(pb) = dir_err / cs + 2u;
    wn = pl / (pl + pb) and wb = pb / (pl + pb) move by (1 - w) (rel(pl) + rel(pb)) relative. A contributing connection ends
    on the face it aimed at (a face turned towards x is its cube's first along the line), so its hit is q within the march's
    own roundings wherever the float32 x lies. The bounce keeps cb = dot(normal, bd) (bound: BOUNCE_DIR_ERR) in the ray.
  * What the float comparison found missing, again: a VERTEX's error across its ray. m.line (above) entered only the distance
    in a medium. A connection reads the vertex itself -- cl = w[ax] / r at a grazing face is w[ax] over a coordinate of x --
    and after two bounces the float32 vertex lay 3.6e-4 from this module's, 40 times its per-axis bound. Every ray now carries
    xerr[3], what its origin may be off by beyond err3: at a hit on a plane of axis b the point moves by e_a + e_b |d_a / d_b|
    in coordinate a and not at all in b (so floor-ceiling-floor chains do not amplify it), plus the march's own m.line3. It
    enters everything continuous of a connection and of an MIS density, and the connection's march. And corners: where a step
    lands within the margin of a plane of another axis, the float32 run may cross that plane first and be in the cell on
    the near side of the crossed axis, which R._floor_undecided's alternatives do not hold; a connection aimed at the rim
    of an emitter's face met exactly that (hit there, missed here). march(corners=True), for connections, tries that cell
    too. And the distance in a medium: a ray of depth >= 2 starts from a vertex its chain has moved and ends on one it
    moves on, so its length carries |xerr|_2 of both ends in edim (a connection's, |xe3|_2 of its vertex). Rays aimed into
    the dragon's penumbrae found it: a last segment 0.15 voxels long after five bounces, whose terminal ambient term
    1 - exp(-dim / 512) is relative to that length, lay 2.3e-3 off at D = 6 and D = 8 under a bound of 4e-4.
  * Known unsound: the floor margins of the shadow and bounce marches at inner vertices (depth >= 1) still take the per-axis
    bound err3 without xerr. The float32 vertex may lie xerr further (3.6e-4 seen, 40 times err3), so a step of such a march
    that passes a cell boundary closer than xerr is decided here although the float32 run may take the other cell. This
    cannot hide a wrong kernel (a decided ray is compared exactly); it can fail a right one on a batch other than the
    tests'. No decided ray of any batch at any setting disagrees. With xerr in those margins every comparison still holds,
    but the undecided share of the lamp room at (8, 0.05, mis) rises from 23 % to 36 %, over the ceiling of 0.30 that the
    tests keep, and the other shares by a tenth to a half; the margins wait for a bound on xerr that does not grow with
    every change of the hit axis.
  * STATS per pixel: shadowing, inner and terminal vertices, vertices whose lit differs from the point sun's, connections
    drawn, marched and contributing, bounce hits on emitters weighted by MIS; self.why counts which rule of a connection
    left a pixel undecided.

Not restated: origins outside the world, the display pass of a mode-2 frame (shader_ref64.display covers quad.frag), the
adaptive rule of the accumulation (tied to its own restatement), INDIRECT_SAMPLES other than 1.

DEEP_FLAWS plants the misreadings of these rules that a kernel and its checker could share. One replaces the name first
thought of: "wb applied where !(pl > 0)" cannot be told from the rule by construction -- pl = 0 there, so pb / (pl + pb) is
1, the value the rule states -- and mis_wb_cosine_at_hit (the bounce's pb from the cosine at the hit, not from cb) stands
in for it as the misreading of the bounce's weight.

flaws= plants one plausible misreading at a time, so the tests can show that the comparison catches it."""
import numpy as np

import deep_ref64 as DR
import shader_ref64 as R

U = R.U
MAX_RAYS = 8
E_EXP = R.E_EXP             # relative, det_expf on [-87, 0]
E_POW = 1.2e-5             # relative, det_powf(x, 5) on [0, 1] where x^5 >= 1.7e-38
E_POW_ABS = 1.7e-38
E_SINCOS = 1.2e-7          # absolute, det_sinf / det_cosf on [0, 2 pi)
BOUNCE_DIR_ERR = E_SINCOS + 2.0 * np.pi * U + 6.0 * U
SUN = 3.0
_M32 = (1 << 32) - 1
_F1E4 = np.float32(1e-4)

FLAWS = ("fifo", "exit_swap", "dim_no_scale", "bounce_offset", "no_pi_deep", "rng_row", "no_miss_absorption",
         "id_reflect_first", "id_zero_locks")
# misreadings of the path depth, the sun disc and the emitter rules (tests/test_deep_reference64.py)
DEEP_FLAWS = ("inner_ambient", "inner_keeps_dim", "depth_off_by_one", "sun_draws_after_bounce", "sun_unit_length", "sun_glass_ndotl",
              "emit_origin_2e3", "emit_draw_order", "emit_keeps_bounce_emission", "emit_any_emitter", "power_six_faces", "power_no_p",
              "mis_m_of_cube", "mis_wb_cosine_at_hit")


def _pcg(st):
    """one step of initRNG / rand's hash (comp:385-387, 391-393) on uint32 values held in int64"""
    st = (st * 747796405 + 2891336453) & _M32
    word = (((st >> ((st >> 28) + 4)) ^ st) * 277803737) & _M32
    return (word >> 22) ^ word


def init_rng(xs, ys, sample, row=1920):
    """initRNG (comp:381-388) -> rngState per pixel"""
    seed = (np.asarray(xs, np.int64) + np.asarray(ys, np.int64) * row + 123456 + (int(sample) & _M32) * 78901) & _M32
    return _pcg(seed)


def rand(state):
    """rand() (comp:390-395) -> (new state, the float32 value float(state) / 2^32 as float64)"""
    state = _pcg(state)
    return state, (state.astype(np.float64).astype(np.float32) / np.float32(4294967296.0)).astype(np.float64)


def cosine_hemisphere(n, rx, ry):
    """cosineSampleHemisphere (comp:402-417) in float64"""
    phi = 2.0 * R.PI * ry
    ct, st = np.sqrt(rx), np.sqrt(1.0 - rx)
    x, z = st * np.cos(phi), st * np.sin(phi)
    up = np.where((np.abs(n[:, 2]) < 0.999)[:, None], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0])
    t = np.cross(up, n)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(n, t)
    r = t * x[:, None] + b * z[:, None] + n * ct[:, None]
    return r / np.linalg.norm(r, axis=1, keepdims=True)


def _spacing_below(P):
    """the float32 spacing just below |P| (0 at P == 0)"""
    a = np.abs(P).astype(np.float32)
    return np.where(a > 0, a - np.nextafter(a, np.float32(0)), 0.0).astype(np.float64)


def _reflect_origin(P, s, err, K=8):
    """float32 hitPoint[axis] + normal[axis]*1e-4 of a reflected ray (comp:559): the landing L on the plane P, pushed by
    s*1e-4 (comp:304), then moved back by the normal -s. Every float32 L within err of P is tried
    -> (origin coordinate of L == P, alike: all of them floor alike, spread: bound on |origin - that coordinate|)"""
    P32 = P.astype(np.float32)
    s32 = s.astype(np.float32)

    def origin(L):
        L1 = (L + s32 * _F1E4).astype(np.float32)
        return (L1 + (-s32) * _F1E4).astype(np.float32)

    o0 = origin(P32)
    f0 = np.floor(o0)
    alike = np.ones(P.size, bool)
    spread = np.zeros(P.size)
    for direction in (np.float32(np.inf), np.float32(-np.inf)):
        L = P32.copy()
        for _ in range(K):
            L = np.nextafter(L, direction)
            inside = np.abs(L.astype(np.float64) - P) <= err
            o = origin(L)
            alike &= ~inside | (np.floor(o) == f0)
            spread = np.where(inside, np.maximum(spread, np.abs(o.astype(np.float64) - o0)), spread)
        more = np.abs(L.astype(np.float64) - P) <= err                        # more than K float32 values within err
        alike &= ~more
        spread = np.where(more, err + 4 * np.spacing(np.abs(P32)).astype(np.float64), spread)
    return o0.astype(np.float64), alike, spread


class _March:
    pass


def _corner_undecided(w, new, mp, ax, sgn, cur, nxt, near):
    """a step that lands within the margin of a plane of another axis j (`near`) may, in float32, cross that plane first: the run
    is then in the cell on the far side of j and the near side of the crossed axis, which the alternatives of R._floor_undecided
    (all on the far side of the crossed axis) do not hold. True where that cell belongs to neither the node left nor the node
    entered (a connection aimed at the rim of an emitter's face clips such corners)"""
    und = np.zeros(new.shape[0], bool)
    rows = np.nonzero(near.any(1))[0]
    if not rows.size:
        return und
    other = np.array([[1, 2], [0, 2], [0, 1]])[ax[rows]]
    for pick in ((0,), (1,), (0, 1)):
        js = other[:, list(pick)]
        ok = np.all(near[rows[:, None], js], 1)
        q, jq = rows[ok], js[ok]
        if not q.size:
            continue
        alt = mp[q].copy()
        alt[np.arange(q.size), ax[q]] -= sgn[q].astype(np.int64)
        for c in range(jq.shape[1]):
            j = jq[:, c]
            v = new[q, j]
            alt[np.arange(q.size), j] += np.where(v >= np.rint(v), -1, 1)
        inw = w.in_world(alt)
        node = np.full(q.size, -2, np.int64)
        node[inw] = w.find(alt[inw])
        und[q[(node != cur[q]) & (node != nxt[q])]] = True
    return und


def march(w, org, err3, d, dir_err, iof, oax, lock_ax, lock_p, lo3=None, given=None, corners=False):
    """hitMarching (comp:248-330) for rays from grid-space origins org[n, 3] (per-axis error err3) with rayIOF iof.
    oax: an axis whose start floor is already decided (-1: none); lock_ax / lock_p: a coordinate that moves away from
    the plane lock_p and cannot cross it again (-1: none); lo3: per-axis error the ray's line keeps however often a
    coordinate lands on a plane (default: the origin's error). -> _March (hit, mp, pt, ax, hv, lv, err3, snap, P, amb)"""
    n = org.shape[0]
    m = _March()
    m.amb = np.zeros(n, bool)
    m.hit = np.zeros(n, bool)
    m.mp = np.zeros((n, 3), np.int64)
    m.pt = np.zeros((n, 3))
    m.ax = np.zeros(n, np.int64)
    m.hv = np.zeros(n, np.int64)
    m.lv = np.zeros(n, np.int64)
    m.err3 = err3.copy()
    lo3 = err3 if lo3 is None else lo3
    m.snap = np.zeros(n, bool)
    m.P = np.zeros(n)
    m.line = np.zeros(n)
    m.line3 = np.zeros((n, 3))
    if not n:
        return m
    small = np.any((d != 0) & (np.abs(d) < np.maximum(R.DIR_MARGIN, 2.0 * dir_err)[:, None]), 1)
    if given is not None:                               # a caller's direction: its error is relative (R.dir_undecided)
        small &= given == 0
    m.amb |= small
    start = np.floor(org).astype(np.int64)
    inw = w.in_world(start)
    m.amb |= ~inw                                       # octreeFind's early return leaves the node box undefined (comp:143)
    node = np.full(n, -1, np.int64)
    node[inw] = w.find(start[inw])
    margin = np.where(np.arange(3)[None] == oax[:, None], -1.0, R.DELTA_FLOOR + R.DELTA_SAFETY * err3)
    near = (org != np.rint(org)) & (np.abs(org - np.rint(org)) < margin)
    m.amb |= R._floor_undecided(w, org, start, node, near)
    pos = org.copy()
    inv = R._inv_dir(d)
    steps = np.zeros(n, np.int64)
    trav = np.zeros(n)
    act = np.nonzero(~m.amb)[0]
    for it in range(R.PRIMARY_CAP):
        if not act.size:
            break
        cur = node[act]
        new, ax, stuck, fr, t = R._step(w, pos[act], d[act], inv[act], cur, 1e-4)
        r = np.arange(act.size)
        dax = d[act][r, ax]
        P = np.where(dax > 0, w.mx[cur][r, ax], w.mn[cur][r, ax]).astype(np.float64)
        span = np.abs(P - pos[act][r, ax])
        with np.errstate(invalid="ignore", over="ignore"):
            e = m.err3[act] + (R._step_error(new, t) + dir_err[act] * np.abs(t))[:, None]
        lk = lock_ax[act]
        has = np.nonzero(lk >= 0)[0]
        if has.size:
            onp = np.rint(new[has, lk[has]]) == lock_p[act][has]
            fr[has[onp], lk[has[onp]]] = np.inf
        with np.errstate(invalid="ignore"):
            mp = np.floor(np.clip(new, -2.0 ** 40, 2.0 ** 40)).astype(np.int64)
        ax_in = (mp[r, ax] >= w.wmin[ax]) & (mp[r, ax] < w.wmax[ax])
        go = w.in_world(mp) & ~stuck
        nxt = np.full(act.size, -1, np.int64)
        nxt[go] = w.find(mp[go])
        near = (ax_in & ~stuck)[:, None] & (fr < R.DELTA_FLOOR + R.DELTA_SAFETY * e)
        m.amb[act] |= R._floor_undecided(w, new, mp, nxt, near)
        if corners:
            m.amb[act] |= _corner_undecided(w, new, mp, ax, np.sign(dax), cur, nxt, near)
        sn = (8.0 * U * (span + e[r, ax]) < _spacing_below(P) / 2) & ~near.any(1)
        s32 = np.sign(dax).astype(np.float32)
        new[sn, ax[sn]] = (P[sn].astype(np.float32) + s32[sn] * _F1E4).astype(np.float32)
        # the crossed coordinate is the plane, computed: off by 4u |P - pos| and two roundings whatever pos's error was
        e = np.maximum(e, lo3[act])
        land = 4.0 * U * (span + e[r, ax]) + 2.0 * np.spacing(np.abs(P).astype(np.float32)).astype(np.float64)
        dec_ax = ~near.any(1)
        e[r[dec_ax], ax[dec_ax]] = np.minimum(e[r[dec_ax], ax[dec_ax]], land[dec_ax])
        e[sn, ax[sn]] = 0.0
        steps[act] = it + 1
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            trav[act] += np.abs(t)
            # the float32 run follows its own line, o + (d + delta) s: where it meets the plane of axis b after a path s,
            # coordinate a is off by s (delta_a - delta_b d_a / d_b), whatever the planes crossed on the way reset
            line = (trav[act] * (dir_err[act] + 6.0 * U))[:, None] * (1.0 + np.abs(d[act] / dax[:, None]))
        line[r, ax] = 0.0
        line = np.where(np.isfinite(line), line, np.inf)
        pos[act], m.err3[act] = new, e
        prev = cur
        pr = np.where(w.refractive[prev], w.refr[prev], iof[act])              # comp:318
        cr = np.where(w.refractive[np.maximum(nxt, 0)], w.refr[np.maximum(nxt, 0)], 1.0)   # comp:319
        hit = go & (np.abs(cr - pr) > 1e-4)                                    # comp:321
        h = act[hit]
        m.hit[h] = True
        m.mp[h], m.pt[h], m.ax[h] = mp[hit], new[hit], ax[hit]
        m.hv[h], m.lv[h], m.snap[h], m.P[h] = nxt[hit], prev[hit], sn[hit], P[hit]
        m.line[h] = line[hit].max(1)
        m.line3[h] = line[hit]
        node[act] = nxt
        act = act[go & ~hit]
    m.amb[act] = True                                                          # capped while still moving
    m.amb |= steps > R.PRIMARY_DECIDED_STEPS
    return m


_FIELDS = {"org": 3, "err3": 3, "lo3": 3, "d": 3, "dir_err": 0, "iof": 0, "w": 0, "tint": 3, "dim": 0, "edim": 0, "mc": 3, "md": 0,
           "depth": 0, "rel": 0, "oax": 0, "lock_ax": 0, "lock_p": 0, "given": 0, "cb": 0, "xerr": 3}
_INT = ("depth", "oax", "lock_ax", "given")
STATS = ("rays", "peak_stack", "dropped_refract", "tir", "exit_glass", "deep_emission", "deep_sky", "miss_absorbed",
         "hit_absorbed", "glass_hits", "deep_ambient", "id_zero_hit", "id_reentry",
         # per ray, for the path depth, the sun disc and the emitter rules
         "shadowing", "inner", "terminal", "sun_differs", "conn_drawn", "conn_marched", "conn_contributing", "mis_bounce_hits")


class PathTrace:
    """pathTrace in VRT_MODE_FULL for every requested pixel at initRNG sample `sample`; frame() assembles the outputs."""

    def __init__(self, world, inv_proj, inv_view, cam_pos, width, height, xs=None, ys=None, sample=0, voxel_scale=1.0,
                 global_light=(1.0, 1.0, 1.0, 1.0), light_dir=None, highlighted=(-1, -1, -1), flaws=(), depth=1, tan_radius=0.0,
                 emit=None, mis=False):
        """a frame: one origin (cameraPos), ray_dirs' directions, the frame's width"""
        self._uniforms(world, voxel_scale, global_light, light_dir, highlighted, flaws, depth, tan_radius, emit, mis)
        self.W, self.H = int(width), int(height)
        if xs is None:
            ys, xs = np.mgrid[0:self.H, 0:self.W]
        self.xs, self.ys = np.asarray(xs, np.int64).ravel(), np.asarray(ys, np.int64).ravel()
        self.cam = np.array(cam_pos, np.float32).astype(np.float64)[:3]
        P = np.array(inv_proj, np.float32).astype(np.float64).reshape(4, 4).T
        Vw = np.array(inv_view, np.float32).astype(np.float64).reshape(4, 4).T
        d = R.ray_dirs(P, Vw, self.xs, self.ys, self.W, self.H, "pixel_center" in self.flaws)
        self.rng = init_rng(self.xs, self.ys, sample, self.W if "rng_row" in self.flaws else 1920)
        self._run(self.cam, d, np.ones(d.shape[0]), given=False)
        if self.outside.any():
            raise ValueError("eye outside the world: octreeFind's early return leaves the node box undefined (comp:143)")

    @classmethod
    def rays(cls, world, origins, dirs, width, sample=0, voxel_scale=1.0, global_light=(1.0, 1.0, 1.0, 1.0), light_dir=None,
             highlighted=(-1, -1, -1), flaws=(), depth=1, tan_radius=0.0, emit=None, mis=False):
        """a ray batch (include/vrt.h, "Rays", "Direction", "width"): origins float32 (n, 3) or (3,) shared, in world units;
        dirs float32 (n, 3) as given, any length; ray i of sample `sample` seeds initRNG((i % width, i // width), sample)"""
        self = cls.__new__(cls)
        self._uniforms(world, voxel_scale, global_light, light_dir, highlighted, flaws, depth, tan_radius, emit, mis)
        d, length = R.given_dirs(dirs)
        self.W = int(width)
        self.xs, self.ys = R.batch_pixels(d.shape[0], self.W, self.flaws)
        self.H = int(self.ys.max()) + 1 if d.shape[0] else 0
        self.rng = init_rng(self.xs, self.ys, sample, self.W if "rng_row" in self.flaws else 1920)
        self._run(np.array(origins, np.float32).astype(np.float64), d, length, given=True)
        return self

    def _uniforms(self, world, voxel_scale, global_light, light_dir, highlighted, flaws, depth=1, tan_radius=0.0, emit=None, mis=False):
        """the shader's uniforms and the context state of include/vrt.h: depth (the path depth D), tan_radius (the sun disc),
        emit (None: sampling off; the importance by name) and mis (read only under the power rule with a list that is not empty)"""
        assert light_dir is not None, "lightDir is a uniform: pass the host's float32 value"
        assert 1 <= int(depth) <= 8 and 0.0 <= float(tan_radius) <= 1.0 and emit in (None, "uniform", "power"), (depth, tan_radius, emit)
        self.D, self.sun_s = int(depth), float(np.float32(tan_radius))
        self.em = DR.Emitters(world) if emit is not None else None
        self.emit = emit if self.em is not None and self.em.N > 0 else None
        self.mis = bool(mis) and self.emit == "power"
        self.sun = DR.sun_basis(light_dir) if self.sun_s > 0 else None
        unknown = set(flaws) - set(FLAWS) - set(R.FLAWS) - set(R.RAY_FLAWS) - set(DEEP_FLAWS)
        assert not unknown, unknown
        self.w, self.flaws = world, frozenset(flaws)
        self.scale = float(np.float32(voxel_scale))
        self.gl = np.array(global_light, np.float32).astype(np.float64)
        self.L = np.array(light_dir, np.float32).astype(np.float64)
        self.hl = np.array(highlighted, np.int64)

    @classmethod
    def lens(cls, world, rays, voxel_scale=1.0, global_light=(1.0, 1.0, 1.0, 1.0), light_dir=None, highlighted=(-1, -1, -1),
             flaws=(), depth=1, tan_radius=0.0, emit=None, mis=False):
        """a jittered and / or thin-lens sample of the accumulation (include/vrt.h VRT_ACCUM_JITTER, vrt_set_lens): `rays` is
        tests/lens_ref64.py's lens_rays(camera block, W, H, xs, ys, sample, jitter, aperture, focus) -- per-ray float64
        origins and unit directions with the bounds of their float32 counterparts; initRNG(pixel, sample)"""
        self = cls.__new__(cls)
        self._uniforms(world, voxel_scale, global_light, light_dir, highlighted, flaws, depth, tan_radius, emit, mis)
        self.W, self.H, self.xs, self.ys = rays.W, rays.H, rays.xs, rays.ys
        self.rng = init_rng(self.xs, self.ys, rays.rng_sample, 1920)
        self._run(rays.o, rays.d, np.ones(rays.d.shape[0]), given=False, err3=rays.err_o * abs(self.scale) + U * np.abs(rays.o * self.scale),
                  dir_err=rays.dir_err, medium_org=rays.medium_org, measure_org=rays.measure_org, amb=rays.amb)
        return self

    def _run(self, origins, d, length, given, err3=None, dir_err=None, medium_org=None, measure_org=None, amb=None):
        """the entry the constructors share: world-space origins (3,) or (n, 3), unit directions d[n, 3] in float64,
        length[n]: |dir| as given (1 for a frame); given: the directions are a caller's (R.given_dirs). Optional, for
        computed rays (R.Trace._trace has the same): err3[n, 3] the origin's bound in grid units on top of ray_start's
        rounding, dir_err[n] the primary ray's direction bound, amb[n] rays undecided before they start, medium_org /
        measure_org (planted misreadings only)"""
        w, n = self.w, d.shape[0]
        self.org = np.broadcast_to(origins.reshape(-1, 3), (n, 3)).copy()
        self.tlen = length if "rays_dir_length" in self.flaws else np.ones(n)
        st = R.ray_start(w, self.org, self.scale, self.flaws, err3)
        if medium_org is not None:
            m = R.ray_start(w, np.broadcast_to(medium_org, self.org.shape), self.scale)
            st.node, st.iof, st.mc, st.md = m.node, m.iof, m.mc, m.md
        self.dim_org = None
        if measure_org is not None:
            self.org = np.broadcast_to(measure_org, self.org.shape).copy()
            self.dim_org = self.org * self.scale
        self.outside = st.outside
        self.amb = st.amb | (R.dir_undecided(d, given) & ~st.outside)
        if amb is not None:
            self.amb |= amb
        self.eye_node = st.node
        S = {k: np.zeros((n, MAX_RAYS, c) if c else (n, MAX_RAYS), np.int64 if k in _INT else np.float64)
             for k, c in _FIELDS.items()}
        self.sp = np.where(st.outside, 0, 1).astype(np.int64)
        S["org"][:, 0] = np.where(st.outside[:, None], 0.0, st.gro)
        S["err3"][:, 0] = S["lo3"][:, 0] = st.err
        S["d"][:, 0] = np.where(st.outside[:, None], 1.0, d)
        S["dir_err"][:, 0] = R.GIVEN_DIR_ERR if given else (0.0 if dir_err is None else dir_err)
        S["iof"][:, 0] = st.iof                                                 # comp:448-449
        S["w"][:, 0] = 1.0
        S["tint"][:, 0] = self.gl[:3]
        S["mc"][:, 0] = st.mc                                                   # comp:460
        S["md"][:, 0] = st.md                                                   # comp:461
        S["oax"][:, 0] = S["lock_ax"][:, 0] = -1
        S["given"][:, 0] = 1 if given else 0
        self.S = S
        self.fc = np.zeros((n, 3))
        self.cerr = np.zeros((n, 3))
        self.ncon = np.zeros(n, np.int64)
        self.id = np.zeros(n, np.int64)
        self.dist = np.full(n, int(w.wmax[0] - w.wmin[0]), np.int64)            # comp:441
        self.und_dist = np.zeros(n, bool)
        self.first_hit = np.zeros(n, bool)
        self.stats = {k: np.zeros(n, np.int64) for k in STATS}
        self.id_written = np.zeros(n, bool)
        self.why = {}
        for _ in range(1024):
            act = np.nonzero((self.sp > 0) & ~self.amb)[0]
            if not act.size:
                break
            self._pass(act)
        else:
            raise AssertionError("a ray tree of more than 1024 rays")

    # ---- one pass: the top ray of every pixel in act ----------------------------------------------------------------
    def _pop(self, act):
        S = self.S
        if "fifo" in self.flaws:
            ray = {k: v[act, 0].copy() for k, v in S.items()}
            for v in S.values():
                v[act, :-1] = v[act, 1:]
            self.sp[act] -= 1
        else:
            self.sp[act] -= 1
            ray = {k: v[act, self.sp[act]].copy() for k, v in S.items()}
        return ray

    def _push(self, idx, **f):
        sl = self.sp[idx]
        assert np.all(sl < MAX_RAYS)
        for k, v in f.items():
            self.S[k][idx, sl] = v
        self.sp[idx] += 1
        self.stats["peak_stack"][idx] = np.maximum(self.stats["peak_stack"][idx], self.sp[idx])

    def _undecide(self, idx, mask, why):
        """pixels idx[mask] are undecided; self.why counts the pixels each rule of the emitter connections was first to leave out"""
        self.why[why] = self.why.get(why, 0) + int((mask & ~self.amb[idx]).sum())
        self.amb[idx] |= mask

    def _add(self, idx, c, rel):
        self.fc[idx] += c
        self.cerr[idx] += c * rel[:, None]
        self.ncon[idx] += 1

    def _pass(self, act):
        w, fl = self.w, self.flaws
        r = self._pop(act)
        self.stats["rays"][act] += 1
        m = march(w, r["org"], r["err3"], r["d"], r["dir_err"], r["iof"], r["oax"], r["lock_ax"], r["lock_p"], r["lo3"], r["given"])
        self.amb[act] |= m.amb
        one = self.stats["rays"][act] == 1                                          # the primary ray
        self.first_hit[act[one]] = m.hit[one]
        ok = ~m.amb
        tint, wt, depth = r["tint"], r["w"], r["depth"]
        deep_pi = 1.0 if "no_pi_deep" in fl else R.PI

        # ---- misses (comp:480-495) ----
        mi = np.nonzero(ok & ~m.hit)[0]
        if mi.size:
            tc = tint[mi].copy()
            rel = r["rel"][mi] + 6 * U
            shallow = depth[mi] <= 0
            ab = shallow & (r["dim"][mi] > 1e-6) & (r["md"][mi] > 0.0) & ("no_miss_absorption" not in fl)
            self.amb[act[mi]] |= shallow & (r["md"][mi] > 0) & (np.abs(r["dim"][mi] - 1e-6) <= r["edim"][mi])
            if ab.any():
                f, e = self._absorb(r["md"][mi[ab]], r["dim"][mi[ab]], r["edim"][mi[ab]], r["mc"][mi[ab]])
                tc[ab] *= f
                rel[ab] += e
                self.stats["miss_absorbed"][act[mi[ab]]] += 1
            sun = 1.0 if "hdr_deep_sky_no_sun" in fl else SUN
            c = np.where(shallow[:, None], self.gl[:3] * R.SKY * tc * wt[mi, None], tc * R.SKY * sun * wt[mi, None] / deep_pi)
            # sky seen by an exact ray (rel 0): the float32 products of comp:489 may be exact too (a white globalLight)
            f32 = ((self.gl[:3].astype(np.float32) * R.SKY.astype(np.float32)) * tc.astype(np.float32)) * wt[mi, None].astype(np.float32)
            exact = shallow & ~ab & (r["rel"][mi] == 0) & np.all(f32.astype(np.float64) == c, 1)
            rel[exact] = 0.0
            self._add(act[mi], c, rel)
            self.stats["deep_sky"][act[mi[~shallow]]] += 1

        # ---- hits ----
        hi = np.nonzero(ok & m.hit)[0]
        if not hi.size:
            return
        idx = act[hi]
        k = hi.size
        kr = np.arange(k)
        org, d, dep = r["org"][hi], r["d"][hi], depth[hi]
        if self.dim_org is not None:
            org = np.where(one[hi][:, None], self.dim_org[idx], org)
        derr = r["dir_err"][hi] + 8 * U
        hv, lv, ax, pt, mp = m.hv[hi], m.lv[hi], m.ax[hi], m.pt[hi], m.mp[hi]
        perr = m.err3[hi]
        s = -np.sign(d[kr, ax])                                                  # comp:294
        normal = np.zeros((k, 3))
        normal[kr, ax] = s
        hpw = pt / self.scale                                                    # comp:498
        ln = np.linalg.norm(hpw - org, axis=1) * np.where(r["given"][hi] == 1, self.tlen[idx], 1.0)
        dim = r["dim"][hi] + (ln if "dim_no_scale" in fl else ln / self.scale)  # comp:501
        lerr = m.line[hi] / self.scale                                           # the hit point's deviation across the ray
        # the same per axis in grid units, with what the ray's origin was off by across its own parent: an origin moved by e moves
        # the point where the line meets the plane of axis b by e_a + e_b |d_a / d_b| in coordinate a, and not at all in b
        # (connections and MIS densities read it; two hits in a row on planes of one axis do not amplify it)
        with np.errstate(divide="ignore", invalid="ignore"):
            xo = r["xerr"][hi]
            xe = xo + xo[kr, ax][:, None] * np.abs(d / d[kr, ax][:, None]) + m.line3[hi]
        xe = np.where(np.isfinite(xe), xe, np.inf)
        xe[kr, ax] = 0.0
        edim = r["edim"][hi] + lerr + (perr.max(1) + r["err3"][hi].max(1) + 4 * U * (np.abs(hpw).max(1) + np.abs(org).max(1) + ln)) / self.scale
        # a ray of depth >= 2 starts from a vertex that its chain has moved (xo) and ends on one that it moves on (xe): its length,
        # and so its distance in the medium, changes by no more than both displacements. A ray of depth 1 starts from the primary
        # hit, whose deviation it already carries in edim, as at D = 1.
        chain = dep >= 2
        if chain.any():
            xn = np.where(chain, (np.linalg.norm(xo, axis=1) + np.linalg.norm(xe, axis=1)) / self.scale, 0.0)
            self.amb[idx] |= ~np.isfinite(xn)
            edim = edim + np.where(np.isfinite(xn), xn, 0.0)
        hva, lva = w.a[hv] > 0, w.a[lv] > 0
        n2 = np.where(w.refractive[hv], w.refr[hv], 1.0)                         # comp:503, 507
        n1 = np.where(w.refractive[lv], w.refr[lv], 1.0)                         # comp:504, 508
        sc = np.where(hva[:, None], w.rgb[hv], w.rgb[lv]) / 255.0               # comp:506
        sa = np.where(hva, w.a[hv], w.a[lv]) / 255.0
        lv_rgb, lv_md = w.rgb[lv] / 255.0, w.a[lv] / 255.0 * 5.0
        hv_rgb, hv_md = w.rgb[hv] / 255.0, w.a[hv] / 255.0 * 5.0
        tc = tint[hi].copy()
        rel = r["rel"][hi].copy()
        md, mc = r["md"][hi], r["mc"][hi]
        self.amb[idx] |= (md > 0) & (np.abs(dim - 1e-6) <= edim)
        ab = (dim > 1e-6) & (md > 0.0)                                           # comp:512-516
        if ab.any():
            f, e = self._absorb(md[ab], dim[ab], edim[ab], mc[ab])
            tc[ab] *= f
            rel[ab] += e
            self.stats["hit_absorbed"][idx[ab]] += 1
        hl = np.all(mp == self.hl, 1)                                            # comp:518-520
        sc[hl] = 1.0 - sc[hl]
        sa[hl] = 1.0
        cosi = np.einsum("ij,ij->i", d, normal)                                  # comp:522-526
        self.amb[idx] |= np.abs(cosi) < r["dir_err"][hi] + R.DIR_MARGIN
        flip = cosi > 0
        normal[flip] = -normal[flip]
        swap = flip | (("exit_swap" in fl) & (n1 > n2))
        n1, n2 = np.where(swap, n2, n1), np.where(swap, n1, n2)
        eta = n1 / n2                                                            # GLSL refract
        dd = np.einsum("ij,ij->i", normal, d)
        kk = 1.0 - eta * eta * (1.0 - dd * dd)
        tir = kk < 0.0                                                           # refract returns 0: |0| < 0.001
        sq = np.sqrt(np.maximum(kk, 0.0))
        refr = eta[:, None] * d - (eta * dd + sq)[:, None] * normal
        refr[tir] = 0.0
        R0 = (n1 - n2) / (n1 + n2) * (n1 - n2) / (n1 + n2)                       # comp:529-531
        cos_t = np.maximum(0.0, -dd)
        pw = (1.0 - cos_t) ** 5
        fres = np.clip(R0 + (1.0 - R0) * pw, 0.0, 1.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            e_f = (R0 * (8 * U + 4 * U * (n1 + n2) / np.where(n1 != n2, np.abs(n1 - n2), 1.0)) + E_POW * pw + E_POW_ABS
                   + 5.0 * (1.0 - cos_t) ** 4 * derr + 3 * U)
        refl_i = fres
        refr_i = np.where(tir, 0.0, 1.0 - fres)
        ndotl = np.maximum(normal @ self.L, 0.0)                                 # comp:537

        # ---- voxel ID and dist (comp:539-544) ----
        open_id = ~self.id_written[idx] if "id_zero_locks" in fl else self.id[idx] == 0
        idset = (dep == 0) & open_id & (sa >= 1.0)
        if idset.any():
            j = idx[idset]
            self.stats["id_reentry"][j] += self.stats["id_zero_hit"][j] > 0       # an earlier ID-0 hit left it open
            self.id_written[j] = True
            lin = mp[idset, 0] + w.tex_dim * (mp[idset, 1] + w.tex_dim * mp[idset, 2])
            face = ax[idset] * 2 + np.where(s[idset] > 0, 0, 1)
            if "face_order" in fl:
                face ^= 1
            self.id[j] = ((lin * 6 + face + (1 << 31)) % (1 << 32)) - (1 << 31)
            eye = self.org[0] if "rays_dist_from_first_origin" in fl else self.org[j]
            lc = np.linalg.norm(hpw[idset] - eye, axis=1) * self.tlen[j]
            self.dist[j] = np.trunc(lc)
            margin = (R.DELTA_FLOOR + R.DELTA_SAFETY * perr[idset].max(1)) / self.scale + 4 * U * lc
            self.und_dist[j] = np.abs(lc - np.rint(lc)) < margin
            self.stats["id_zero_hit"][j] += self.id[j] == 0

        # ---- glass at depth <= 0 (comp:547-572) ----
        glass = (dep <= 0) & (sa < 1.0)
        g = np.nonzero(glass)[0]
        if g.size:
            gi = idx[g]
            self.stats["glass_hits"][gi] += 1
            self.stats["tir"][gi] += tir[g]
            self.stats["exit_glass"][gi] += n1[g] > n2[g]
            sp = self.sp[gi]
            wg = r["w"][hi][g]
            rw = wg * refl_i[g]
            und = (np.abs(refl_i[g] - 0.001) <= e_f[g]) | (~tir[g] & (np.abs(refr_i[g] - 0.001) <= e_f[g]))
            und |= np.abs(kk[g]) <= 6 * U * (1 + eta[g] ** 2) + 2 * eta[g] ** 2 * np.abs(dd[g]) * derr[g]
            und |= np.abs(rw - 1e-4) <= wg * e_f[g] + rw * (rel[g] + 2 * U)
            self.amb[gi] |= und
            fall = (sp == MAX_RAYS) | (refl_i[g] <= 0.001) | (refr_i[g] <= 0.001)
            fb = g[fall]
            if fb.size:
                nd_fb = ndotl[fb]                                                # point 4 of the sun disc: ndotl from L
                if self.sun is not None and "sun_glass_ndotl" in fl:
                    st, u1 = rand(self.rng[idx[fb]])
                    self.rng[idx[fb]], u2 = rand(st)
                    nd_fb = np.maximum((normal[fb] * DR.sun_dirs(self.sun, self.sun_s, u1, u2, fl)).sum(1), 0.0)
                c = tc[fb] * (sc[fb] * (self.gl[:3] * nd_fb[:, None])) * r["w"][hi][fb, None]
                self._add(idx[fb], c, rel[fb] + 5 * U)
            sp_g = g[~fall]
            if sp_g.size:
                self._spawn_glass(idx[sp_g], d=d[sp_g], normal=normal[sp_g], pt=pt[sp_g], perr=perr[sp_g], ax=ax[sp_g],
                                  P=m.P[hi[sp_g]], hv=hv[sp_g], lv=lv[sp_g], iof=r["iof"][hi[sp_g]], w=r["w"][hi[sp_g]],
                                  rel=rel[sp_g], tc=tc[sp_g], fres=fres[sp_g], e_f=e_f[sp_g], n1=n1[sp_g], n2=n2[sp_g],
                                  dep=dep[sp_g], tir=tir[sp_g], refr=refr[sp_g], eta=eta[sp_g], dd=dd[sp_g], kk=kk[sp_g],
                                  dir_err=r["dir_err"][hi[sp_g]], dim=dim[sp_g], edim=edim[sp_g], lerr=lerr[sp_g], lv_rgb=lv_rgb[sp_g],
                                  lv_md=lv_md[sp_g], hv_rgb=hv_rgb[sp_g], hv_md=hv_md[sp_g], xerr=xe[sp_g])
        # ---- opaque, and glass deeper (comp:573-618) ----
        o = np.nonzero(~glass)[0]
        if not o.size:
            return
        em = np.where(hva[o], w.p[hv[o], 1] / 255.0, 0.0) * 10.0                 # comp:575
        em0 = em / 10.0 if "hdr_emission_x1" in fl else em
        wo = r["w"][hi][o]
        base = sc[o] * tc[o] * wo[:, None]
        e0 = (em > 0) & (dep[o] == 0)
        e1 = (em > 0) & (dep[o] != 0)
        if e0.any():
            self._add(idx[o[e0]], base[e0] * em0[e0, None], rel[o[e0]] + 5 * U)
        if e1.any():
            self._deep_emission(idx[o[e1]], base[e1] * em[e1, None] / deep_pi, rel[o[e1]] + 6 * U, r, hi[o[e1]], m, xe[o[e1]])
        Dt = max(self.D - 1, 1) if "depth_off_by_one" in fl else self.D
        dull = em <= 0
        inner = dull & (dep[o] >= 1) & (dep[o] < Dt)
        deep = dull & (dep[o] >= Dt)                                              # the terminal branch (comp:590-594)
        if "inner_ambient" in fl:
            deep = deep | inner
        if deep.any():
            q = o[deep]
            ex = np.exp(-dim[q] / 512.0)
            amb_c = np.maximum(1.0 - ex, 0.01)
            e_amb = E_EXP * ex + ex * (edim[q] + 2 * U * dim[q]) / 512.0 + 2 * U
            self._add(idx[q], base[deep] * amb_c[:, None] / deep_pi, rel[q] + e_amb / amb_c + 6 * U)
            self.stats["deep_ambient"][idx[q]] += 1
            self.stats["terminal"][idx[q]] += dep[q] >= self.D
        top = dull & (dep[o] < Dt)                                                # a vertex that casts a shadow ray
        if top.any():
            q = o[top]
            iq = idx[q]
            self.stats["shadowing"][iq] += 1
            self.stats["inner"][iq] += dep[q] >= 1
            assert np.all(self.sp[iq] < MAX_RAYS)                                 # comp:597: a pop came first
            # the vertex's draws, in the stream's order: the sun's two, the connection's four, the bounce's two
            st = self.rng[iq]
            draws = {}
            late_sun = "sun_draws_after_bounce" in fl
            names = (("u1", "u2") if self.sun is not None and not late_sun else ()) \
                + ((("ua", "ub", "u0", "uf") if "emit_draw_order" in fl else ("u0", "uf", "ua", "ub")) if self.emit else ()) \
                + ("rx", "ry") + (("u1", "u2") if self.sun is not None and late_sun else ())
            for name in names:
                st, draws[name] = rand(st)
            self.rng[iq] = st
            wq = r["w"][hi][q]
            # the floor margins of the shadow and bounce marches keep the per-axis bounds from vertex to vertex: a known gap
            # (module docstring, "Known unsound")
            pq = perr[q]
            if self.sun is None:
                lit, samb = R.not_in_shadow(w, pt[q], normal[q], pq.max(1), self.L, self.flaws)
                self.amb[iq] |= samb
                c = (self.gl[:3] * (lit * ndotl[q])[:, None]) * sc[q] * tc[q] * wq[:, None] / R.PI
                self._add(iq, c, rel[q] + 6 * U)
            else:
                Lp = DR.sun_dirs(self.sun, self.sun_s, draws["u1"], draws["u2"], fl)
                de = DR.sun_dir_err(self.sun_s, self.sun[0])
                lit, samb = R.not_in_shadow(w, pt[q], normal[q], pq.max(1), Lp, self.flaws, dir_err=de)
                self.amb[iq] |= samb
                lit0, _ = R.not_in_shadow(w, pt[q], normal[q], perr[q].max(1), self.L, self.flaws)
                self.stats["sun_differs"][iq] += lit != lit0
                nd = np.maximum((normal[q] * Lp).sum(1), 0.0)                        # ndotl', within de of the float32 value
                full = self.gl[:3] * sc[q] * tc[q] * wq[:, None] / R.PI
                self._add(iq, full * (lit * nd)[:, None], rel[q] + 6 * U)
                self.cerr[iq] += full * (lit * de)[:, None]
            off = 1e-4 if "bounce_offset" in fl else 1e-1
            o_ = pt[q] + normal[q] * off
            eo = pq + U * np.abs(o_)
            if self.emit:
                x = pt[q] + normal[q] * 2e-3 if "emit_origin_2e3" in fl else pt[q] + normal[q] * 1e-1
                self._connect(iq, x, perr[q] + U * np.abs(x), xe[q], normal[q], n1[q], wq, tc[q] * sc[q], rel[q] + 2 * U, lv_rgb[q], lv_md[q],
                              lerr[q], draws["u0"], draws["uf"], draws["ua"], draws["ub"])
            bd = cosine_hemisphere(normal[q], draws["rx"], draws["ry"])
            keep = (dep[q] >= 1) & ("inner_keeps_dim" in fl)
            self._push(iq, org=o_, err3=eo, lo3=eo, d=bd, dir_err=np.full(q.size, BOUNCE_DIR_ERR),
                       iof=n1[q], w=wq, tint=tc[q] * sc[q], dim=np.where(keep, dim[q], 0.0), edim=np.where(keep, edim[q], lerr[q]),
                       mc=lv_rgb[q], md=lv_md[q], depth=dep[q] + 1, rel=rel[q] + 2 * U, oax=-1, lock_ax=-1, lock_p=0.0, given=0,
                       cb=(normal[q] * bd).sum(1), xerr=xe[q])

    # ---- emitter rules (include/vrt.h "Emitter sampling", "Emitter importance", "Emitter MIS") -----------------------------
    def _deep_emission(self, iq, c, rel, r, hq, m, xe):
        """a ray of depth >= 1 on an emissive voxel (comp:575-581): the shader's term with sampling off; nothing with sampling on
        (rule 7); the term times wb under MIS. c[k, 3]: the shader's term; hq: the rays' rows in the popped arrays and the march"""
        fl = self.flaws
        if self.emit is None or "emit_keeps_bounce_emission" in fl:
            self._add(iq, c, rel)
            self.stats["deep_emission"][iq] += 1
            return
        if not self.mis:
            return
        cs = r["cb"][hq]
        derr = r["dir_err"][hq]
        if "mis_wb_cosine_at_hit" in fl:
            cs = np.abs(r["d"][hq][np.arange(hq.size), m.ax[hq]])
        ev3 = r["err3"][hq] + r["xerr"][hq] + m.err3[hq] + xe
        pl, pb, rel_pl, rel_pb, und = self._mis_density(r["org"][hq], r["err3"][hq] + r["xerr"][hq], ev3, r["d"][hq], derr, cs, m.pt[hq], m.ax[hq], m.mp[hq],
                                                        m.hv[hq])
        self._undecide(iq, und, "MIS density of a bounce hit")
        pos = pl > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            wb = np.where(pos, pb / (pl + pb), 1.0)
        self._add(iq, c * wb[:, None], rel + np.where(pos, (1.0 - wb) * (rel_pl + rel_pb), 0.0) + 3 * U)
        self.stats["deep_emission"][iq] += 1
        self.stats["mis_bounce_hits"][iq] += pos

    def _mis_density(self, x, ex3, ev3, dirv, derr, cs, pt, ax, mp, hv, m_cube=None):
        """emit_mis_density(x, dir, cs, hit) -> (pl, pb, relative bound of pl, of pb, undecided). x within ex3 per axis as the floor
        margins take it, v = hit.point - x within ev3, dir within derr per component, cs within derr. Undecided: a visible-axis test within ex3 of its plane,
        cl or cs within derr of 0 (the !(pl > 0) test, and pb's relative bound)"""
        w = self.w
        kr = np.arange(x.shape[0])
        v = pt - x
        r2 = (v * v).sum(1)
        cl = np.abs(dirv[kr, ax])
        lo = mp.astype(np.float64)
        und = np.any((np.abs(x - lo) <= ex3) | (np.abs(x - (lo + 1.0)) <= ex3), 1)
        mm = ((x < lo) | (x > lo + 1.0)).sum(1)
        if m_cube is not None:
            mm = m_cube
        wv = (w.p[hv, 1] * w.rgb[hv].sum(1)).astype(np.float64)
        und |= (cl <= derr) | (np.abs(cs) <= derr)
        ok = (mm > 0) & (cl > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            pl = np.where(ok, ((wv * self.em.inv_power) * r2) / (np.maximum(mm, 1) * np.where(ok, cl, 1.0)), 0.0)
            pb = np.maximum(cs, 0.0) / R.PI
            e_v = np.linalg.norm(ev3 + U * np.abs(v), axis=1)
            rel_pl = 2.0 * e_v / np.sqrt(np.maximum(r2, 1e-300)) + derr / np.where(ok, cl, 1.0) + 8 * U
            rel_pb = derr / np.maximum(np.abs(cs), 1e-300) + 2 * U
        return pl, pb, rel_pl, rel_pb, und

    def _connect(self, iq, x, ex3, xe3, normal, n1, wt, tint, rel, mc, md, edim0, u0, uf, ua, ub):
        """steps 1-6 of "Emitter sampling" (the uniform rule) or of "Emitter importance" (the power rule), then "Emitter MIS",
        at the shadowing vertices of pixels iq. x[k, 3]: hitPoint + normal * 1e-1 within ex3 per axis as the floor margins take it, and
        within ex3 + xe3 for the continuous quantities (xe3: the chain's deviation across its rays, 0 along the normal); n1, wt, tint, rel, mc, md: what the
        bounce ray would carry (make_ray, comp:604-615); edim0: the hit's deviation across its ray, as the bounce takes it"""
        w, fl, E = self.w, self.flaws, self.em
        k = iq.size
        kr = np.arange(k)
        self.stats["conn_drawn"][iq] += 1
        power = self.emit == "power"
        if power:
            j, p = DR.pick_power(u0, E.T)
        else:
            j, p = DR.pick_uniform(u0, E.N), np.ones(k)
        lo, sz = E.lo[j].astype(np.float64), E.size[j].astype(np.float64)
        hi_ = lo + sz[:, None]
        if power:
            low, high = x < lo, x > hi_
            self._undecide(iq, np.any((np.abs(x - lo) <= ex3 + xe3) | (np.abs(x - hi_) <= ex3 + xe3), 1), "visible face")
            vis = low | high
            mf = vis.sum(1)
            go = mf > 0
            i = DR.pick_index(uf, np.maximum(mf, 1))
            axf = np.argmax(vis & ((np.cumsum(vis, 1) - 1) == i[:, None]), 1)
            side = high[kr, axf]
        else:
            f = DR.pick_index(uf, 6)
            axf, side = f >> 1, (f & 1) == 1
            mf = np.full(k, 6)
            go = np.ones(k, bool)
        a1, a2 = (axf + 1) % 3, (axf + 2) % 3
        q = np.zeros((k, 3))
        eq = np.zeros((k, 3))
        q[kr, axf] = lo[kr, axf] + np.where(side, sz, 0.0)
        for a, u in ((a1, ua), (a2, ub)):
            q[kr, a] = lo[kr, a] + u * sz
            eq[kr, a] = U * (u * sz) + U * np.abs(q[kr, a])
        wv = q - x
        r2 = (wv * wv).sum(1)
        e3 = ex3 + xe3 + eq + U * np.abs(wv)
        e_w = np.linalg.norm(e3, axis=1)
        self._undecide(iq, go & (np.sqrt(r2) <= 2.0 * e_w), "r2 > 0")
        go &= r2 > 0
        rr = np.sqrt(np.where(r2 > 0, r2, 1.0))
        dirv = wv / rr[:, None]
        derr = R.GIVEN_DIR_ERR + e_w / rr
        cs = (normal * dirv).sum(1)
        cl = np.where(side, -dirv[kr, axf], dirv[kr, axf])
        self._undecide(iq, go & ((np.abs(cs) <= derr) | (np.abs(cl) <= derr)), "cs > 0 and cl > 0")
        go &= (cs > 0) & (cl > 0)
        g_ = np.nonzero(go & ~self.amb[iq])[0]
        if not g_.size:
            return
        gi = iq[g_]
        self.stats["conn_marched"][gi] += 1
        none = np.full(g_.size, -1, np.int64)
        ef = (ex3 + xe3)[g_]
        m = march(w, x[g_], ef, dirv[g_], derr[g_], n1[g_], none, none, np.zeros(g_.size), ef, np.zeros(g_.size, np.int64), corners=True)
        self._undecide(gi, m.amb, "the connection's march")
        h = np.nonzero(m.hit & ~m.amb)[0]
        if not h.size:
            return
        g_, gi = g_[h], gi[h]
        hr = np.arange(h.size)
        pt, mp, hv, axh = m.pt[h], m.mp[h], m.hv[h], m.ax[h]
        inside = np.all((mp >= lo[g_]) & (mp < hi_[g_]), 1)                      # step 5
        margin = R.DELTA_FLOOR + R.DELTA_SAFETY * m.err3[h]
        # for the continuous quantities: a connection that contributes ends on the face it aimed at (a face turned towards x is
        # the cube's first along the line), so wherever the float32 x lies its line runs through the float32 q, and the hit is q
        # within the march's own roundings: the per-axis bound and the deviation across the line by the rounded direction
        perr = m.err3[h] + m.line3[h] + eq[g_]
        nearp = (np.abs(pt - lo[g_]) <= margin) | (np.abs(pt - hi_[g_]) <= margin)
        nearp[hr, axh] = False
        if "emit_any_emitter" in fl:
            inside[:] = True
        else:
            self._undecide(gi, nearp.any(1), "in-cube test")
        hva = w.a[hv] > 0
        emission = np.where(hva, w.p[hv, 1] / 255.0, 0.0) * 10.0
        c_ = np.nonzero(inside & (emission > 0))[0]
        if not c_.size:
            return
        g_, gi = g_[c_], gi[c_]
        pt, mp, hv, axh, perr, emission = pt[c_], mp[c_], hv[c_], axh[c_], perr[c_], emission[c_]
        xg, exg, dg, deg = x[g_], ex3[g_], dirv[g_], derr[g_]
        # step 6: the hit of a ray of depth >= 1 up to the emissive test (comp:499-520)
        hpw = pt / self.scale
        ln = np.linalg.norm(hpw - xg, axis=1)
        dim = ln / self.scale
        edim = edim0[g_] + m.line[h][c_] / self.scale + (perr.max(1) + exg.max(1) + 4 * U * (np.abs(hpw).max(1) + np.abs(xg).max(1) + ln)) / self.scale
        edim = edim + np.linalg.norm(xe3[g_], axis=1) / self.scale             # the connection's length moves with its vertex
        tc = tint[g_].copy()
        rl = rel[g_].copy()
        self._undecide(gi, (md[g_] > 0) & (np.abs(dim - 1e-6) <= edim), "distanceInMedium > 1e-6")
        ab = (dim > 1e-6) & (md[g_] > 0.0)
        if ab.any():
            f, e = self._absorb(md[g_][ab], dim[ab], edim[ab], mc[g_][ab])
            tc[ab] *= f
            rl[ab] += e
        sc = w.rgb[hv] / 255.0
        hl = np.all(mp == self.hl, 1)
        sc[hl] = 1.0 - sc[hl]
        E_k = tc * sc * (emission * wt[g_])[:, None] / R.PI
        szg, mg, pg = sz[g_], mf[g_].astype(np.float64), p[g_]
        if power:
            if "power_six_faces" in fl:
                mg = np.full(g_.size, 6.0)
            gg = ((cs[g_] * cl[g_]) * (mg * (szg * szg))) / ((R.PI * r2[g_]) * (1.0 if "power_no_p" in fl else pg))
        else:
            gg = ((cs[g_] * cl[g_]) * ((E.N * 6.0) * (szg * szg))) / (R.PI * r2[g_])
        rl += deg / cs[g_] + deg / cl[g_] + 2.0 * e_w[g_] / rr[g_] + 14 * U
        c = E_k * gg[:, None]
        if self.mis:
            pl, pb, rel_pl, rel_pb, und = self._mis_density(xg, exg + xe3[g_], exg + xe3[g_] + perr, dg, deg, cs[g_], pt, axh, mp, hv,
                                                            mf[g_] if "mis_m_of_cube" in fl else None)
            self._undecide(gi, und, "MIS density of a connection")
            pos = pl > 0
            with np.errstate(divide="ignore", invalid="ignore"):
                wn = np.where(pos, pl / (pl + pb), 0.0)
            c, rl, gi = (c * wn[:, None])[pos], (rl + (1.0 - wn) * (rel_pl + rel_pb) + 3 * U)[pos], gi[pos]
        self._add(gi, c, rl)
        self.stats["conn_contributing"][gi] += 1

    def _spawn_glass(self, gi, d, normal, pt, perr, ax, P, hv, lv, iof, w, rel, tc, fres, e_f, n1, n2, dep, tir, refr, eta,
                     dd, kk, dir_err, dim, edim, lerr, lv_rgb, lv_md, hv_rgb, hv_md, xerr):
        """push the reflected and the refracted ray of the glass hits of pixels gi (comp:555-571); every array has one
        row per pixel: the hit (point, normal after the flip, error, axis, plane P, hit and last voxel), the popped ray
        (rayIOF, weight, direction error, distanceInMedium) and what comp:497-537 made of them"""
        kr = np.arange(gi.size)
        s = np.sign(d[kr, ax])
        Wd = self.w

        def reflect(sel):
            if not sel.any():
                return
            q = np.nonzero(sel)[0]
            rw = w[q] * fres[q]
            q, rw = q[rw > 1e-4], rw[rw > 1e-4]                                   # comp:557
            if not q.size:
                return
            qr, aq = np.arange(q.size), ax[q]
            o = pt[q] + normal[q] * 1e-4
            oc, alike, spread = _reflect_origin(P[q], s[q], perr[q, aq])
            # The start voxel is the last voxel (A: the near side of P) or the hit voxel (B). When the float32 landings
            # disagree, B is still A's tree if B's first step -- back across P, pushed 1e-4 into the last voxel -- is no
            # change of medium (comp:318-321 with rayIOF n1): then B is A's ray moved 1e-4 along the axis.
            prev_b = np.where(Wd.refractive[hv[q]], Wd.refr[hv[q]], n1[q])
            cur_b = np.where(Wd.refractive[lv[q]], Wd.refr[lv[q]], 1.0)
            same = np.abs(cur_b - prev_b) <= 1e-4
            near_side = np.nextafter(P[q].astype(np.float32), (P[q] - s[q]).astype(np.float32)).astype(np.float64)
            use_a = ~alike & same
            oc = np.where(use_a, near_side, oc)
            spread = np.where(use_a, spread + 1e-4 + 2 * np.abs(near_side - P[q]), spread)
            o[qr, aq] = oc
            self.amb[gi[q]] |= ~alike & ~same
            away = np.floor(oc) != np.floor(pt[q, aq])                           # started on the near side of P
            rd = d[q] - 2.0 * dd[q, None] * normal[q]
            e3 = perr[q] + U * np.abs(o)
            e3[qr, aq] = spread
            # the line's offset along the axis shows in the other coordinates where it crosses planes of that axis
            with np.errstate(divide="ignore", invalid="ignore"):
                e3 += spread[:, None] * np.abs(rd / rd[qr, aq][:, None])
            e3[qr, aq] = spread
            self._push(gi[q], org=o, err3=e3, lo3=e3, d=rd, dir_err=dir_err[q], iof=n1[q], w=rw, tint=tc[q], dim=dim[q],
                       edim=edim[q] + lerr[q], mc=lv_rgb[q], md=lv_md[q], depth=dep[q],
                       rel=rel[q] + e_f[q] / np.maximum(fres[q], 1e-30) + 2 * U, oax=aq,
                       lock_ax=np.where(away, aq, -1), lock_p=P[q], given=0, cb=0.0, xerr=xerr[q])

        def refract(sel):
            q = np.nonzero(sel & (self.sp[gi] < MAX_RAYS) & ~tir)[0]
            self.stats["dropped_refract"][gi[sel & (self.sp[gi] >= MAX_RAYS) & ~tir]] += 1
            if not q.size:
                return
            o = pt[q] - normal[q] * 1e-4
            sq = np.sqrt(kk[q])
            de = dir_err[q] * (eta[q] + eta[q] ** 2 * np.abs(dd[q]) / sq) + 8 * U + 4 * U * (1 + eta[q] ** 2) / sq
            self._push(gi[q], org=o, err3=perr[q] + U * np.abs(o), lo3=perr[q] + U * np.abs(o), d=refr[q] / np.linalg.norm(refr[q], axis=1, keepdims=True),
                       dir_err=de, iof=n2[q], w=w[q] * (1.0 - fres[q]), tint=tc[q], dim=0.0, edim=lerr[q], mc=hv_rgb[q],
                       md=hv_md[q], depth=dep[q], rel=rel[q] + e_f[q] / np.maximum(1.0 - fres[q], 1e-30) + 2 * U, oax=-1,
                       lock_ax=-1, lock_p=0.0, given=0, cb=0.0, xerr=xerr[q])

        first = np.ones(gi.size, bool)
        if "id_reflect_first" in self.flaws:
            refract(first)
            reflect(self.sp[gi] < MAX_RAYS)
        else:
            reflect(self.sp[gi] < MAX_RAYS)                                      # comp:555
            refract(first)                                                       # comp:565

    def _absorb(self, md, dim, edim, mc):
        """exp(-density * distanceInMedium * (1 - mediumColor)) -> (factor[k, 3], relative error bound[k])"""
        return R.absorb(md, dim, edim, mc)

    def bound(self):
        """what a float32 run's colour may differ from fc by: cerr + (ncon + 1) * u * |fc| + EPS_COLOR / 255 (the margin the
        byte test keeps around a .5 tie, in colour units); 0 for one exact term. frame()'s tie test and radiance() both
        use it, so bytes and floats are held to the same bound."""
        b = self.cerr + (self.ncon + 1)[:, None] * U * np.abs(self.fc) + R.EPS_COLOR / 255.0
        b[(self.ncon == 1) & (self.cerr == 0).all(1)] = 0.0                      # one exact term: rint's ties-to-even
        return b

    def radiance(self):
        """-> (h(fc) float64[n, 3], bound[n, 3], decided[n]): the unclamped colour through vrt.h's h (R.hdr_value)"""
        return R.hdr_value(self.fc), self.bound(), ~self.amb & ~self.outside

    def frame(self):
        """-> shader_ref64.Frame of mode 2 with every field decided or not"""
        n = self.xs.size
        f = PathFrame(self.xs, self.ys, 2)
        f.id, f.dist = self.id.copy(), self.dist.copy()
        x = np.clip(self.fc, 0.0, 1.0) * 255.0
        f.rgba = np.concatenate([np.rint(x), np.full((n, 1), 255.0)], 1).astype(np.int64)
        tie = np.abs(x - np.floor(x) - 0.5) < 255.0 * self.bound()
        f.hit = self.first_hit.copy()
        f.kind = np.where(self.first_hit, R.KIND_OPAQUE, R.KIND_SKY)
        f.outside = self.outside.copy()
        f.dec_id = ~self.amb & ~self.outside
        f.dec_dist = f.dec_id & ~self.und_dist
        f.dec_rgb = f.dec_id[:, None] & ~tie
        f.stats = {k: v.copy() for k, v in self.stats.items()}
        return f


class PathFrame(R.Frame):
    def hit_undecided_share(self):
        """of the pixels whose primary ray hits: not every field decided"""
        full = self.dec_id & self.dec_dist & self.dec_rgb.all(1)
        return float((~full[self.hit]).mean()) if self.hit.any() else 0.0

    def undecided_share(self):
        return float((~(self.dec_id & self.dec_dist & self.dec_rgb.all(1))).mean())
