"""A float64 restatement of shaders/raytracing.comp and shaders/quad.frag at voxel granularity (test helper, not a test).

Independent of oracle/rt_oracle.c and of the product's tracing: the only inputs are the texel stream (pinned to the
reference's octree_texture() by tests/golden/flatten.json), the camera block (pinned to the reference's Camera.hpp by
tests/golden/camera.json) and the shader's uniforms. Nothing here imports or loads anything under oracle/
(tests/test_shader_reference64.py enforces that).

What is restated, from the GLSL:
  * octreeFind (comp:137-220): decodePointer, the child mask in .a with bitCount offsets, the leaf colour from the node
    texel and alpha + decodeProperties from the next one, getChildBounds' truncating midpoint. The stream is decoded level
    by level into the nodes octreeFind can return (a leaf, or a missing child with its box), painted into a dense index
    grid over the leaves' bounding box padded by one voxel; points outside it take a vectorised descent.
  * hitMarching (comp:248-330) as node-to-node steps in float64, with the shader's 1e20 branch for |d| < 1e-8, its
    per-step push of 1e-4 along the crossed axis (the pushes shift the ray sideways, so they are kept) and the rule
    that a hit is a change of refraction index by more than 1e-4 (a voxel counts as air unless a > 0 and p0 > 0).
  * notInShadow (comp:333-377): origin hitPoint + normal*2e-3, pushes of 1e-3, occluders a > 0.1 && illumination == 0,
    lit on leaving the world or after 64 octreeFinds.
  * pathTrace / main (comp:435-645) for the first hit: startIOF, pixel-corner rays u = x/W*2-1, the highlight inversion
    forcing alpha to 1, voxelID = toLinear(mapPos)*6 + getFaceIndex(hitNormal) only when surfaceColor.a >= 1,
    dist = int(length(hitPoint/voxelScale - cameraPos)); colour of the primary ray for VRT_MODE_PRIMARY (0) and
    VRT_MODE_PRIMARY_SHADOW (1); in VRT_MODE_FULL (2) only what the first hit decides (id/dist of an opaque first hit,
    sky and emissive colour). The whole mode-2 ray tree -- bounce colour, in-medium absorption (exp), the glass
    stack -- is restated by tests/path_ref64.py on top of this module.
  * quad.frag: the ID-aware box blur at chosen pixels.

Undecided pixels. A pixel is left out of a comparison when float32 rounding in the shader could change the answer:
  * Position margin DELTA_FLOOR + DELTA_SAFETY * err: a crossing point lies that close to another grid plane (and the
    voxel on the other side belongs to another node), or the eye does. err bounds the float32 error of the shader's
    rayPos, accumulated along the ray with u = 2^-24: u*|eye| at the start and, per node step of length t,
    u*(10*t + |rayPos|): t itself is off by ~3u relative (plane - pos, 1/d and their product round once each), d*t and
    the sum round once each (<= u*t + u*|rayPos|), and the float32 direction is off by up to ~6u relative, which the
    step carries into the position. At |coord| <= 1024 that is at most 6.1e-5 per step plus 6e-7 per voxel travelled,
    e.g. ~2.6e-3 for 40 steps over a 1500-voxel ray; DELTA_SAFETY = 2 doubles the bound and DELTA_FLOOR = 1e-5 covers
    the exactly-integer eyes and planes. The bound grows with the real coordinates, so a model near the origin keeps
    a margin of ~1e-4 while a terrain ray at |coord| ~ 1000 gets several 1e-3.
  * DIR_MARGIN: a direction component with 0 < |d| < 1e-6 (float32 may round it to 0, flip its sign or cross the 1e-8
    branch); exact zeros come from structural zeros and are decided (such a ray never hits: comp:282-287 send it
    backwards out of the world, or it steps by zero until the cap).
  * EPS_COLOR = 2.5e-4 byte: c*255 that close to a .5 tie. The colour is a product of at most six float32-rounded
    factors and the *255 (relative error <= 7u), i.e. <= 1.1e-4 byte at 255.
  * dist: |length - round(length)| below the position margin / voxelScale (+ the float32 error of the length).
  * Caps: a shadow occluder at octreeFind 63..66 (the cap is 64), a primary path of more than 1000 node steps.
  * Display pass: the mean that close to a .5 tie, EPS_COLOR + 1.52e-5*(count+2) bytes (a float32 sum of `count` terms in
    [0, 1] is off by at most (count+1)*u relative; 255*u ~ 1.52e-5), or a radius 200/sqrt(d) within 1e-5 of an integer
    without being one exactly.

Ray batches (Trace.rays; include/vrt.h "Rays", "Direction", "width"). The camera constructor is a thin caller of the same
entry: one origin, ray_dirs' directions, the frame's width. Per ray:
  * gro = float32(origin * voxelScale) is the march's start, exactly as the shader has it; the position bound is the
    rounding |gro - origin * voxelScale| (zero when the product is exact, e.g. voxelScale 1, 0.5 or 2). An origin whose
    floor is not decided within DELTA_FLOOR + DELTA_SAFETY * that bound is undecided (exact integers are decided).
  * The start medium (startIOF, colour, density a * 5) is the voxel at floor(gro) (comp:445-461); distanceInMedium is
    length(hitPoint / voxelScale - gro) / voxelScale as the GLSL has it and dist is int(length(hitPoint / voxelScale -
    origin)), both from the ray's own origin. In modes 0 and 1 the start medium's absorption of the first hit
    (comp:512-516) is restated: its relative error is |arg| * 5u (three products and the float32 distance) +
    density * (1 - mediumColor) * (the distance's error) + E_EXP; distanceInMedium within its error of 1e-6 is undecided.
  * Direction: d * (1 / sqrt(dot(d, d))) in float32, every operation rounded once. dot is three products and two sums
    of non-negative terms (relative error <= 3u), sqrt halves that and rounds (<= 2.5u), the reciprocal rounds (<= 3.5u)
    and the product rounds (<= 4.5u): every component has RELATIVE error <= GIVEN_DIR_ERR = 4.5u, below the ~6u
    _step_error already carries for a frame's ray. So an exactly-zero component stays exactly zero with its sign, no
    component changes sign, and the 1e-8 branch is the float32 run's unless |d| lies within BRANCH_MARGIN (1e-5 relative)
    of 1e-8: given components below DIR_MARGIN are decided by restating the shader's rule for them (the 1e20 branch
    sends such a ray backwards out of the world), as the zero_direction edge case does for exact zeros.
  * The RNG pixel of ray i is (i % width, i // width) (mode 2: tests/path_ref64.py; modes 0 and 1 draw nothing).
  * Origins outside the world are not restated: octreeFind's early return leaves the node box undefined (comp:143).
    They are reported in `outside`, never compared, and counted neither as decided nor as undecided.

Jittered and thin-lens samples (Trace.lens; include/vrt.h VRT_ACCUM_JITTER, vrt_set_lens). tests/lens_ref64.py restates
the sample's rays in float64 with a per-axis origin bound and a per-ray direction bound; _trace takes them as optional
inputs: the origin bound joins ray_start's rounding (the floor of the origin, the position error, the distances), the
direction bound adds dir_err * t to every step's position error and makes a component within 2 * dir_err of 0 undecided.
Still not restated: origins outside the world, the adaptive rule, INDIRECT_SAMPLES other than 1 (path depth, the sun disc
and the emitter rules: tests/path_ref64.py; notInShadow takes the disc's per-ray direction with its bound).

Radiance. colour_bound is the one bound on a colour: rel * |c| + EPS_COLOR / 255, rel = 7u for the products (+ the
absorption's terms), 0 for a sky whose float32 products are exact. frame()'s tie test and radiance() both call it.
radiance() returns (h(c), bound, decided) with h of vrt_accum_keep_hdr point 1 (clamp to [0, 65504]; 1-Lipschitz, so the
bound holds after clamping both sides). hdr_mean and tonemap restate vrt.h points 2-4 in float64 with the bound carried.

flaws= plants one plausible misreading at a time, so the tests can show that the comparison catches it (FLAWS: the
frame's; RAY_FLAWS: the ray-batch entry's and the HDR arithmetic's, kept apart because the frame tests pin FLAWS)."""
import numpy as np

U = 2.0 ** -24             # float32 unit roundoff
DELTA_FLOOR = 1e-5
DELTA_SAFETY = 2.0
DIR_MARGIN = 1e-6
EPS_COLOR = 2.5e-4
SHADOW_CAP = 64
SHADOW_CAP_MARGIN = 2
PRIMARY_CAP = 1024
PRIMARY_DECIDED_STEPS = 1000

FLAWS = ("face_order", "pixel_center", "dist_round", "alpha_hit", "no_shadow_cap", "emissive_shadows", "highlight_alpha",
         "display_across_ids")
# misreadings of the ray-batch entry and of the HDR arithmetic (both references take them; tests/test_rays_reference64.py)
RAY_FLAWS = ("rays_shared_medium", "rays_dist_from_first_origin", "rays_rng_linear", "rays_dir_length", "hdr_clamp_before_mean",
             "hdr_emission_x1", "hdr_deep_sky_no_sun")
E_EXP = 1.2e-7             # relative, det_expf on [-87, 0] (measured by tests/test_path_reference64.py)
GIVEN_DIR_ERR = 4.5 * U    # relative error of each component of a caller's direction after the float32 normalisation
BRANCH_MARGIN = 1e-5       # relative distance of a given component from the 1e-8 branch below which it is undecided
COLOUR_REL = 7.0 * U       # a product of at most six float32-rounded factors
HDR_MAX = 65504.0


def _f32(x):
    return float(np.float32(x))


PI = _f32(3.14159265359)
SKY = np.array([_f32(0.5), _f32(0.7), _f32(1.0)])
KIND_SKY, KIND_OPAQUE, KIND_EMISSIVE, KIND_TRANSLUCENT = 0, 1, 2, 3
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


class World:
    """The texel stream decoded into what octreeFind returns, in world coordinates."""

    def __init__(self, texels, tex_dim, world_min=(-1023, -1023, -1023), world_max=(1024, 1024, 1024), max_cells=1 << 26):
        b = np.ascontiguousarray(texels, np.uint8).ravel()
        self.T = np.frombuffer(b[: b.size // 4 * 4].tobytes(), "<u4").astype(np.int64)
        self.tex_dim = int(tex_dim)
        self.wmin = np.array(world_min, np.int64)
        self.wmax = np.array(world_max, np.int64)
        self._decode()
        self._paint(max_cells)

    def _fetch(self, idx):
        out = np.zeros(idx.shape, np.int64)
        ok = (idx >= 0) & (idx < self.T.size)
        out[ok] = self.T[idx[ok]]
        return out

    def _child(self, coord, mn, mx, ci_of):
        """one octreeFind iteration on internal nodes (comp:181-215) -> child box, exists, next coord, leaf flag"""
        nd = self._fetch(coord)
        mid = mn + (mx - mn) // 2                      # extents are >= 0: floor division is C's truncation
        ci = ci_of(mid)
        mask = nd >> 24
        exists = ((mask >> ci) & 1) == 1
        off = _POP8[mask & ((1 << ci) - 1)]
        ptr = self._fetch((nd & 0x7FFFFF) + off)
        hi = np.stack([(ci >> 2) & 1, (ci >> 1) & 1, ci & 1], 1) == 1
        return (np.where(hi, mid, mn), np.where(hi, mx, mid), exists, ptr & 0x7FFFFF, (ptr & 0x800000) != 0, ci)

    def _decode(self):
        """every node octreeFind can return, level by level: key (leaf texel >= 0, missing child -(parent*8+ci)-1), box,
        colour bytes, alpha byte, property bytes"""
        keys, mns, mxs, leafc = [], [], [], []
        coord = np.zeros(1, np.int64)
        mn, mx = self.wmin[None].copy(), self.wmax[None].copy()
        for depth in range(16):
            if not coord.size:
                break
            nxt = ([], [], [])
            for ci in range(8):
                cmn, cmx, exists, nc, leaf, _ = self._child(coord, mn, mx, lambda mid, ci=ci: np.full(mid.shape[0], ci))
                live = np.all(cmx > cmn, 1)
                m = live & ~exists
                keys.append(-(coord[m] * 8 + ci) - 1); mns.append(cmn[m]); mxs.append(cmx[m]); leafc.append(np.full(m.sum(), -1))
                lf = live & exists & leaf
                keys.append(nc[lf]); mns.append(cmn[lf]); mxs.append(cmx[lf]); leafc.append(nc[lf])
                it = live & exists & ~leaf
                nxt[0].append(nc[it]); nxt[1].append(cmn[it]); nxt[2].append(cmx[it])
            coord, mn, mx = (np.concatenate(a) for a in nxt)
            mn, mx = mn.reshape(-1, 3), mx.reshape(-1, 3)
        if coord.size:
            raise ValueError("octree deeper than octreeFind's 16 iterations")
        self.key = np.concatenate(keys)
        self.mn = np.concatenate(mns).reshape(-1, 3)
        self.mx = np.concatenate(mxs).reshape(-1, 3)
        lc = np.concatenate(leafc)
        isleaf = lc >= 0
        t0, t1 = self._fetch(np.where(isleaf, lc, -1)), self._fetch(np.where(isleaf, lc + 1, -1))
        self.rgb = np.stack([t0 & 255, (t0 >> 8) & 255, (t0 >> 16) & 255], 1)     # comp:173
        self.a = (t1 >> 24) & 255                                                  # comp:174
        self.p = np.stack([t1 & 255, (t1 >> 8) & 255, (t1 >> 16) & 255], 1)       # comp:177-178
        self.isleaf = isleaf
        order = np.argsort(self.key, kind="stable")
        self._order, self._sorted = order, self.key[order]
        # refraction as hitMarching sees it: p0*3 when a > 0 && p0 > 0, else "air"
        self.refractive = (self.a > 0) & (self.p[:, 0] > 0)
        self.refr = self.p[:, 0] / 255.0 * 3.0

    def _paint(self, max_cells):
        self.g0 = self.g1 = None
        lf = self.isleaf & (self.a > 0)
        if not lf.any():
            return
        g0 = np.maximum(self.mn[lf].min(0) - 1, self.wmin)
        g1 = np.minimum(self.mx[lf].max(0) + 1, self.wmax)
        if np.prod(g1 - g0) > max_cells:
            return
        grid = np.full(tuple(g1 - g0), -1, np.int32)
        lo = np.maximum(self.mn, g0) - g0
        hi = np.minimum(self.mx, g1) - g0
        sel = np.all(hi > lo, 1)
        unit = sel & np.all(hi - lo == 1, 1)
        u = np.nonzero(unit)[0]
        grid[lo[u, 0], lo[u, 1], lo[u, 2]] = u
        for i in np.nonzero(sel & ~unit)[0]:
            grid[lo[i, 0]:hi[i, 0], lo[i, 1]:hi[i, 1], lo[i, 2]:hi[i, 2]] = i
        if (grid < 0).any():
            raise AssertionError("the decoded nodes do not tile the painted box")
        self.g0, self.g1, self.grid = g0, g1, grid

    def descend(self, p):
        """octreeFind from the root for in-world points p[n, 3] -> node index"""
        p = np.asarray(p, np.int64).reshape(-1, 3)
        out = np.full(p.shape[0], -1, np.int64)
        idx = np.arange(p.shape[0])
        coord = np.zeros(p.shape[0], np.int64)
        mn = np.broadcast_to(self.wmin, p.shape).copy()
        mx = np.broadcast_to(self.wmax, p.shape).copy()
        for _ in range(16):
            if not idx.size:
                break
            q = p[idx]
            cmn, cmx, exists, nc, leaf, ci = self._child(coord, mn, mx, lambda mid: (q >= mid) @ np.array([4, 2, 1]))
            key = np.where(~exists, -(coord * 8 + ci) - 1, nc)
            done = ~exists | leaf
            out[idx[done]] = key[done]
            k = ~done
            idx, coord, mn, mx = idx[k], nc[k], cmn[k], cmx[k]
        if idx.size:
            raise ValueError("octree deeper than octreeFind's 16 iterations")
        pos = np.searchsorted(self._sorted, out)
        found = self._order[np.minimum(pos, self._sorted.size - 1)]
        assert np.array_equal(self.key[found], out)
        return found

    def find(self, p):
        """node index for in-world voxel coordinates p[n, 3]"""
        p = np.asarray(p, np.int64).reshape(-1, 3)
        out = np.empty(p.shape[0], np.int64)
        if self.g0 is None:
            return self.descend(p)
        ing = np.all((p >= self.g0) & (p < self.g1), 1)
        q = p[ing] - self.g0
        out[ing] = self.grid[q[:, 0], q[:, 1], q[:, 2]]
        if (~ing).any():
            out[~ing] = self.descend(p[~ing])
        return out

    def in_world(self, p):
        return np.all((p >= self.wmin) & (p < self.wmax), -1)


def _inv_dir(d):
    """comp:259-262"""
    with np.errstate(divide="ignore"):
        return np.where(np.abs(d) < 1e-8, 1e20, 1.0 / np.where(d == 0, 1.0, d))


def _step(world, pos, d, inv, node, push):
    """one node-to-node step of comp:278-307 / 357-372 -> (new position, axis, stuck, distance of each coordinate from
    its nearest grid plane, inf for the axis stepped)"""
    r = np.arange(pos.shape[0])
    plane = np.where(d > 0, world.mx[node], world.mn[node])
    tm = (plane - pos) * inv
    t = np.minimum(tm[:, 0], np.minimum(tm[:, 1], tm[:, 2]))
    ax = np.where(tm[:, 0] < tm[:, 1], np.where(tm[:, 0] < tm[:, 2], 0, 2), np.where(tm[:, 1] < tm[:, 2], 1, 2))
    new = pos + d * t[:, None]
    s = np.sign(d[r, ax])
    new[r, ax] += s * push
    with np.errstate(invalid="ignore"):
        fr = np.abs(new - np.rint(new))
    fr[r, ax] = np.inf
    return new, ax, (t == 0) & (s == 0), fr, t


def _step_error(new, t):
    """what one float32 step adds to the error of rayPos: t is off by ~3u relative (plane - pos, 1/d, the product), d*t
    and the sum round once each, and the float32 direction itself is off by up to ~6u relative"""
    with np.errstate(invalid="ignore", over="ignore"):
        return U * (10.0 * np.abs(t) + np.abs(new).max(1))


_SUBSETS = ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2))


def _floor_undecided(world, new, mp, node, near):
    """True where flooring `new` differently on a coordinate that lies within the margin of a grid plane (`near`) could
    change the node octreeFind returns (mp: the floor taken, node: its node, -1 outside the world)"""
    und = np.zeros(new.shape[0], bool)
    rows = np.nonzero(near.any(1))[0]
    if not rows.size:
        return und
    out = rows[node[rows] < 0]                                                   # outside: undecided only next to the world
    und[out] = np.all((mp[out] >= world.wmin - 1) & (mp[out] <= world.wmax), 1)
    for sub in _SUBSETS:
        q = rows[np.all(near[rows][:, list(sub)], 1) & (node[rows] >= 0)]
        if not q.size:
            continue
        alt = mp[q].copy()
        for j in sub:
            alt[:, j] += np.where(new[q, j] >= np.rint(new[q, j]), -1, 1)
        inw = world.in_world(alt)
        same = np.zeros(q.size, bool)
        same[inw] = world.find(alt[inw]) == node[q[inw]]
        und[q[~same]] = True
    return und


def ray_dirs(P, Vw, xs, ys, W, H, pixel_center=False):
    """comp:631-638: the float64 world direction of pixels (xs, ys) from the float32 camera block (P, Vw: row-major 4x4)"""
    off = 0.5 if pixel_center else 0.0
    u = (xs + off) / W * 2.0 - 1.0
    v = (ys + off) / H * 2.0 - 1.0
    clip = np.stack([u, v, -np.ones_like(u), np.ones_like(u)], 1)
    view = clip @ P.T
    w = view[:, 3:4]
    view = np.where(np.abs(w) > 1e-6, view / np.where(w == 0, 1.0, w), view)
    vd = view[:, :3] / np.linalg.norm(view[:, :3], axis=1, keepdims=True)
    wd = np.concatenate([vd, np.zeros_like(u)[:, None]], 1) @ Vw.T
    return wd[:, :3] / np.linalg.norm(wd[:, :3], axis=1, keepdims=True)


def not_in_shadow(w, pt, normal, err, L, flaws=(), dir_err=None):
    """notInShadow (comp:333-377) from hit points pt[n, 3] with axis normals normal[n, 3] (origin pt + normal*2e-3) and
    float32 position error bounds err[n] -> (lit bool[n], undecided bool[n]). L is the uniform lightDir (3,) or one
    direction per ray (n, 3) as the sun disc makes them (include/vrt.h, "Sun disc": the set-up of comp:335-345 computed
    from L'); then dir_err[n] bounds the absolute float32 error of each of its components: every step adds dir_err * t to
    the position error as path_ref64.march() does (and scales the step's own relative terms by |L'| where that exceeds
    1), and a ray with a non-zero component within max(DIR_MARGIN, 2 * dir_err) of 0 is undecided"""
    n = pt.shape[0]
    lit = np.ones(n, bool)
    amb = np.zeros(n, bool)
    if not n:
        return lit, amb
    pos = pt + normal * 2e-3
    err = np.asarray(err, np.float64).copy()
    d = np.broadcast_to(L, pos.shape).copy()
    inv = _inv_dir(d)
    mp = np.floor(pos).astype(np.int64)
    assert np.all(w.in_world(mp))
    near = np.abs(pos - np.rint(pos))[np.abs(normal) > 0] < 2.5e-4            # the offset origin, along the normal
    amb[near] = True
    if dir_err is not None:
        dir_err = np.broadcast_to(np.asarray(dir_err, np.float64), (n,))
        amb |= np.any((d != 0) & (np.abs(d) < np.maximum(DIR_MARGIN, 2.0 * dir_err)[:, None]), 1)
        dlen = np.maximum(1.0, np.sqrt((d * d).sum(1)))
    occluder = (w.a > 25) if "emissive_shadows" in flaws else ((w.a > 25) & (w.p[:, 1] == 0))   # comp:355
    cap = 1 << 16 if "no_shadow_cap" in flaws else SHADOW_CAP
    act = np.arange(n)
    node = w.find(mp)
    for k in range(1, cap + SHADOW_CAP_MARGIN + 1):                             # k: the octreeFind just made
        if not act.size:
            break
        occ = occluder[node]
        o = act[occ]
        lit[o] = k > cap
        amb[o] |= abs(k - (cap + 0.5)) < SHADOW_CAP_MARGIN
        act, node = act[~occ], node[~occ]
        new, ax, stuck, fr, t = _step(w, pos[act], d[act], inv[act], node, 1e-3)
        if dir_err is None:
            err[act] += _step_error(new, t)
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                err[act] += _step_error(new, t * dlen[act]) + dir_err[act] * np.abs(t)
        margin = DELTA_FLOOR + DELTA_SAFETY * err[act]
        with np.errstate(invalid="ignore"):
            m = np.floor(np.clip(new, -2.0 ** 40, 2.0 ** 40)).astype(np.int64)
        r = np.arange(act.size)
        ax_in = (m[r, ax] >= w.wmin[ax]) & (m[r, ax] < w.wmax[ax])
        go = w.in_world(m)                                                     # comp:374
        nn = np.full(act.size, -1, np.int64)
        nn[go] = w.find(m[go])
        if k <= cap:
            near = (ax_in & ~stuck)[:, None] & (fr < margin[:, None])
            amb[act] |= _floor_undecided(w, new, m, nn, near)
        pos[act], mp[act] = new, m
        act, node = act[go], nn[go]
    # rays still inside after cap + margin finds are lit by the cap (lit stays True)
    return lit, amb


def given_dirs(dirs):
    """pathTrace's normalisation of a caller's direction (comp:441 as include/vrt.h states it: d * (1 / sqrt(dot(d, d))),
    float32, every operation rounded once) -> (unit direction in float64 of the float32 input, |dir| as given).
    Exactly-zero components stay exactly zero (0 * x == 0) and keep their sign; every other component keeps its sign and
    has relative error <= GIVEN_DIR_ERR (see the module docstring)"""
    g = np.array(dirs, np.float32).astype(np.float64).reshape(-1, 3)
    length = np.sqrt((g * g).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return g / length[:, None], length


def batch_pixels(n, width, flaws=()):
    """the RNG pixel of ray i of a batch read as an image `width` wide: (i % width, i // width)"""
    i = np.arange(n, dtype=np.int64)
    if "rays_rng_linear" in flaws:
        return i, np.zeros(n, np.int64)
    return i % int(width), i // int(width)


def dir_undecided(d, given):
    """a component float32 may put on the other side of a rule of hitMarching: for a frame's ray 0 < |d| < DIR_MARGIN (its
    error is absolute, ~6u); for a given direction the error is relative, so zero-ness, sign and the 1e-8 branch are the
    float32 run's unless |d| is within BRANCH_MARGIN (relative) of 1e-8"""
    a = np.abs(d)
    if given:
        return np.any(np.abs(a - 1e-8) <= BRANCH_MARGIN * 1e-8, 1) | ~np.isfinite(d).all(1)
    return np.any((d != 0) & (a < DIR_MARGIN), 1)


class _Start:
    pass


def ray_start(w, org, scale, flaws=(), err3=None):
    """comp:443-462 per ray from world-space origins org[n, 3] (float32 values): gro = float32(origin * voxelScale), its
    rounding as the position bound (zero when the product is exact), the voxel at floor(gro) as the start medium
    (startIOF, colour, density a * 5). Origins outside the world are reported in .outside and nothing else is said
    about them (octreeFind's early return leaves the node box undefined there, comp:143). err3[n, 3]: what the float32
    run's gro may differ by on top of that rounding, in grid units (a computed origin: tests/lens_ref64.py)
    -> .gro .err[n, 3] .outside .amb .start (node, -1 outside) .node (the medium's node) .iof .mc[n, 3] .md"""
    st = _Start()
    n = org.shape[0]
    exact = org * scale
    with np.errstate(invalid="ignore", over="ignore"):
        st.gro = exact.astype(np.float32).astype(np.float64)
        st.err = np.abs(st.gro - exact)
        if err3 is not None:
            st.err = st.err + err3
        mp = np.floor(np.clip(st.gro, -2.0 ** 40, 2.0 ** 40)).astype(np.int64)
    st.outside = ~w.in_world(mp) | ~np.isfinite(st.gro).all(1)
    ins = np.nonzero(~st.outside)[0]
    st.start = np.full(n, -1, np.int64)
    st.start[ins] = w.find(mp[ins])
    st.amb = np.zeros(n, bool)
    g = st.gro[ins]
    near = (g != np.rint(g)) & (np.abs(g - np.rint(g)) < DELTA_FLOOR + DELTA_SAFETY * st.err[ins].max(1)[:, None])
    st.amb[ins] = _floor_undecided(w, g, mp[ins], st.start[ins], near)
    e = np.maximum(st.start, 0)
    if "rays_shared_medium" in flaws:
        e = np.full(n, e[0])
    st.node = e
    p0 = w.p[e, 0] / 255.0 * 3.0
    st.iof = np.where((p0 > 0.0) & (p0 < 3.0), p0, 1.0)                       # comp:448-449
    st.mc = np.where((w.a[e] > 0)[:, None], w.rgb[e] / 255.0, 1.0)             # comp:460
    st.md = w.a[e] / 255.0 * 5.0                                              # comp:461
    return st


def absorb(md, dim, edim, mc):
    """exp(-density * distanceInMedium * (1 - mediumColor)) (comp:512-516) -> (factor[k, 3], relative error bound[k]):
    the exponent's three products and the float32 distance (|arg| * 5u), the distance's own error, det_expf"""
    arg = -md[:, None] * dim[:, None] * (1.0 - mc)
    e = np.abs(arg) * 5 * U + md[:, None] * (1.0 - mc) * edim[:, None] + E_EXP
    return np.exp(arg), e.max(1)


def colour_bound(c, rel, extra=0.0):
    """what a float32 run may differ from the float64 colour c by: rel * |c| + extra, plus EPS_COLOR / 255 (the margin the
    byte test has always kept around a .5 tie, in colour units); rel < 0 marks a colour that is exact in float32 (bound 0:
    the byte is rint's ties-to-even). frame()'s tie test and radiance() both use it."""
    rel = np.asarray(rel)
    return np.where((rel < 0)[:, None], 0.0, rel[:, None] * np.abs(c) + extra + EPS_COLOR / 255.0)


def hdr_value(c):
    """h(c) of vrt_accum_keep_hdr point 1 (include/vrt.h): clamp to [0, 65504]. 1-Lipschitz: |h(a) - h(b)| <= |a - b|, so a
    value within its bound of either end is compared after clamping both sides with the same bound."""
    return np.clip(c, 0.0, HDR_MAX)


def hdr_mean(values, bounds, decided, flaws=()):
    """vrt.h points 2-3 over samples: values / bounds float64[k][n, 3], decided bool[k][n] -> (mean, bound, decided).
    The mean of h(c_k); its bound is the mean of the samples' bounds plus u * |mean| for the final cast to float (the
    float64 sums' own error, <= k * 2^-53 relative, is far below that and is not carried). A ray's mean is decided only
    when every one of its samples is."""
    v = [np.minimum(x, 1.0) for x in values] if "hdr_clamp_before_mean" in flaws else values
    k = len(v)
    mean = sum(hdr_value(x) for x in v) / k
    return mean, sum(bounds) / k + U * np.abs(mean), np.all(decided, axis=0)


def tonemap(mean, bound, op, exposure):
    """vrt.h point 4 on a float64 mean with its bound -> (bytes int64[n, 3], byte decided[n, 3], y, y's bound).
    clamp: y = e * x, bound e * b (exact in float32 for a power-of-two exposure; u * |y| more for any other).
    reinhard: x' = e * x, y = x' / (1 + x'): 1-Lipschitz in x' for x' >= 0, plus 3u of its value (the product, the sum and
    the quotient round once each). A byte is decided when unorm8's x = clamp(y, 0, 1) * 255 is further than 255 * bound
    from a .5 tie (the bound already holds EPS_COLOR / 255)."""
    e = float(np.float32(exposure))
    x = e * mean
    b = e * bound
    if np.frexp(e)[0] != 0.5:
        b = b + U * np.abs(x)
    if op == "reinhard":
        y = x / (1.0 + x)
        b = b + 3 * U * np.abs(y)
    else:
        assert op == "clamp", op
        y = x
    t = np.clip(y, 0.0, 1.0) * 255.0
    return np.rint(t).astype(np.int64), np.abs(t - np.floor(t) - 0.5) >= 255.0 * b, y, b


class Trace:
    """The first hit of every requested pixel (and its shadow ray), from which frame(mode) assembles the outputs."""

    def __init__(self, world, inv_proj, inv_view, cam_pos, width, height, xs=None, ys=None, voxel_scale=1.0,
                 global_light=(1.0, 1.0, 1.0, 1.0), light_dir=None, highlighted=(-1, -1, -1), flaws=()):
        """a frame: one origin (cameraPos), ray_dirs' directions, the frame's width"""
        self._uniforms(world, voxel_scale, global_light, light_dir, highlighted, flaws)
        self.W, self.H = int(width), int(height)
        if xs is None:
            ys, xs = np.mgrid[0:self.H, 0:self.W]
        self.xs, self.ys = np.asarray(xs, np.int64).ravel(), np.asarray(ys, np.int64).ravel()
        self.cam = np.array(cam_pos, np.float32).astype(np.float64)[:3]
        d = ray_dirs(np.array(inv_proj, np.float32).astype(np.float64).reshape(4, 4).T,
                     np.array(inv_view, np.float32).astype(np.float64).reshape(4, 4).T,
                     self.xs, self.ys, self.W, self.H, "pixel_center" in self.flaws)
        self._trace(self.cam, d, np.ones(d.shape[0]), given=False)
        if self.outside.any():
            raise ValueError("eye outside the world: octreeFind's early return leaves the node box undefined (comp:143)")

    @classmethod
    def rays(cls, world, origins, dirs, width, sample=0, voxel_scale=1.0, global_light=(1.0, 1.0, 1.0, 1.0), light_dir=None,
             highlighted=(-1, -1, -1), flaws=()):
        """a ray batch (include/vrt.h, "Rays", "Direction", "width"): origins float32 (n, 3) or (3,) shared, in world units;
        dirs float32 (n, 3) as given, any length; ray i is pixel (i % width, i // width) of an image of that width for the
        random numbers (modes 0 and 1 draw none, so `sample` changes nothing here)"""
        self = cls.__new__(cls)
        self._uniforms(world, voxel_scale, global_light, light_dir, highlighted, flaws)
        d, length = given_dirs(dirs)
        self.W = int(width)
        self.xs, self.ys = batch_pixels(d.shape[0], self.W, self.flaws)
        self.H = int(self.ys.max()) + 1 if d.shape[0] else 0
        self._trace(np.array(origins, np.float32).astype(np.float64), d, length, given=True)
        return self

    def _uniforms(self, world, voxel_scale, global_light, light_dir, highlighted, flaws):
        assert light_dir is not None, "lightDir is a uniform: pass the host's float32 value"
        unknown = set(flaws) - set(FLAWS) - set(RAY_FLAWS)
        assert not unknown, unknown
        self.w, self.flaws = world, frozenset(flaws)
        self.scale = float(np.float32(voxel_scale))
        self.gl = np.array(global_light, np.float32).astype(np.float64)
        self.L = np.array(light_dir, np.float32).astype(np.float64)
        self.hl = np.array(highlighted, np.int64)

    @classmethod
    def lens(cls, world, rays, voxel_scale=1.0, global_light=(1.0, 1.0, 1.0, 1.0), light_dir=None, highlighted=(-1, -1, -1),
             flaws=()):
        """a jittered and / or thin-lens sample of the accumulation (include/vrt.h VRT_ACCUM_JITTER, vrt_set_lens): `rays` is
        tests/lens_ref64.py's lens_rays(camera block, W, H, xs, ys, sample, jitter, aperture, focus) -- per-ray float64
        origins and unit directions with the bounds of their float32 counterparts (modes 0 and 1 draw no random number)"""
        self = cls.__new__(cls)
        self._uniforms(world, voxel_scale, global_light, light_dir, highlighted, flaws)
        self.W, self.H, self.xs, self.ys = rays.W, rays.H, rays.xs, rays.ys
        self._trace(rays.o, rays.d, np.ones(rays.d.shape[0]), given=False, err3=rays.err_o * abs(self.scale) + U * np.abs(rays.o * self.scale),
                    dir_err=rays.dir_err, medium_org=rays.medium_org, measure_org=rays.measure_org)
        self.amb |= rays.amb
        return self

    def _trace(self, origins, d, length, given, err3=None, dir_err=None, medium_org=None, measure_org=None):
        """the entry the constructors share: world-space origins (3,) or (n, 3), unit directions d[n, 3] in float64,
        length[n]: |dir| as given (1 for a frame); given: the directions are a caller's (see given_dirs). Optional, for
        computed rays: err3[n, 3] the origin's bound in grid units on top of ray_start's rounding, dir_err[n] the absolute
        bound of each direction component (it replaces nothing: the step error's own ~6u stays), medium_org / measure_org
        world-space origins the start medium is looked up at / dist and distanceInMedium are measured from instead of the
        ray's own (planted misreadings only)"""
        n = d.shape[0]
        self.d = d
        self.org = np.broadcast_to(origins.reshape(-1, 3), (n, 3)).copy()
        self.tlen = length if "rays_dir_length" in self.flaws else np.ones(n)
        self.amb = dir_undecided(d, given)
        self._err3, self._dir_err, self._medium_org, self._measure_org = err3, dir_err, medium_org, measure_org
        if dir_err is not None:
            self.amb |= np.any((d != 0) & (np.abs(d) < 2.0 * np.asarray(dir_err)[:, None]), 1)
        self._primary()
        self._shadow()

    def _primary(self):
        """pathTrace's first hitMarching (comp:443-478) for every ray"""
        w, n = self.w, self.d.shape[0]
        st = ray_start(w, self.org, self.scale, self.flaws, self._err3)
        if self._medium_org is not None:
            m = ray_start(w, np.broadcast_to(self._medium_org, self.org.shape), self.scale)
            st.node, st.iof, st.mc, st.md = m.node, m.iof, m.mc, m.md
        self.outside, self.gro, self.err0 = st.outside, st.gro, st.err.max(1)
        self.dim_gro = self.gro
        if self._measure_org is not None:
            self.org = np.broadcast_to(self._measure_org, self.org.shape).copy()
            self.dim_gro = self.org * self.scale
        self.err = self.err0.copy()                                            # float32 error bound of rayPos so far
        self.amb |= st.amb
        self.eye_node, self.iof, self.in_medium, self.mc, self.md = st.node, st.iof, st.md > 0, st.mc, st.md
        pos = self.gro.copy()
        inv = _inv_dir(self.d)
        cur = np.maximum(st.start, 0)
        self.hit = np.zeros(n, bool)
        self.mp = np.zeros((n, 3), np.int64)
        self.pt = np.zeros((n, 3))
        self.ax = np.zeros(n, np.int64)
        self.hv = np.zeros(n, np.int64)
        self.lv = np.zeros(n, np.int64)
        self.steps = np.zeros(n, np.int64)
        act = np.nonzero(~self.outside)[0]
        for it in range(PRIMARY_CAP):
            if not act.size:
                break
            new, ax, stuck, fr, t = _step(w, pos[act], self.d[act], inv[act], cur[act], 1e-4)
            self.err[act] += _step_error(new, t)
            if self._dir_err is not None:
                with np.errstate(invalid="ignore", over="ignore"):
                    self.err[act] += self._dir_err[act] * np.abs(t)
            with np.errstate(invalid="ignore"):
                mp = np.floor(np.clip(new, -2.0 ** 40, 2.0 ** 40)).astype(np.int64)
            r = np.arange(act.size)
            ax_in = (mp[r, ax] >= w.wmin[ax]) & (mp[r, ax] < w.wmax[ax])
            go = w.in_world(mp) & ~stuck                                       # comp:310
            node = np.full(act.size, -1, np.int64)
            node[go] = w.find(mp[go])                                          # comp:315
            near = (ax_in & ~stuck)[:, None] & (fr < (DELTA_FLOOR + DELTA_SAFETY * self.err[act])[:, None])
            self.amb[act] |= _floor_undecided(w, new, mp, node, near)
            self.steps[act] = it + 1
            act, new, ax, mp, nxt = act[go], new[go], ax[go], mp[go], node[go]
            prev = cur[act]
            if "alpha_hit" in self.flaws:
                hit = (w.a[nxt] > 0) & (w.a[prev] == 0)
            else:
                pr = np.where(w.refractive[prev], w.refr[prev], self.iof[act])  # comp:318-321
                cr = np.where(w.refractive[nxt], w.refr[nxt], 1.0)
                hit = np.abs(cr - pr) > 1e-4
            h = act[hit]
            self.hit[h] = True
            self.mp[h], self.pt[h], self.ax[h] = mp[hit], new[hit], ax[hit]
            self.hv[h], self.lv[h] = nxt[hit], prev[hit]
            pos[act], cur[act] = new, nxt
            act = act[~hit]
        self.amb[act] = True                                                   # capped while still moving
        self.amb |= self.steps > PRIMARY_DECIDED_STEPS

    def _surface(self):
        w, i = self.w, np.nonzero(self.hit)[0]
        hv, lv = self.hv[i], self.lv[i]
        hva = w.a[hv] > 0
        rgb = np.where(hva[:, None], w.rgb[hv], w.rgb[lv]) / 255.0            # comp:506
        a = np.where(hva, w.a[hv], w.a[lv]) / 255.0
        hl = np.all(self.mp[i] == self.hl, 1)                                  # comp:518-520
        rgb[hl] = 1.0 - rgb[hl]
        if "highlight_alpha" not in self.flaws:
            a[hl] = 1.0
        emission = np.where(hva, w.p[hv, 1] / 255.0, 0.0) * (1.0 if "hdr_emission_x1" in self.flaws else 10.0)   # comp:503, 575
        s = -np.sign(self.d[i, self.ax[i]])                                    # comp:293-294
        normal = np.zeros((i.size, 3))
        normal[np.arange(i.size), self.ax[i]] = s
        nonzero = s != 0
        normal[~nonzero] = (0.0, 1.0, 0.0)                                     # comp:497
        flip = np.einsum("ij,ij->i", self.d[i], normal) > 0                    # comp:522-526
        normal[flip] = -normal[flip]
        ndotl = np.maximum(normal @ self.L, 0.0)                               # comp:537
        return i, rgb, a, emission, normal, ndotl, np.where(nonzero, self.ax[i], -1), s

    def _shadow(self):
        """notInShadow (comp:333-377) from every opaque, non-emissive first hit"""
        n = self.d.shape[0]
        self.lit = np.ones(n, bool)
        self.shadow_amb = np.zeros(n, bool)
        i, rgb, a, emission, normal, ndotl, _, _ = self._surface()
        need = (a >= 1.0) & (emission <= 0.0)
        i, normal = i[need], normal[need]
        self.lit[i], self.shadow_amb[i] = not_in_shadow(self.w, self.pt[i], normal, self.err[i], self.L, self.flaws)

    def _colour(self, mode):
        """-> (c float64[n, 3], rel[n] relative error bound, open[n]: colour not restated, hits i, surface tuple)"""
        n = self.d.shape[0]
        c = np.zeros((n, 3))
        rel = np.full(n, COLOUR_REL)
        colour_open = np.zeros(n, bool)
        tc = self.gl[:3]
        c[~self.hit] = self.gl[:3] * SKY * tc                                 # comp:489
        # the float32 products of comp:489 may be exact (a white globalLight): then the sky is the float32 run's, bound 0
        f32 = (self.gl[:3].astype(np.float32) * SKY.astype(np.float32)) * tc.astype(np.float32)
        if np.all(f32.astype(np.float64) == self.gl[:3] * SKY * tc):
            rel[~self.hit] = -1.0
        sf = self._surface()
        i, rgb, a, emission, normal, ndotl, ax, s = sf
        opaque = a >= 1.0
        em = opaque & (emission > 0)
        tr = ~opaque
        op = opaque & ~em
        # the start medium's absorption (comp:501, 512-516): length(hitPoint / voxelScale - origin) / voxelScale with the
        # grid-space origin, as the GLSL has it
        tci = np.tile(tc, (i.size, 1))
        hpw = self.pt[i] / self.scale
        ln = np.linalg.norm(hpw - self.dim_gro[i], axis=1) * self.tlen[i]
        dim = ln / self.scale
        edim = (self.err[i] + self.err0[i] + 4 * U * (np.abs(hpw).max(1) + np.abs(self.gro[i]).max(1) + ln)) / self.scale
        md = self.md[i]
        colour_open[i] |= (md > 0) & (np.abs(dim - 1e-6) <= edim)
        ab = (dim > 1e-6) & (md > 0.0)
        if ab.any():
            f, e = absorb(md[ab], dim[ab], edim[ab], self.mc[i[ab]])
            tci[ab] *= f
            rel[i[ab]] += e + U
        cc = np.zeros((i.size, 3))
        cc[tr] = tci[tr] * rgb[tr] * (self.gl[:3] * ndotl[tr, None])           # comp:548-552
        cc[em] = tci[em] * rgb[em] * emission[em, None]                        # comp:576-577
        lit = self.lit[i] if mode == 1 else np.ones(i.size, bool)
        cc[op] = self.gl[:3] * (lit[op] * ndotl[op])[:, None] * rgb[op] * tci[op] / PI   # comp:587-588
        c[i] = cc
        if mode == 1:
            colour_open[i[op]] |= self.shadow_amb[i[op]]
        if mode == 2:                                                          # bounce and glass stack: not restated
            colour_open[i[op | tr]] = True
        return c, rel, colour_open, sf, (em, tr, op)

    def frame(self, mode):
        """-> Frame for VRT_MODE_PRIMARY (0), VRT_MODE_PRIMARY_SHADOW (1) or VRT_MODE_FULL (2)"""
        w, n = self.w, self.d.shape[0]
        f = Frame(self.xs, self.ys, mode)
        f.id = np.zeros(n, np.int64)
        f.dist = np.full(n, int(w.wmax[0] - w.wmin[0]), np.int64)            # comp:441
        f.kind = np.full(n, KIND_SKY, np.int64)
        f.hit = self.hit.copy()
        f.outside = self.outside.copy()
        und_dist = np.zeros(n, bool)
        c, rel, colour_open, (i, rgb, a, emission, normal, ndotl, ax, s), (em, tr, op) = self._colour(mode)
        opaque = a >= 1.0
        idset = opaque                                                         # comp:539
        j = i[idset]
        lin = self.mp[j, 0] + w.tex_dim * (self.mp[j, 1] + w.tex_dim * self.mp[j, 2])
        face = self._face(ax[idset], s[idset])
        f.id[j] = ((lin * 6 + face + (1 << 31)) % (1 << 32)) - (1 << 31)     # int arithmetic wraps in GLSL
        eye = self.org[0] if "rays_dist_from_first_origin" in self.flaws else self.org[j]
        ln = np.linalg.norm(self.pt[j] / self.scale - eye, axis=1) * self.tlen[j]   # comp:498, 543
        f.dist[j] = np.rint(ln) if "dist_round" in self.flaws else np.trunc(ln)
        margin = (DELTA_FLOOR + DELTA_SAFETY * self.err[j]) / self.scale + 4 * U * ln
        und_dist[j] = np.abs(ln - np.rint(ln)) < margin
        f.kind[i[em]], f.kind[i[tr]], f.kind[i[op]] = KIND_EMISSIVE, KIND_TRANSLUCENT, KIND_OPAQUE
        cl = np.clip(c, 0.0, 1.0)
        x = cl * 255.0
        f.rgba = np.concatenate([np.rint(x), np.full((n, 1), 255.0)], 1).astype(np.int64)
        tie = np.abs(x - np.floor(x) - 0.5) < 255.0 * colour_bound(cl, rel)
        f.dec_id = ~self.amb & ~self.outside
        if mode == 2:                                                          # a glass first hit leaves the id to the stack
            f.dec_id[i[tr]] = False
        f.dec_dist = f.dec_id & ~und_dist
        f.dec_rgb = (~self.amb & ~self.outside & ~colour_open)[:, None] & ~tie
        return f

    def radiance(self, mode):
        """the unclamped colour of mode 0 or 1 -> (h(c) float64[n, 3], bound[n, 3], decided[n]): a float32 run's h(c) lies
        within bound of it wherever decided (frame()'s tie test uses the same bound on the clamped colour)"""
        assert mode in (0, 1)
        c, rel, colour_open, _, _ = self._colour(mode)
        return hdr_value(c), colour_bound(c, rel), ~self.amb & ~self.outside & ~colour_open

    def _face(self, ax, s):
        """getFaceIndex (comp:419-433) of an axis normal with sign s (ax -1: the zero normal)"""
        face = np.where(ax == 0, np.where(s > 0, 0, 1), np.where(ax == 1, np.where(s > 0, 2, 3), np.where(s > 0, 4, 5)))
        if "face_order" in self.flaws:
            face = face ^ 1
        return np.where(ax < 0, 0, face)


class Frame:
    """Outputs of one mode at the traced pixels, with what is decided."""

    def __init__(self, xs, ys, mode):
        self.xs, self.ys, self.mode = xs, ys, mode

    def hit_undecided_share(self):
        """of the hit pixels (in mode 2 those whose first hit is not glass: the stack is not restated)"""
        full = self.dec_id & self.dec_dist
        scope = self.hit.copy()
        if self.mode != 2:
            full = full & self.dec_rgb.all(1)
        else:
            scope &= self.kind != KIND_TRANSLUCENT
        return float((~full[scope]).mean()) if scope.any() else 0.0

    def all_decided(self):
        return self.dec_id & self.dec_dist & self.dec_rgb.all(1)

    def in_world_undecided_share(self):
        """of a batch's rays whose origin is inside the world: not every field decided (outside origins are neither)"""
        inw = ~self.outside
        return float((~self.all_decided()[inw]).mean()) if inw.any() else 0.0


def compare(ref, rgba, idd):
    """ref (Frame) against images rgba8[H, W, 4] / id_dist[H, W, 2] at ref's pixels, on decided fields only.
    -> dict: checked / mismatch counts per field, decided hit pixels, undecided share of hit pixels, first mismatch"""
    rgba, idd = np.asarray(rgba), np.asarray(idd)
    if rgba.ndim == 2:                                                         # a ray batch: one row per ray
        got_rgba, got = rgba.astype(np.int64), idd.astype(np.int64)
    else:
        got_rgba, got = rgba[ref.ys, ref.xs].astype(np.int64), idd[ref.ys, ref.xs].astype(np.int64)
    bad_id = ref.dec_id & (got[:, 0] != ref.id)
    bad_dist = ref.dec_dist & (got[:, 1] != ref.dist)
    bad_rgb = ref.dec_rgb & (got_rgba[:, :3] != ref.rgba[:, :3])
    bad_a = ref.dec_rgb.any(1) & (got_rgba[:, 3] != 255)
    bad = bad_id | bad_dist | bad_rgb.any(1) | bad_a
    out = {"checked_id": int(ref.dec_id.sum()), "checked_dist": int(ref.dec_dist.sum()),
           "checked_rgb": int(ref.dec_rgb.sum()), "bad_id": int(bad_id.sum()), "bad_dist": int(bad_dist.sum()),
           "bad_rgb": int(bad_rgb.any(1).sum() + bad_a.sum()), "bad": int(bad.sum()),
           "decided_hits": int((ref.hit & ref.dec_id & ref.dec_dist).sum()),
           "undecided_share": ref.hit_undecided_share(), "first": None}
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        out["first"] = {"x": int(ref.xs[k]), "y": int(ref.ys[k]), "got_id_dist": got[k].tolist(), "want_id_dist": [int(ref.id[k]), int(ref.dist[k])],
                        "got_rgba": got_rgba[k].tolist(), "want_rgba": ref.rgba[k].tolist(), "kind": int(ref.kind[k])}
    return out


def display(rgba, idd, xs, ys, flaws=()):
    """quad.frag (82 lines) at pixels (xs, ys) of the frame rgba8[H, W, 4] / id_dist[H, W, 2]
    -> (rgba8[n, 4] int64, decided[n, 3] bool)"""
    rgba = np.asarray(rgba).astype(np.int64)
    idd = np.asarray(idd).astype(np.int64)
    H, W = rgba.shape[:2]
    xs, ys = np.asarray(xs, np.int64).ravel(), np.asarray(ys, np.int64).ravel()
    cid, cd = idd[ys, xs, 0], idd[ys, xs, 1]
    r64 = 200.0 / np.sqrt(np.maximum(1, cd).astype(np.float64))
    R = np.clip(np.trunc(r64), 1, 20).astype(np.int64)                        # quad.frag:44-47
    k = np.rint(r64)
    radius_tie = (np.abs(r64 - k) < 1e-5) & (k * k * np.maximum(1, cd) != 40000)
    s = np.zeros((xs.size, 3), np.int64)
    cnt = np.zeros(xs.size, np.int64)
    across = "display_across_ids" in flaws
    for dy in range(-20, 21):
        for dx in range(-20, 21):
            nx, ny = xs + dx, ys + dy
            ok = (np.abs(dy) <= R) & (np.abs(dx) <= R) & (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)   # :59-62
            q = np.nonzero(ok)[0]
            same = idd[ny[q], nx[q], 0] == cid[q]
            if not across:
                q = q[same]                                                    # :68
            s[q] += rgba[ny[q], nx[q], :3]
            cnt[q] += 1
    x = s / np.maximum(cnt, 1)[:, None]                                        # mean of byte/255, times 255
    out = np.concatenate([np.rint(np.clip(x, 0, 255)), np.full((xs.size, 1), 255)], 1).astype(np.int64)
    eps = EPS_COLOR + 1.52e-5 * (cnt + 2)
    dec = (np.abs(x - np.floor(x) - 0.5) >= eps[:, None]) & ~radius_tie[:, None]
    sky = cid == 0                                                             # :35-38
    out[sky] = rgba[ys[sky], xs[sky]]
    dec[sky] = True
    return out, dec
