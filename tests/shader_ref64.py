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

flaws= plants one plausible misreading at a time, so the tests can show that the comparison catches it."""
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


def not_in_shadow(w, pt, normal, err, L, flaws=()):
    """notInShadow (comp:333-377) from hit points pt[n, 3] with axis normals normal[n, 3] (origin pt + normal*2e-3) and
    float32 position error bounds err[n] -> (lit bool[n], undecided bool[n])"""
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
        err[act] += _step_error(new, t)
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


class Trace:
    """The first hit of every requested pixel (and its shadow ray), from which frame(mode) assembles the outputs."""

    def __init__(self, world, inv_proj, inv_view, cam_pos, width, height, xs=None, ys=None, voxel_scale=1.0,
                 global_light=(1.0, 1.0, 1.0, 1.0), light_dir=None, highlighted=(-1, -1, -1), flaws=()):
        assert light_dir is not None, "lightDir is a uniform: pass the host's float32 value"
        unknown = set(flaws) - set(FLAWS)
        assert not unknown, unknown
        self.w, self.flaws = world, frozenset(flaws)
        self.W, self.H = int(width), int(height)
        if xs is None:
            ys, xs = np.mgrid[0:self.H, 0:self.W]
        self.xs, self.ys = np.asarray(xs, np.int64).ravel(), np.asarray(ys, np.int64).ravel()
        self.scale = float(np.float32(voxel_scale))
        self.gl = np.array(global_light, np.float32).astype(np.float64)
        self.L = np.array(light_dir, np.float32).astype(np.float64)
        self.hl = np.array(highlighted, np.int64)
        self.cam = np.array(cam_pos, np.float32).astype(np.float64)[:3]
        self._rays(np.array(inv_proj, np.float32).astype(np.float64).reshape(4, 4).T,
                   np.array(inv_view, np.float32).astype(np.float64).reshape(4, 4).T)
        self._primary()
        self._shadow()

    def _rays(self, P, Vw):
        self.d = ray_dirs(P, Vw, self.xs, self.ys, self.W, self.H, "pixel_center" in self.flaws)
        self.amb = np.any((self.d != 0) & (np.abs(self.d) < DIR_MARGIN), 1)

    def _primary(self):
        """pathTrace's first hitMarching (comp:443-478) for every ray"""
        w, n = self.w, self.d.shape[0]
        eye = self.cam * self.scale
        emp = np.floor(eye).astype(np.int64)
        if not w.in_world(emp):
            raise ValueError("eye outside the world: octreeFind's early return leaves the node box undefined (comp:143)")
        e = int(w.find(emp[None])[0])
        self.err = np.full(n, U * np.abs(eye).max())                          # float32 error bound of rayPos so far
        near = (eye != np.rint(eye)) & (np.abs(eye - np.rint(eye)) < DELTA_FLOOR + DELTA_SAFETY * self.err[0])
        if _floor_undecided(w, eye[None], emp[None], np.array([e]), near[None])[0]:
            self.amb[:] = True
        self.eye_node = e
        p0 = w.p[e, 0] / 255.0 * 3.0
        self.iof = p0 if 0.0 < p0 < 3.0 else 1.0                              # comp:448-449
        self.in_medium = w.a[e] > 0                                            # comp:460-461: mediumDensity = a*5
        pos = np.tile(eye, (n, 1))
        inv = _inv_dir(self.d)
        cur = np.full(n, e, np.int64)
        self.hit = np.zeros(n, bool)
        self.mp = np.zeros((n, 3), np.int64)
        self.pt = np.zeros((n, 3))
        self.ax = np.zeros(n, np.int64)
        self.hv = np.zeros(n, np.int64)
        self.lv = np.zeros(n, np.int64)
        self.steps = np.zeros(n, np.int64)
        act = np.arange(n)
        for it in range(PRIMARY_CAP):
            if not act.size:
                break
            new, ax, stuck, fr, t = _step(w, pos[act], self.d[act], inv[act], cur[act], 1e-4)
            self.err[act] += _step_error(new, t)
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
                pr = np.where(w.refractive[prev], w.refr[prev], self.iof)      # comp:318-321
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
        emission = np.where(hva, w.p[hv, 1] / 255.0, 0.0) * 10.0               # comp:503, 575
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

    def frame(self, mode):
        """-> Frame for VRT_MODE_PRIMARY (0), VRT_MODE_PRIMARY_SHADOW (1) or VRT_MODE_FULL (2)"""
        w, n = self.w, self.d.shape[0]
        f = Frame(self.xs, self.ys, mode)
        f.id = np.zeros(n, np.int64)
        f.dist = np.full(n, int(w.wmax[0] - w.wmin[0]), np.int64)            # comp:441
        c = np.zeros((n, 3))
        f.kind = np.full(n, KIND_SKY, np.int64)
        f.hit = self.hit.copy()
        tc = self.gl[:3]
        c[~self.hit] = self.gl[:3] * SKY * tc                                 # comp:489
        und_dist = np.zeros(n, bool)
        colour_open = np.zeros(n, bool)
        i, rgb, a, emission, normal, ndotl, ax, s = self._surface()
        opaque = a >= 1.0
        idset = opaque                                                         # comp:539
        j = i[idset]
        lin = self.mp[j, 0] + w.tex_dim * (self.mp[j, 1] + w.tex_dim * self.mp[j, 2])
        face = self._face(ax[idset], s[idset])
        f.id[j] = ((lin * 6 + face + (1 << 31)) % (1 << 32)) - (1 << 31)     # int arithmetic wraps in GLSL
        ln = np.linalg.norm(self.pt[j] / self.scale - self.cam, axis=1)        # comp:498, 543
        f.dist[j] = np.rint(ln) if "dist_round" in self.flaws else np.trunc(ln)
        margin = (DELTA_FLOOR + DELTA_SAFETY * self.err[j]) / self.scale + 4 * U * ln
        und_dist[j] = np.abs(ln - np.rint(ln)) < margin
        em = opaque & (emission > 0)
        tr = ~opaque
        op = opaque & ~em
        f.kind[i[em]], f.kind[i[tr]], f.kind[i[op]] = KIND_EMISSIVE, KIND_TRANSLUCENT, KIND_OPAQUE
        cc = np.zeros((i.size, 3))
        cc[tr] = tc * rgb[tr] * (self.gl[:3] * ndotl[tr, None])                # comp:548-552
        cc[em] = tc * rgb[em] * emission[em, None]                             # comp:576-577
        lit = self.lit[i] if mode == 1 else np.ones(i.size, bool)
        cc[op] = self.gl[:3] * (lit[op] * ndotl[op])[:, None] * rgb[op] * tc / PI   # comp:587-588
        c[i] = cc
        if self.in_medium:                                                     # absorption (comp:512-516) is not restated
            colour_open[i] = True
        if mode == 1:
            colour_open[i[op]] |= self.shadow_amb[i[op]]
        if mode == 2:                                                          # bounce and glass stack: not restated
            colour_open[i[op | tr]] = True
        x = np.clip(c, 0.0, 1.0) * 255.0
        f.rgba = np.concatenate([np.rint(x), np.full((n, 1), 255.0)], 1).astype(np.int64)
        tie = np.abs(x - np.floor(x) - 0.5) < EPS_COLOR
        f.dec_id = ~self.amb.copy()
        if mode == 2:                                                          # a glass first hit leaves the id to the stack
            f.dec_id[i[tr]] = False
        f.dec_dist = f.dec_id & ~und_dist
        f.dec_rgb = (~self.amb & ~colour_open)[:, None] & ~tie
        return f

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


def compare(ref, rgba, idd):
    """ref (Frame) against images rgba8[H, W, 4] / id_dist[H, W, 2] at ref's pixels, on decided fields only.
    -> dict: checked / mismatch counts per field, decided hit pixels, undecided share of hit pixels, first mismatch"""
    got_rgba = np.asarray(rgba)[ref.ys, ref.xs].astype(np.int64)
    got = np.asarray(idd)[ref.ys, ref.xs].astype(np.int64)
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
