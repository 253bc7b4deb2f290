"""The worlds of the sample-stack sweep (test_sample_sweep.py, test_gpu_sample_sweep.py, fuzz/fuzz_samples.py) -- TEST INFRASTRUCTURE
ONLY, not collected by pytest.

case(V, O, family, index) is a pure function of (family, index): np.random.default_rng([SEED, family_id, index]) draws a world
out of fuzz_worlds.py's vocabulary -- slabs, clusters, its eight-material palette -- and three things the emitter rules need: an
emissive translucent material, a black emitter, and aligned filled cubes of one emissive material (2^3 at even corners, 4^3 at
multiple-of-4 corners: merged entries of the emitter list). With the world come its texels, records, emitter list and weights, the
uniforms (Case.fill_params for a vrt_params, Case.scene for the checker's), a pose, a frame size, a lens, a batch of 257 arbitrary
rays and the setting the schedule assigns to the case.

The pose rule uses the reference alone: a drawn pose is kept only if the checker's frame (corner sample 0, D = 1) has a voxel ID on
at least one eighth of the pixels (and, in every family but `inside`, only if the eye is in an empty cell); otherwise the next draw
of the same stream is taken, MAX_REDRAWS times at the most. An eye outside the world bounds sees nothing by the shader's own rule, so
it cannot pass: `far` 2 carries one as Case.outside_pose, beside its pose inside the bounds.

The schedule: case number c = 6 * family_id + index picks the path depth, the sun radius, the emitter rule, the ray source and the
variant. A stride modulo 4 per axis cannot cover every pair of values of two axes (all axes would be functions of c mod 4), so the
four 4-valued axes are the rows, the columns and two orthogonal Latin squares of order 4 over (c mod 4, c div 4 mod 4), the variant
the low bit of the third; the module asserts at import that every pair of values of two different axes occurs and every value at
least four times, with the `opaque` family's sampling-off half already applied."""
import itertools

import numpy as np

import oracle_emit_power as oep
from test_gpu_shade_rays import _ray_mix

SEED = 20261021
FAMILIES = ("opaque", "mixed", "inside", "origin", "uniforms", "far")
N_INDEX = 6
SIZES = ((33, 19), (24, 16))          # even, odd indices: ragged right and bottom tiles; whole 8 x 8 tiles only
N_RAYS = 257
N_SHARED = 65                         # the sub-batch that shares one origin: the first N_SHARED directions from the eye
MIN_HIT_SHARE = 8                     # the pose rule: hit pixels * 8 >= pixels
MAX_REDRAWS = 8
FAR_FLOOR = 400                       # the side of the `far` family's floor under the content
F = np.float32

# fuzz_worlds.py's palette (colour, refraction, illumination, k) ...
PALETTE = [(0xa0a0a0ff, 3.0, 0.0, 0.0), (0x50b43cff, 3.0, 0.0, 0.0), (0xffd2d2ff, 3.0, 1.0, 0.0), (0x3c64dc96, 1.33, 0.0, 0.02),
           (0xc8dcff50, 1.5, 0.0, 0.0), (0xff3030ff, 3.0, 0.25, 0.0), (0x20202000, 1.2, 0.0, 0.0), (0x80ff80c0, 1.0, 0.0, 0.0),
           # ... an emissive translucent material and a black emitter
           (0xffe0a0a0, 1.4, 0.6, 0.0), (0x000000ff, 3.0, 0.8, 0.0)]
STONE, GRASS, LAMP, WATER, GLASS, EMBER, AIR12, GREEN_GLASS, GLOW_GLASS, BLACK = range(10)
OPAQUE_ONLY = (STONE, GRASS, LAMP, EMBER, AIR12, BLACK)      # alpha 255 or 0: the stack-free full path tracer may run
INSIDE_KINDS = (GLASS, WATER, STONE, LAMP, AIR12, "cube")    # the `inside` family's eye voxel by index

DEPTHS = (1, 2, 3, 8)
RADII = (0.0, 0.00465, 0.05, 1.0)
RULES = ("off", "uniform", "power", "power+mis")
SOURCES = ("corner", "jitter", "lens", "jitter+lens")
VARIANTS = (0, 1)
AXES = (DEPTHS, RADII, RULES, SOURCES, VARIANTS)
_MUL2, _MUL3 = (0, 2, 3, 1), (0, 3, 1, 2)                    # multiplication by the two other non-zero elements of GF(4)


def sampling_off(family, index):
    """the `opaque` family's override: its even indices run with emitter sampling off"""
    return family == "opaque" and index % 2 == 0


def schedule(c):
    """-> the axis indices (depth, radius, rule, source, variant) of case number c"""
    a, b = c % 4, (c // 4 + c // 16) % 4
    rule = a ^ _MUL2[b]
    if sampling_off(FAMILIES[c // N_INDEX], c % N_INDEX):
        rule = 0
    return a, b, rule, a ^ b, (a ^ _MUL3[b]) & 1


def _assert_schedule():
    rows = [schedule(c) for c in range(len(FAMILIES) * N_INDEX)]
    for i, j in itertools.combinations(range(len(AXES)), 2):
        seen = {(r[i], r[j]) for r in rows}
        assert len(seen) == len(AXES[i]) * len(AXES[j]), f"axes {i} and {j}: {len(seen)} pairs"
    for i, axis in enumerate(AXES):
        for v in range(len(axis)):
            assert sum(r[i] == v for r in rows) >= 4, f"axis {i} value {v}"


_assert_schedule()


def setting_of(idx):
    return {"D": DEPTHS[idx[0]], "radius": RADII[idx[1]], "rule": RULES[idx[2]], "source": SOURCES[idx[3]], "variant": VARIANTS[idx[4]]}


def scheduled_setting(family, index):
    return setting_of(schedule(N_INDEX * FAMILIES.index(family) + index))


class Case:
    """one world with everything the sweep runs on it"""

    def name(self):
        s = self.setting
        return (f"sweep case {self.family} {self.index} [D={s['D']} radius={s['radius']} rule={s['rule']} source={s['source']} "
                f"variant={s['variant']}] {self.W} x {self.H}")

    def fill_params(self, p):
        """the case's uniforms into a vrt_params that holds the defaults -> p"""
        u = self.uniforms
        p.voxel_scale = u["voxel_scale"]
        p.global_light[:] = u["global_light"]
        p.light_dir[:] = u["light_dir"]
        p.highlighted[:] = u["highlighted"]
        if self.bounds:
            p.world_min[:] = self.bounds[0]
            p.world_max[:] = self.bounds[1]
        return p

    def scene(self, O, cam=None):
        u = self.uniforms
        s = O.make_scene(self.tex, self.dim, *(cam or self.cam))
        s.voxel_scale = u["voxel_scale"]
        s.global_light[:] = u["global_light"]
        s.light_dir[:] = u["light_dir"]
        s.highlighted[:] = u["highlighted"]
        if self.bounds:
            s.bounds_min[:] = self.bounds[0]
            s.bounds_max[:] = self.bounds[1]
        return s

    def close(self):
        self.world.close()


def _put(vox, xyz, m):
    for p in np.asarray(xyz, np.int64).reshape(-1, 3).tolist():
        vox[tuple(p)] = m


def _cube(vox, corner, size, m):
    g = np.arange(size)
    _put(vox, np.asarray(corner) + np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), m)


def _draw_voxels(rng, family, index):
    """-> ({(x, y, z): material}, [(corner, size)] of the emissive cubes, world bounds or None, the `far` family's floor (cells,
    material) or None). Later shapes overwrite earlier ones; the cubes come last, so each is whole: one merged leaf of the host tree."""
    vox = {}
    bounds = None
    palette = list(OPAQUE_ONLY) if family == "opaque" else list(range(len(PALETTE)))
    span = int(rng.choice([12, 24, 40]))
    around = family == "origin" or (family == "far" and index in (2, 3))
    base = np.zeros(3, np.int64)
    if family == "far" and index == 0:
        base[:] = 256                                        # content in the octant [0, 1024)^3 only, off the corner
    elif family == "far" and index == 1:
        bounds = ((0, 0, 0), (1024, 1024, 1024))             # custom world bounds
        base[:] = 220
    elif family == "far" and index == 2:
        bounds = ((-256,) * 3, (256,) * 3)                   # eight wide roots: no wide layout, the record-array kernels unasked
    elif family == "far":
        base[:] = 0 if around else 256
    elif not around:
        base[:] = rng.integers(0, 3, size=3) * int(rng.choice([0, 16, 64]))
    lo = -span // 2 if around else 0
    hi = span // 2 if around else span
    weight = np.array([0.25 if PALETTE[m][2] > 0 else 1.0 for m in palette])   # emitters are the rarer materials
    weight /= weight.sum()

    def material():
        return palette[int(rng.choice(len(palette), p=weight))]

    def clip(xyz):
        return np.clip(xyz, lo, hi - 1) + base

    _put(vox, clip(np.stack([g.ravel() for g in np.meshgrid(np.arange(lo, hi), [lo], np.arange(lo, hi), indexing="ij")], 1)),
         palette[int(rng.integers(0, 2))])                   # a floor, so that most downward looks end on something
    for _ in range(int(rng.integers(2, 5))):                 # slabs
        y = int(rng.integers(lo, lo + span // 2 + 1))
        x0, z0 = (int(v) for v in rng.integers(lo, hi - 2, size=2))
        sx, sz = (int(v) for v in rng.integers(2, 12, size=2))
        xs, zs = np.meshgrid(np.arange(x0, x0 + sx), np.arange(z0, z0 + sz))
        _put(vox, clip(np.stack([xs.ravel(), np.full(xs.size, y), zs.ravel()], 1)), material())
    if family == "origin":
        xs, zs = np.meshgrid(np.arange(-4, 5), np.arange(-3, 4))
        _put(vox, np.stack([xs.ravel(), np.zeros(xs.size, int), zs.ravel()], 1), STONE)       # one slab on the plane y = 0
        _put(vox, [(-1, 2, 1), (0, 2, 1), (-1, 3, -2), (0, 3, -2)], GLASS)                   # voxels on x = -1 / 0
    for _ in range(int(rng.integers(4, 10))):                # clusters
        c = rng.integers(lo, hi, size=3)
        k = int(rng.integers(4, 60))
        _put(vox, clip(c + rng.integers(-3, 4, size=(k, 3))), material())
    if family != "opaque":                                   # a standing pane, and every translucent kind at least once: three refractions
        x = int(rng.integers(lo + 2, hi - 2))
        ys, zs = np.meshgrid(np.arange(lo + 1, lo + 7), int(rng.integers(lo, hi - 6)) + np.arange(6))
        _put(vox, clip(np.stack([np.full(ys.size, x), ys.ravel(), zs.ravel()], 1)), (WATER, GLASS, GREEN_GLASS, GLOW_GLASS)[int(rng.integers(0, 4))])
        for m in (WATER, GLASS, GREEN_GLASS, GLOW_GLASS, AIR12):
            c = rng.integers(lo + 1, hi - 1, size=3)
            _put(vox, clip(c + rng.integers(-1, 2, size=(int(rng.integers(3, 12)), 3))), m)
    if family == "inside" and INSIDE_KINDS[index] != "cube":  # the eye's own kind of voxel
        _put(vox, clip(rng.integers(lo + 1, hi - 1, size=3) + rng.integers(-1, 2, size=(6, 3))), INSIDE_KINDS[index])
    for m in (LAMP, EMBER, BLACK):                           # single emitters, a black one among them
        _put(vox, clip(rng.integers(lo, hi, size=(int(rng.integers(1, 4)), 3))), m)
    cubes = []
    for size in (4, 2, 2):
        cells = (hi - lo) // size
        corner = (lo // size + rng.integers(0, cells, size=3)) * size
        if family == "origin" and size == 2:
            corner = -np.abs(corner) - size                   # a merged cube at negative coordinates
        corner = np.clip(corner, (lo // size) * size, ((hi - size) // size) * size) + base
        if any(np.all(np.abs(np.asarray(c0) + s0 / 2 - (corner + size / 2)) < (s0 + size) / 2) for c0, s0 in cubes):
            continue                                         # would overwrite part of an earlier cube
        _cube(vox, corner, size, LAMP if size == 4 or family != "origin" else EMBER)
        cubes.append((tuple(int(v) for v in corner), size))
    if family == "far" and index == 2:                       # test_world_with_eight_wide_roots_and_a_refused_one's cloud, thinned
        for p in rng.integers(-60, 70, size=(600, 3)).tolist():
            vox.setdefault(tuple(p), palette[int(rng.integers(0, 5))])
    if family == "far":                                      # from 700 units a pixel is some 30 voxels wide: a floor of FAR_FLOOR^2
        centre = base + (lo + hi) // 2
        g = np.arange(-FAR_FLOOR // 2, FAR_FLOOR // 2)
        xs, zs = np.meshgrid(g + centre[0], g + centre[2])
        far_floor = (np.stack([xs.ravel(), np.full(xs.size, lo - 1 + base[1]), zs.ravel()], 1), palette[int(rng.integers(0, 2))])
        return vox, cubes, bounds, far_floor
    return vox, cubes, bounds, None


def _build_world(V, vox, bounds, far_floor):
    w = V.World(*bounds) if bounds else V.World()
    if far_floor is not None:                                # one row below everything else: nothing overwrites it
        c, refr, illum, k = PALETTE[far_floor[1]]
        w.insert_many(far_floor[0].astype(np.int32), np.full(len(far_floor[0]), c, np.uint32), refr, illum, k)
    for m in range(len(PALETTE)):
        xyz = np.array([p for p, mm in vox.items() if mm == m], np.int32).reshape(-1, 3)
        if len(xyz):
            c, refr, illum, k = PALETTE[m]
            w.insert_many(xyz, np.full(len(xyz), c, np.uint32), refr, illum, k)
    return w


def _angles(d):
    yaw = float(np.degrees(np.arctan2(d[2], d[0])))
    pitch = float(np.clip(np.degrees(np.arctan2(d[1], np.hypot(d[0], d[2]))), -89.0, 89.0))
    return yaw, pitch


def _mergeable(vox, p):
    """the eight cells of p's aligned 2^3 block hold one material: the host tree keeps them as one leaf"""
    lo = [v & ~1 for v in p]
    return all(vox.get((lo[0] + dx, lo[1] + dy, lo[2] + dz)) == vox[p] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))


def _draw_pose(rng, family, index, vox, cubes, keys, scale, outside=False):
    """-> (x, y, z, yaw, pitch) in world units: a voxel-space eye divided by voxel_scale; outside: far 2's second pose, 700 away"""
    pts = np.array(keys, np.float64)
    target = pts[int(rng.integers(0, len(pts)))] + 0.5
    if family in ("mixed", "inside", "uniforms") and index % 2 == 0:   # half of these look at something translucent
        clear = [p for p in keys if (PALETTE[vox[p]][0] & 0xff) not in (0, 255)]
        target = np.asarray(clear[int(rng.integers(0, len(clear)))], np.float64) + 0.5
    if family == "inside":
        kind = INSIDE_KINDS[index]
        if kind == "cube":
            c0, s0 = cubes[0]
            eye = np.asarray(c0, np.float64) + rng.uniform(0.1, s0 - 0.1, size=3)
        else:
            own = [p for p in keys if vox[p] == kind and not _mergeable(vox, p)]
            eye = np.asarray(own[int(rng.integers(0, len(own)))], np.float64) + 0.5 + rng.uniform(-0.4, 0.4, size=3)
    else:
        away = rng.normal(size=3)
        away[1] = abs(away[1]) + 0.3
        away /= np.linalg.norm(away)
        if family == "far":
            dist = 230.0 if index == 2 and not outside else 700.0            # index 2: 700 is outside its world, where a ray sees nothing (C8)
            away[[0, 2]] *= 0.3                              # from above: the floor fills a good part of the frame
            away /= np.linalg.norm(away)
        else:
            dist = float(rng.choice([3.0, 8.0, 20.0, 35.0]))
        eye = target + away * dist
    yaw, pitch = _angles(target - eye if np.any(target - eye) else np.array([1.0, 0.0, 0.0]))
    eye = eye / scale
    return (float(eye[0]), float(eye[1]), float(eye[2]), yaw, pitch)


def _draw_uniforms(rng, family, index, vox, keys):
    u = {"voxel_scale": 1.0, "global_light": None, "light_dir": None, "highlighted": [-1, -1, -1]}
    if family != "uniforms":
        return u
    u["voxel_scale"] = float(F((0.5, 1.25, 2.0)[index % 3]))
    ld = rng.normal(size=3)
    ld[1] = abs(ld[1]) + 0.1                                 # the default sun stands above ...
    if index == 4:
        ld[1] = -ld[1]                                       # ... here it shines up from below
    if index in (1, 3):
        ld[(index // 2) * 2] = 0.0                           # one component exactly 0: x, then z
    ld = (ld / np.linalg.norm(ld)).astype(F)
    u["light_dir"] = [float(v) for v in ld]
    u["global_light"] = [float(v) for v in rng.uniform(0.0, 1.5, size=4).astype(F)]
    u["highlight_kinds"] = {0: (LAMP, EMBER, BLACK), 1: (GLASS, WATER, GREEN_GLASS), 2: None}[index // 2]   # an emitter, glass, any voxel
    return u


def _lens(rng, focus):
    """-> (aperture, focus distance) in world units"""
    return (float(F(rng.uniform(0.05, 0.6))), float(F(max(focus, 1.0))))


def case(V, O, family, index, setting=None, seed=SEED):
    """The case (family, index); `setting` replaces the scheduled one and `seed` the suite's (fuzz_samples.py draws its own settings,
    under its own seed, at any index: what a family does by index it does by index % N_INDEX)"""
    fid = FAMILIES.index(family)
    rng = np.random.default_rng([seed, fid, index])
    number, index = index, index % N_INDEX
    vox, cubes, bounds, far_floor = _draw_voxels(rng, family, index)
    assert cubes, "no emissive cube fitted"
    keys = sorted(vox)
    c = Case()
    c.family, c.index, c.seed, c.bounds, c.cubes, c.vox = family, number, seed, bounds, cubes, vox
    c.W, c.H = SIZES[index % 2]
    c.setting = dict(setting or scheduled_setting(family, index))
    c.world = _build_world(V, vox, bounds, far_floor)
    c.tex, c.dim = c.world.flatten()
    c.records = c.world.records()[0]
    c.list, c.words = oep.walk(c.records, *(bounds or ()))
    c.weights = np.array(oep.weights(c.list, c.words), np.uint64)
    c.uniforms = _draw_uniforms(rng, family, index, vox, keys)
    defaults = O.make_scene(c.tex, c.dim, np.zeros(16, F), np.zeros(16, F), np.zeros(4, F))
    for k in ("global_light", "light_dir"):
        if c.uniforms[k] is None:
            c.uniforms[k] = [float(v) for v in getattr(defaults, k)]
    scale = c.uniforms["voxel_scale"]
    for redraw in range(MAX_REDRAWS + 1):
        pose = _draw_pose(rng, family, index, vox, cubes, keys, scale)
        cam = V.camera_block(pose[:3], pose[3], pose[4], c.W, c.H)[:3]
        if family != "inside" and tuple(np.floor(np.asarray(cam[2][:3], np.float64) * F(scale)).astype(int).tolist()) in vox:
            hits = 0                                         # these families' eyes are in empty space: a draw inside a voxel is not kept
            continue
        ids = O.render(c.scene(O, cam), c.W, c.H, 2)[1][..., 0]
        hits = int(np.count_nonzero(ids))
        if hits * MIN_HIT_SHARE >= c.W * c.H:
            break
    else:
        raise AssertionError(f"{family} {index}: no pose with a voxel on an eighth of the frame in {MAX_REDRAWS + 1} draws")
    c.pose, c.cam, c.redraws, c.hit_pixels = pose, cam, redraw, hits
    # the eye outside the world bounds, looking in: every ray is sky by the shader's rule, so the pose rule cannot apply to it
    c.outside_pose = _draw_pose(rng, family, index, vox, cubes, keys, scale, outside=True) if (family, index) == ("far", 2) else None
    if family == "uniforms":
        c.uniforms["highlighted"] = _highlight(rng, O, c, vox, keys, c.uniforms.pop("highlight_kinds"))
    eye_vox = np.asarray(pose[:3]) * scale
    c.lens = _lens(rng, float(np.linalg.norm(np.asarray(keys[len(keys) // 2], np.float64) + 0.5 - eye_vox)) / scale)
    lo, hi = np.min(keys, axis=0), np.max(keys, axis=0) + 1
    glass = [p for p in keys if (PALETTE[vox[p]][0] & 0xff) not in (0, 255)] or keys
    solid = [p for p in keys if (PALETTE[vox[p]][0] & 0xff) == 255]
    g, s = glass[int(rng.integers(0, len(glass)))], solid[int(rng.integers(0, len(solid)))]
    o, d = _ray_mix(rng, N_RAYS, lo, hi, (g, tuple(v + 1 for v in g)), (s, tuple(v + 1 for v in s)))
    c.rays = ((o / F(scale)).astype(F), d)
    c.shared_origin = np.array(pose[:3], F)
    return c


def _highlight(rng, O, c, vox, keys, kinds):
    """a voxel of `kinds` (None: any) that the frame shows: the first of a drawn order whose highlight changes a byte of the checker's
    primary frame; where none of 300 does, the first of that order"""
    own = [p for p in keys if kinds is None or vox[p] in kinds]
    order = [own[i] for i in rng.permutation(len(own))[:300]]
    s = c.scene(O)
    s.highlighted[:] = [-1, -1, -1]
    plain = O.render(s, c.W, c.H, 0)[0]
    for p in order:
        s.highlighted[:] = list(p)
        if not np.array_equal(O.render(s, c.W, c.H, 0)[0], plain):
            return [int(v) for v in p]
    return [int(v) for v in order[0]]
