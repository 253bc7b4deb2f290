"""The CPU oracle against the independent float64 restatement of the shader (tests/shader_ref64.py).

Every decided pixel must agree exactly (voxel ID, dist, RGBA8); each frame also states how many decided hit pixels it
checked and caps the undecided share, so no frame passes by deciding nothing. The planted flaws show that the
comparison can fail and that these scenes exercise every rule restated there."""
import ast
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, MAPS, ROOT, room_world, terrain_world
import shader_ref64 as R

UNDECIDED_CAP = 0.02          # of the hit pixels of a frame (measured: 0.1 % - 1.4 %)
TERRAIN_WINDOW = {"x0": 448, "z0": 660, "nx": 128, "nz": 128}   # 128 x 128 columns of config 4 in front of its pose
POSES = {"dragon": (63.5, 60.5, 140.5, -90.0, -10.0), "dragon_inside": (60.3, 30.7, 25.2, 37.0, 12.0),
         "monu9": (48.5, 60.5, 170.5, -90.0, -12.0), "nature": (60.5, 80.5, 200.5, -90.0, -20.0),
         "terrain": (512.5, 420.5, 1000.5, -90.0, -20.0), "room_inside": (14.5, 30.5, 16.5, 32.0, -10.0),
         "room_outside": (98.5, 34.5, 52.5, 197.0, -8.0)}


def light_dir_bits():
    g = json.load(open(os.path.join(GOLDEN, "camera.json")))
    return np.array(g["light_dir"], np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def scenes(V):
    """scene name -> (texels, tex_dim), flattened by the product host library"""
    out = {}
    for m in ("dragon", "monu9", "nature"):
        w = V.World()
        assert w.load_vox(os.path.join(MAPS, m + ".vox"))
        out[m] = w.flatten()
        w.close()
    out["terrain"] = terrain_world(V, window=TERRAIN_WINDOW).flatten()
    out["room"] = room_world(V).flatten()
    return out


_worlds = {}


def ref_world(scenes, name, tex=None, dim=None, wmin=(-1023,) * 3, wmax=(1024,) * 3):
    key = (name, tuple(wmin), tuple(wmax))
    if key not in _worlds:
        if tex is None:
            tex, dim = scenes[name]
        _worlds[key] = R.World(tex, dim, wmin, wmax)
    return _worlds[key]


class Case:
    """one frame: texels + uniforms + camera, rendered by the oracle and traced by the reference"""

    def __init__(self, V, tex, dim, pose, W, H, wmin=(-1023,) * 3, wmax=(1024,) * 3, scale=1.0, gl=(1, 1, 1, 1), light=None,
                 hl=(-1, -1, -1), camera=None):
        self.tex, self.dim, self.W, self.H = tex, dim, W, H
        self.wmin, self.wmax, self.scale, self.gl, self.hl = wmin, wmax, scale, gl, hl
        self.light = light_dir_bits() if light is None else np.asarray(light, np.float32)
        self.cam = camera if camera is not None else V.camera_block(pose[:3], pose[3], pose[4], W, H)[:3]

    def oracle(self, O, mode):
        s = O.make_scene(self.tex, self.dim, *self.cam, highlighted=self.hl)
        s.voxel_scale = self.scale
        s.bounds_min[:], s.bounds_max[:] = list(self.wmin), list(self.wmax)
        s.global_light[:] = [float(v) for v in self.gl]
        s.light_dir[:] = [float(v) for v in self.light]
        rgba, idd, _, _ = O.render(s, self.W, self.H, mode)
        return rgba, idd

    def trace(self, world, flaws=()):
        return R.Trace(world, *self.cam, self.W, self.H, voxel_scale=self.scale, global_light=self.gl, light_dir=self.light,
                       highlighted=self.hl, flaws=flaws)


def check(frame, rgba, idd, min_decided_hits, what, cap=UNDECIDED_CAP):
    r = R.compare(frame, rgba, idd)
    assert r["bad"] == 0, (what, r)
    assert r["decided_hits"] >= min_decided_hits, (what, r)
    assert r["undecided_share"] <= cap, (what, r)
    return r


def test_reference_never_touches_the_oracle_or_the_product():
    """shader_ref64.py, path_ref64.py, lens_ref64.py, deep_ref64.py and guide_ref64.py (on the first, second and third) read texels, a camera block, uniforms and the context's
    settings: they import numpy (path_ref64, lens_ref64 and deep_ref64 the first reference too, path_ref64 also deep_ref64) and
    nothing else, and name no file, library or entry point of oracle/, of the checkers or of the product's tracing."""
    for module, allowed in (("shader_ref64.py", {"numpy"}), ("path_ref64.py", {"numpy", "shader_ref64", "deep_ref64"}),
                            ("lens_ref64.py", {"numpy", "shader_ref64"}), ("deep_ref64.py", {"numpy", "shader_ref64"}),
                            ("guide_ref64.py", {"numpy", "shader_ref64", "path_ref64", "lens_ref64"})):
        _independent(module, allowed)


def _independent(module, allowed):
    tree = ast.parse(open(os.path.join(ROOT, "tests", module)).read())
    imported = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    imported |= {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert imported == allowed, imported
    names = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)} | {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)}
    for banned in ("open", "exec", "eval", "__import__", "ctypes", "CDLL", "subprocess", "importlib", "load", "fromfile",
                   "vrt", "dispatch", "render", "oracle_py", "oracle_samples", "oracle_jitter", "oracle_lens"):
        assert banned not in names, banned
    docs = {id(n.body[0].value) for n in ast.walk(tree) if isinstance(n, (ast.Module, ast.ClassDef, ast.FunctionDef))
            and n.body and isinstance(n.body[0], ast.Expr) and isinstance(n.body[0].value, ast.Constant)}
    strings = [n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str) and id(n) not in docs]
    assert strings
    for s in strings:
        for needle in ("oracle", ".so", "o_render", "o_octree", "vrt", "/"):
            assert needle not in s.lower(), (needle, s)


# min_hits: decided hit pixels each mode must check (~90 % of what was measured). The terrain window is seen from its golden
# pose ~300-800 voxels away at |coord| ~ 500-1000, where the float32 bound is several 1e-3 voxels: 5-10 % undecided there.
@pytest.mark.parametrize("scene,pose,W,H,min_hits,cap", [
    ("dragon", "dragon", 256, 144, 16000, UNDECIDED_CAP), ("dragon", "dragon", 97, 55, 2400, UNDECIDED_CAP),
    ("dragon", "dragon_inside", 101, 67, 6000, UNDECIDED_CAP), ("monu9", "monu9", 256, 144, 9400, UNDECIDED_CAP),
    ("monu9", "monu9", 61, 37, 640, UNDECIDED_CAP), ("nature", "nature", 256, 144, 16000, UNDECIDED_CAP),
    ("nature", "nature", 123, 71, 4000, UNDECIDED_CAP), ("terrain", "terrain", 240, 136, 1700, 0.12),
    ("terrain", "terrain", 77, 45, 190, 0.12), ("room", "room_inside", 256, 144, 15600, UNDECIDED_CAP),
    ("room", "room_outside", 256, 144, 12200, UNDECIDED_CAP), ("room", "room_inside", 83, 49, 1700, UNDECIDED_CAP)])
def test_oracle_matches_float64_reference(V, O, scenes, scene, pose, W, H, min_hits, cap):
    """modes 0 and 1 on every field, mode 2 on what the first hit decides (id/dist of opaque first hits, sky, emissive)"""
    tex, dim = scenes[scene]
    c = Case(V, tex, dim, POSES[pose], W, H)
    tr = c.trace(ref_world(scenes, scene))
    for mode in (0, 1, 2):
        rgba, idd = c.oracle(O, mode)
        check(tr.frame(mode), rgba, idd, min_hits, f"{scene}/{pose} {W}x{H} mode {mode}", cap)


@pytest.mark.parametrize("scene,pose", [("dragon", "dragon"), ("monu9", "monu9"), ("nature", "nature"), ("terrain", "terrain"),
                                        ("room", "room_outside")])
def test_full_mode_only_adds_light_to_opaque_scenes(V, O, scenes, scene, pose):
    """Seen from air, mode 2 keeps mode 1's ids and dists, its sky and its emissive pixels, and is channel-wise >= on every
    other pixel: the one bounce only adds non-negative terms (comp:596-616). The room's glass is left out (the stack)."""
    tex, dim = scenes[scene]
    c = Case(V, tex, dim, POSES[pose], 160, 90)
    ref = c.trace(ref_world(scenes, scene)).frame(1)
    rgba1, idd1 = c.oracle(O, 1)
    rgba2, idd2 = c.oracle(O, 2)
    first = np.zeros((90, 160), np.int64)
    first[ref.ys, ref.xs] = np.where(ref.dec_id, ref.kind, -1)
    glass = (first == R.KIND_TRANSLUCENT) | (first < 0)
    assert np.array_equal(idd2[~glass], idd1[~glass])
    same = (first == R.KIND_SKY) | (first == R.KIND_EMISSIVE)
    assert same.sum() > 0 and np.array_equal(rgba2[same], rgba1[same])
    assert np.all(rgba2[~glass] >= rgba1[~glass])
    if scene != "room":
        assert not (first == R.KIND_TRANSLUCENT).any()


def test_decoded_grid_agrees_with_octree_find_descent(scenes):
    """the painted index grid and the per-point descent are two readings of the same stream"""
    rng = np.random.default_rng(5)
    for name in ("dragon", "room", "terrain"):
        w = ref_world(scenes, name)
        p = rng.integers(w.g0 - 2, w.g1 + 2, size=(20000, 3))
        p = p[w.in_world(p)]
        assert np.array_equal(w.find(p), w.descend(p))
        n = w.find(p)
        assert np.all((w.mn[n] <= p) & (p < w.mx[n]))


# ---- hand-built edge worlds ------------------------------------------------------------------------------------------------
OPAQUE, GREY = 0xC08040FF, 0xA0A0A0FF


def _world(V, voxels, wmin=None, wmax=None):
    """voxels: (x, y, z, rgba, refraction, illumination) -> (texels, tex_dim)"""
    w = V.World(wmin, wmax)
    for x, y, z, c, r, i in voxels:
        w.insert(int(x), int(y), int(z), int(c), float(r), float(i), 0.0)
    out = w.flatten()
    w.close()
    return out


def _slab(x0, x1, y0, y1, z0, z1, c=GREY, r=3.0, i=0.0):
    return [(x, y, z, c, r, i) for x in range(x0, x1) for y in range(y0, y1) for z in range(z0, z1)]


def _identity_camera(eye):
    return (np.eye(4, dtype=np.float32).ravel(), np.eye(4, dtype=np.float32).ravel(), np.array([*eye, 1.0], np.float32))


def edge_cases(V):
    """name -> (Case, world bounds, what it pins, check(ref frames by mode))"""
    cases = {}
    L_up = np.array([0.3, 0.9, 0.2], np.float32) / np.float32(np.linalg.norm([0.3, 0.9, 0.2]))

    # the voxel at the origin, seen on its +X face: voxelID 0 like the sky, with a real dist
    tex, dim = _world(V, [(0, 0, 0, OPAQUE, 3.0, 0.0)])
    def origin(f):
        k = (f.xs == 31) & (f.ys == 15)
        assert f.kind[k][0] == R.KIND_OPAQUE and f.id[k][0] == 0 and f.dist[k][0] == 5 and f.dec_dist[k][0]
    cases["origin_plus_x"] = (Case(V, tex, dim, (6.5, 0.5, 0.5, 180.0, 0.0), 63, 31), origin)

    # refraction byte 85 (exactly 1.0) and 0 are air to hitMarching; alpha <= 25 is visible but casts no shadow; an
    # emissive voxel shows illum*10 and casts no shadow; all in front of / above a lit opaque floor
    vox = _slab(-8, 24, -1, 0, -8, 24)                                         # floor y = -1
    vox += _slab(0, 4, 2, 6, 0, 4, c=0xFF0000FF, r=1.0)                         # refraction 1.0 -> byte 85: invisible
    vox += _slab(6, 10, 2, 6, 0, 4, c=0x00FF00FF, r=0.0)                        # refraction 0: invisible
    vox += _slab(0, 4, 2, 6, 8, 12, c=0x2040FF14)                               # alpha 20: visible, no shadow
    vox += _slab(8, 12, 2, 6, 8, 12, c=0xFFC080FF, r=3.0, i=0.5)                # emissive: no shadow
    vox += _slab(14, 18, 2, 6, 2, 6)                                            # opaque: a shadow
    tex, dim = _world(V, vox)
    def materials(f):
        assert (f.kind == R.KIND_EMISSIVE).sum() > 50 and (f.kind == R.KIND_TRANSLUCENT).sum() > 50
        red = (f.rgba[:, 0] == 255) & (f.rgba[:, 1] == 0)
        assert not red.any()                                                   # the byte-85 block never shows
    cases["materials"] = (Case(V, tex, dim, (6.5, 14.5, 30.5, -100.0, -40.0), 160, 96, light=L_up), materials)

    # a highlighted glass voxel takes alpha 1: it gets an id and the opaque (lit) branch, colour inverted
    vox = _slab(-4, 12, -1, 0, -4, 12) + _slab(2, 6, 0, 4, 2, 6, c=0x80C0FF80, r=1.5)
    tex, dim = _world(V, vox)
    def highlight(f, lin=3 + dim * (3 + dim * 5)):
        k = f.dec_id & (f.kind == R.KIND_OPAQUE) & (f.id // 6 == lin)
        assert k.sum() > 20
    cases["highlight_glass"] = (Case(V, tex, dim, (4.5, 6.5, 14.5, -90.0, -20.0), 96, 64, hl=(3, 3, 5)), highlight)

    # voxels on the planes octreeFind splits unevenly on the negative side of the default world (-512, -513, -768)
    vox = _slab(-512, -511, 0, 6, 0, 6) + _slab(-513, -512, 8, 14, 0, 6) + _slab(-768, -767, 0, 6, 8, 14)
    vox += _slab(-770, -500, -2, -1, -4, 18)
    tex, dim = _world(V, vox)
    def planes(f):
        assert (f.dec_id & (f.id < 0)).sum() > 300                              # negative coordinates -> negative ids
    cases["negative_planes"] = (Case(V, tex, dim, (-480.5, 10.5, 6.5, 180.0, -5.0), 160, 90), planes)
    cases["negative_planes_far"] = (Case(V, tex, dim, (-700.5, 8.5, 30.5, -110.0, -12.0), 120, 80), planes)

    # a custom world with geometry against its bounds, and the eye next to the max corner
    vox = _slab(0, 16, 0, 1, 0, 16) + _slab(15, 16, 0, 16, 0, 16) + _slab(0, 16, 0, 16, 0, 1, c=0x4080C0FF)
    tex, dim = _world(V, vox, (0, 0, 0), (16, 16, 16))
    def bounds(f):
        assert (f.dec_id & (f.kind == R.KIND_OPAQUE)).sum() > 3000 and (f.dist[f.kind == R.KIND_SKY] == 16).all()
    cases["custom_bounds"] = (Case(V, tex, dim, (3.5, 12.5, 13.5, -60.0, -30.0), 96, 64, wmin=(0, 0, 0), wmax=(16, 16, 16)), bounds)

    # voxelScale 0.5 and 2.0: the grid origin is cameraPos * scale, dist is in world units
    vox = _slab(-8, 24, -1, 0, -8, 24) + _slab(2, 6, 0, 6, 2, 6) + _slab(10, 12, 0, 3, 4, 9, c=0x30A050FF)
    tex, dim = _world(V, vox)
    def scaled(f):
        assert (f.dec_id & (f.kind == R.KIND_OPAQUE)).sum() > 2000
    cases["scale_half"] = (Case(V, tex, dim, (12.5, 14.0, 40.5, -100.0, -20.0), 96, 64, scale=0.5), scaled)
    cases["scale_two"] = (Case(V, tex, dim, (3.25, 3.5, 10.25, -100.0, -20.0), 96, 64, scale=2.0, gl=(0.9, 0.8, 0.6, 1.0)), scaled)

    # a shadow ray that crosses more than 64 nodes before its occluder is lit by the cap (comp:352): a floor, a roof, and
    # between them a 3D checkerboard of alpha-20, refraction-0 voxels (air to primary rays, no shadow, but unit nodes)
    vox = _slab(-20, 44, 0, 1, -20, 44) + _slab(-40, 64, 84, 85, -40, 64)
    vox += [(x, y, z, 0x10101014, 0.0, 0.0) for x in range(0, 24) for y in range(1, 80) for z in range(0, 24) if (x + y + z) % 2]
    tex, dim = _world(V, vox)
    L_steep = np.array([0.1, 0.98, 0.15], np.float32) / np.float32(np.linalg.norm([0.1, 0.98, 0.15]))
    def cap(f):
        lit = f.dec_rgb.all(1) & (f.kind == R.KIND_OPAQUE) & (f.rgba[:, :3].sum(1) > 0)
        assert lit.sum() > 500
    cases["shadow_cap"] = (Case(V, tex, dim, (12.3, 60.5, 12.6, -90.0, -89.0), 64, 64, light=L_steep), cap)

    # exactly zero direction components (the 1e20 branch, comp:260-262): an identity camera block, even W and H, so
    # the middle column has d.x == 0 and the middle row d.y == 0; such rays never hit (comp:282-298)
    vox = _slab(-6, 6, -6, 6, -20, -18)
    tex, dim = _world(V, vox)
    def zero(f):
        mid = (f.xs == 32) | (f.ys == 16)
        assert f.dec_id[mid].all() and (f.kind[mid] == R.KIND_SKY).all()
        assert (f.dec_id & (f.kind == R.KIND_OPAQUE)).sum() > 150
    cases["zero_direction"] = (Case(V, tex, dim, None, 64, 32, camera=_identity_camera((0.5, 0.5, 0.5))), zero)
    return cases


@pytest.fixture(scope="module")
def edges(V):
    return edge_cases(V)


# the checkerboard of unit nodes puts a crossing near another node's edge on ~7 % of its rays (measured)
EDGE_CAPS = {"shadow_cap": 0.1, "negative_planes": 0.03, "zero_direction": 0.05}
EDGE_MIN_HITS = {"origin_plus_x": 30, "shadow_cap": 3000, "zero_direction": 150}
EDGE_NAMES = ["origin_plus_x", "materials", "highlight_glass", "negative_planes", "negative_planes_far", "custom_bounds",
              "scale_half", "scale_two", "shadow_cap", "zero_direction"]


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_worlds(O, edges, name):
    c, pin = edges[name]
    world = R.World(c.tex, c.dim, c.wmin, c.wmax)
    tr = c.trace(world)
    for mode in (0, 1, 2):
        rgba, idd = c.oracle(O, mode)
        f = tr.frame(mode)
        check(f, rgba, idd, EDGE_MIN_HITS.get(name, 1000), f"{name} mode {mode}", EDGE_CAPS.get(name, UNDECIDED_CAP))
        if mode == 1:
            pin(f)


def test_display_pass_matches_float64_quad_frag(V, O, scenes):
    """O.denoise against the float64 quad.frag on oracle frames (mode 2 and 0), at a seeded sample of pixels"""
    rng = np.random.default_rng(11)
    for scene, pose, mode in (("dragon", "dragon", 2), ("room", "room_inside", 2), ("monu9", "monu9", 0)):
        tex, dim = scenes[scene]
        c = Case(V, tex, dim, POSES[pose], 192, 108)
        rgba, idd = c.oracle(O, mode)
        shown = O.denoise(rgba, idd)
        xs, ys = rng.integers(0, 192, 3000), rng.integers(0, 108, 3000)
        want, dec = R.display(rgba, idd, xs, ys)
        got = shown[ys, xs].astype(np.int64)
        assert dec.mean() > 0.9 and (idd[ys, xs, 0] != 0).sum() > 500
        assert np.array_equal(got[:, :3][dec], want[:, :3][dec]), scene
        assert np.all(got[:, 3] == want[:, 3])


# ---- the comparison can fail: one planted misreading at a time ----------------------------------------------------------------
MUTATIONS = {"face_order": ["origin_plus_x", "negative_planes"], "pixel_center": ["materials"], "dist_round": ["custom_bounds"],
             "alpha_hit": ["materials"], "no_shadow_cap": ["shadow_cap"], "emissive_shadows": ["materials"],
             "highlight_alpha": ["highlight_glass"]}


@pytest.mark.parametrize("flaw", sorted(MUTATIONS) + ["display_across_ids"])
def test_each_planted_flaw_is_detected(O, edges, flaw):
    assert set(MUTATIONS) | {"display_across_ids"} == set(R.FLAWS)
    if flaw == "display_across_ids":
        c, _ = edges["materials"]
        rgba, idd = c.oracle(O, 1)
        ys, xs = np.mgrid[0:c.H:3, 0:c.W:3]
        want, dec = R.display(rgba, idd, xs, ys, flaws=(flaw,))
        got = O.denoise(rgba, idd)[ys.ravel(), xs.ravel()].astype(np.int64)
        assert (dec & (got[:, :3] != want[:, :3])).any()
        return
    bad = 0
    for name in MUTATIONS[flaw]:
        c, _ = edges[name]
        tr = c.trace(R.World(c.tex, c.dim, c.wmin, c.wmax), flaws=(flaw,))
        for mode in (0, 1):
            rgba, idd = c.oracle(O, mode)
            bad += R.compare(tr.frame(mode), rgba, idd)["bad"]
    assert bad > 0, flaw
