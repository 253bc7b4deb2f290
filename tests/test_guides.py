"""The guide planes' checker (tests/oracle_guides.c) on the CPU: hand-built worlds whose first hit is known in closed form, the
float64 reference's first hit (tests/shader_ref64.py) on the committed small frames, the independence of the planes from how
the samples were split, and two planted misreadings that the closed forms catch."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import MAPS, room_world, terrain_world
import guide_worlds as GW
import oracle_guides as G
import shader_ref64 as R
from test_shader_reference64 import POSES, TERRAIN_WINDOW, UNDECIDED_CAP, light_dir_bits

W, H = 33, 17                   # odd: the middle pixel's corner ray is a little off the axis, no component is zero
CX, CY = 16, 8
OPAQUE = 0xC08040FF             # R, G, B, A = 192, 128, 64, 255
BYTES = np.array([0xC0, 0x80, 0x40, 0xFF], np.uint8)
GLASS, GLASS_REFR = 0x80C0FF80, 1.5
GLASS_BYTES = np.array([0x80, 0xC0, 0xFF, 0x80], np.uint8)
VIEWS = ((0, 0), (180, 0), (90, 0), (-90, 0), (0, 89), (0, -89))   # yaw, pitch: along +x, -x, +z, -z, +y, -y


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return G.build(tmp_path_factory.mktemp("oracle_guides"))


def _world(V, voxels):
    """voxels: (x, y, z, rgba, refraction, illumination) -> (texels, tex_dim)"""
    w = V.World()
    for x, y, z, c, r, i in voxels:
        w.insert(int(x), int(y), int(z), int(c), float(r), float(i), 0.0)
    out = w.flatten()
    w.close()
    return out


def _slab(x0, x1, y0, y1, z0, z1, c=OPAQUE, r=3.0):
    return [(x, y, z, c, r, 0.0) for x in range(x0, x1) for y in range(y0, y1) for z in range(z0, z1)]


def _main_axis(V, yaw, pitch):
    """the axis and sign the camera looks along"""
    iv = V.camera_block((0.0, 0.0, 0.0), yaw, pitch, W, H)[1]
    d = -np.array(iv[8:11], np.float64)
    a = int(np.argmax(np.abs(d)))
    return a, 1 if d[a] > 0 else -1


def _dir(cam, px, py):
    """the float64 direction of the corner ray of pixel (px, py)"""
    ip, iv = (np.array(m, np.float32).astype(np.float64).reshape(4, 4).T for m in cam[:2])
    return R.ray_dirs(ip, iv, np.array([px]), np.array([py]), W, H)[0]


def _six(V, L, O, plant=None):
    """the one voxel (10, 10, 10) seen along each axis from 9 units off its centre -> per view (guide, axis, sign, direction)"""
    tex, dim = _world(V, [(10, 10, 10, OPAQUE, 3.0, 0.0)])
    out = []
    for yaw, pitch in VIEWS:
        a, sg = _main_axis(V, yaw, pitch)
        eye = np.full(3, 10.5)
        eye[a] -= 9.0 * sg
        cam = V.camera_block(tuple(eye), yaw, pitch, W, H)[:3]
        g = G.sample(L, O.make_scene(tex, dim, *cam), W, H, 0, plant=plant)
        out.append((g, a, sg, _dir(cam, CX, CY)))
    return out


def test_single_voxel_along_each_axis(V, L, O):
    """the face towards the eye: normal -sign(d) on the view's axis, the voxel's four bytes, depth 8.5 / |d_axis|"""
    seen = set()
    for g, a, sg, d in _six(V, L, O):
        assert g.hit[CY, CX] == 1 and 1 <= g.hit.sum() <= 12
        want = np.zeros(3, np.int8)
        want[a] = -sg
        assert np.array_equal(g.normal[CY, CX], want)
        assert np.array_equal(g.albedo[CY, CX], BYTES)
        assert np.array_equal(g.cell[CY, CX], [10, 10, 10])
        assert abs(float(g.depth[CY, CX]) - 8.5 / abs(d[a])) < 1e-3      # the 1e-4 push along the ray, float32 rounding
        assert not g.normal[g.hit == 0].any() and not g.albedo[g.hit == 0].any() and not g.depth[g.hit == 0].any()
        seen.add((a, -sg))
    assert len(seen) == 6


def test_planted_normal_sign_is_caught(V, L, O):
    for g, a, sg, _ in _six(V, L, O, plant="normal_sign"):
        assert g.normal[CY, CX][a] == sg                                    # the flipped sign: the check above fails on it


def _glass_exit(V, L, O, phantom):
    """the eye inside a block of glass looking along +x: the march hits where the medium ends, in the cell after the glass"""
    vox = _slab(0, 8, 0, 8, 0, 8, c=GLASS, r=GLASS_REFR)
    if phantom:
        vox += _slab(8, 9, 0, 8, 0, 8, c=0x11223300, r=3.0)                 # alpha 0: a leaf that is there and is air
    tex, dim = _world(V, vox)
    cam = V.camera_block((2.5, 4.5, 4.5), 0, 0, W, H)[:3]
    return G.sample(L, O.make_scene(tex, dim, *cam), W, H, 0), _dir(cam, CX, CY)


@pytest.mark.parametrize("phantom", [False, True])
def test_alpha0_hit_leaf_takes_the_previous_voxels_bytes(V, L, O, phantom):
    """comp:505-507: the hit leaf behind the glass has alpha 0 (empty space, or a phantom leaf of alpha 0), so the surface colour is
    the glass the ray leaves -- all four bytes, its alpha too"""
    g, d = _glass_exit(V, L, O, phantom)
    assert g.hit[CY, CX] == 1
    assert np.array_equal(g.cell[CY, CX], [8, 4, 4])
    assert np.array_equal(g.albedo[CY, CX], GLASS_BYTES)
    assert np.array_equal(g.normal[CY, CX], [-1, 0, 0])
    assert abs(float(g.depth[CY, CX]) - 5.5 / abs(d[0])) < 1e-3


def test_highlighted_voxel_inverts_rgb_and_takes_alpha_255(V, L, O):
    tex, dim = _world(V, [(10, 10, 10, GLASS, GLASS_REFR, 0.0)])
    cam = V.camera_block((1.5, 10.5, 10.5), 0, 0, W, H)[:3]
    plain = G.sample(L, O.make_scene(tex, dim, *cam), W, H, 0)
    marked = G.sample(L, O.make_scene(tex, dim, *cam, highlighted=(10, 10, 10)), W, H, 0)
    assert plain.hit[CY, CX] == 1 and np.array_equal(plain.albedo[CY, CX], GLASS_BYTES)
    assert np.array_equal(marked.albedo[CY, CX], [255 - 0x80, 255 - 0xC0, 255 - 0xFF, 255])
    assert np.array_equal(marked.normal, plain.normal) and np.array_equal(marked.depth, plain.depth)


def test_glass_pane_shows_alpha_below_one_and_nothing_behind_it(V, L, O):
    """through glass the guide is the glass surface: the wall behind the pane does not show"""
    tex, dim = _world(V, _slab(10, 11, 0, 21, 0, 21, c=GLASS, r=GLASS_REFR) + _slab(14, 15, 0, 21, 0, 21))
    cam = V.camera_block((2.5, 10.5, 10.5), 0, 0, W, H)[:3]
    planes, _ = G.planes(L, O.make_scene(tex, dim, *cam), W, H, 0, 1)
    assert planes["coverage"][CY, CX] == 1.0
    assert np.array_equal(planes["albedo"][CY, CX], (GLASS_BYTES.astype(np.float64) / 255.0).astype(np.float32))
    assert planes["albedo"][CY, CX, 3] < 1.0
    assert abs(float(planes["depth"][CY, CX]) - 7.5 / abs(_dir(cam, CX, CY)[0])) < 1e-3


def test_all_miss_frame_is_all_zeros(V, L, O):
    tex, dim = _world(V, [(10, 10, 10, OPAQUE, 3.0, 0.0)])
    cam = V.camera_block((1.5, 10.5, 10.5), 180, 0, W, H)[:3]                # looking away
    planes, st = G.planes(L, O.make_scene(tex, dim, *cam), W, H, 3, 4, jitter=True)
    assert st.n == 4
    for k in G.KEYS:
        assert not planes[k].any(), k
        assert not np.signbit(planes[k]).any(), k


# ---- the checker's first hit against the float64 reference ---------------------------------------------------------------------
FRAMES = {"dragon": ("dragon", UNDECIDED_CAP), "room": ("room_inside", UNDECIDED_CAP), "terrain": ("terrain", 0.12)}


@pytest.fixture(scope="module")
def scenes(V):
    out = {}
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    out["dragon"] = w.flatten()
    w.close()
    out["room"] = room_world(V).flatten()
    out["terrain"] = terrain_world(V, window=TERRAIN_WINDOW).flatten()
    return out


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_first_hit_matches_float64_reference(V, L, O, scenes, name):
    """Wherever the reference's error model keeps the pixel: hit or miss, the hit cell, the face and the four albedo bytes are
    equal, and the depth lies within the model's float32 bound of the reference's: its position margin e on the hit point
    (sqrt(3) e in length) plus e / |d[ax]| for the last crossing, plus the length's own 4u. (The model's margin on dist, e + 4u * length,
    leaves the last crossing's term out, which an integer dist rarely sees: the dragon frame's depths pass it at all but 4 of 16,639
    pixels, whose last crossing is grazing -- |d[ax]| <= 0.05, over by up to 2.3e-4; printed per frame.) The share of hit pixels left
    out is no larger than the share tests/test_shader_reference64.py leaves out of the same frame (its mode 1), and within that test's
    cap."""
    pose, cap = FRAMES[name]
    fw, fh = 240, 136
    tex, dim = scenes[name]
    cam = V.camera_block(POSES[pose][:3], POSES[pose][3], POSES[pose][4], fw, fh)[:3]
    scene = O.make_scene(tex, dim, *cam)
    scene.light_dir[:] = [float(v) for v in light_dir_bits()]
    g = G.sample(L, scene, fw, fh, 0)
    tr = R.Trace(R.World(tex, dim), *cam, fw, fh, light_dir=light_dir_bits())
    keep = ~tr.amb & ~tr.outside
    hit = g.hit[tr.ys, tr.xs] != 0
    assert np.array_equal(hit[keep], tr.hit[keep])
    k = keep & tr.hit
    assert k.sum() > 1500
    assert np.array_equal(g.cell[tr.ys, tr.xs][k], tr.mp[k])
    s = -np.sign(tr.d[np.arange(len(tr.ax)), tr.ax])
    want_n = np.zeros((len(tr.ax), 3), np.int64)
    want_n[np.arange(len(tr.ax)), tr.ax] = s
    want_n[s == 0] = (0, 1, 0)
    assert np.array_equal(g.normal[tr.ys, tr.xs][k], want_n[k])
    w = tr.w
    hva = w.a[tr.hv] > 0
    want_a = np.concatenate([np.where(hva[:, None], w.rgb[tr.hv], w.rgb[tr.lv]), np.where(hva, w.a[tr.hv], w.a[tr.lv])[:, None]], 1)
    assert np.array_equal(g.albedo[tr.ys, tr.xs][k].astype(np.int64), want_a[k].astype(np.int64))
    ln = np.linalg.norm(tr.pt / tr.scale - tr.org, axis=1)
    e = R.DELTA_FLOOR + R.DELTA_SAFETY * tr.err                  # the model's margin on every coordinate of rayPos
    plain = e / tr.scale + 4 * R.U * ln                          # ... and Trace.frame()'s margin on dist, which is a length too
    # The depth is a float, not dist's integer, so the last crossing counts: t = (plane - pos[ax]) / d[ax] carries pos[ax]'s e into
    # the hit point as e / |d[ax]| along the ray (|d| = 1), on top of the point's own e per coordinate (sqrt(3) e in length).
    amp = 1.0 / np.maximum(np.abs(tr.d[np.arange(len(tr.ax)), tr.ax]), 1e-30)
    bound = (np.sqrt(3.0) + amp) * e / tr.scale + 4 * R.U * ln
    err = np.abs(g.depth[tr.ys, tr.xs].astype(np.float64) - ln)
    over = k & (err > plain)
    print(f"{name}: depth beyond the plain dist margin at {int(over.sum())} of {int(k.sum())} pixels"
          + (f", by up to {float((err - plain)[over].max()):.2e} at |d[ax]| <= {float((1.0 / amp)[over].max()):.3f}" if over.any() else ""))
    assert (err[k] <= bound[k]).all(), float((err[k] - bound[k]).max())
    left_out = float((~keep[tr.hit]).mean())
    theirs = tr.frame(1).hit_undecided_share()
    print(f"{name}: {int(k.sum())} hit pixels compared, left out {left_out:.4f} (test_shader_reference64 mode 1: {theirs:.4f}, cap {cap})")
    assert left_out <= theirs and left_out <= cap


# ---- the sums ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter,aperture", [(True, 0.0), (False, 1.5), (True, 1.5)])
def test_split_independence(V, L, O, scenes, jitter, aperture):
    """3 + 5 samples are 8, bit for bit, in the state and in every plane"""
    tex, dim = scenes["room"]
    pose = POSES["room_inside"]
    cam = V.camera_block(pose[:3], pose[3], pose[4], 40, 24)[:3]
    scene = O.make_scene(tex, dim, *cam)
    whole, st8 = G.planes(L, scene, 40, 24, 5, 8, jitter, aperture, 20.0)
    _, st3 = G.planes(L, scene, 40, 24, 5, 3, jitter, aperture, 20.0)
    split, st35 = G.planes(L, scene, 40, 24, 8, 5, jitter, aperture, 20.0, state=st3)
    assert st35.n == 8 and 0 < whole["coverage"].sum()
    G.same(split, whole, f"3 + 5 vs 8 (jitter {jitter}, aperture {aperture})")
    for a, b in ((st35.asum, st8.asum), (st35.nsum, st8.nsum), (st35.hits, st8.hits), (st35.dsum.view(np.uint64), st8.dsum.view(np.uint64))):
        assert np.array_equal(a, b)
    # jitter moves the samples: a mean over 8 is not one sample's plane
    one, _ = G.planes(L, scene, 40, 24, 5, 1, jitter, aperture, 20.0)
    assert not np.array_equal(one["depth"], whole["depth"])


def test_resolve_arithmetic(L):
    """the planes of a hand-written state: float64 divisions, one rounding"""
    st = G.State(L, (1, 2))
    st.n = 3
    st.asum[0, 0] = (255 * 3, 128 * 2, 1, 0)
    st.nsum[0, 0] = (-2, 0, 1)
    st.hits[0, 0] = 3
    st.dsum[0, 0] = 10.0
    out = st.resolve()
    assert np.array_equal(out["albedo"][0, 0], np.array([1.0, 256 / 765.0, 1 / 765.0, 0.0]).astype(np.float32))
    assert np.array_equal(out["normal"][0, 0], np.array([-2 / 3.0, 0.0, 1 / 3.0]).astype(np.float32))
    assert out["coverage"][0, 0] == 1.0 and out["depth"][0, 0] == np.float32(10.0 / 3.0)
    assert not any(out[k][0, 1].any() for k in G.KEYS)                     # no hit: depth 0, not 0 / 0


# ---- the depth is measured from the sample's own origin -------------------------------------------------------------------------
def _lens_wall(V, L, O, plant):
    """a wall x = 30 seen through a lens of aperture 2 focused at 10: per pixel the checker's depth and the closed form
    (30 - o.x) / d.x from the sample's own origin o and direction d (tests/oracle_lens.c o_lens_ray)"""
    tex, dim = _world(V, _slab(30, 31, -20, 40, -20, 40))
    cam = V.camera_block((2.5, 10.5, 10.5), 0, 0, W, H)[:3]
    scene = O.make_scene(tex, dim, *cam)
    k, ap, focus = 5, 2.0, 10.0
    g = G.sample(L, scene, W, H, k, False, ap, focus, plant=plant)
    L.o_lens_ray.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    L.o_lens_ray.restype = C.c_int
    o, d = np.zeros(3, np.float32), np.zeros(3, np.float32)
    moved = L.o_lens_ray(C.addressof(scene), W, H, CX, CY, k, 0, ap, focus, o.ctypes.data, d.ctypes.data)
    assert moved == 1 and np.linalg.norm(o - np.array(cam[2][:3], np.float32)) > 0.5
    return float(g.depth[CY, CX]), (30.0 - float(o[0])) / float(d[0])


def test_lens_depth_is_from_the_lens_origin_and_the_planted_eye_is_caught(V, L, O):
    got, want = _lens_wall(V, L, O, None)
    assert abs(got - want) < 1e-3
    got, want = _lens_wall(V, L, O, "depth_from_eye")
    assert abs(got - want) > 1e-2


# ---- what the GPU tests assume of their fixtures (tests/guide_worlds.py), checked here ----------------------------------------------
@pytest.mark.parametrize("name", sorted(GW.FRAMES))
def test_gpu_frames_have_hits_misses_glass_and_no_voxel_at_linear_index_0(V, L, O, name):
    """voxel ID 0 must mean "no opaque first hit" in these frames: no sample's guide hits cell (0, 0, 0) (linear index 0, face 0)"""
    w = GW.world(V, name)
    tex, dim = w.flatten()
    w.close()
    scene = O.make_scene(tex, dim, *GW.camera(V, name))
    glass = 0
    for source, (jitter, lens) in GW.SOURCES.items():
        ap, focus = GW.lens_of(name, source)
        for k in range(GW.FIRST, GW.FIRST + GW.N):
            g = G.sample(L, scene, GW.W, GW.H, k, jitter, ap, focus)
            assert g.hit.sum() > GW.W * GW.H // 4
            assert not ((g.cell == 0).all(-1) & (g.hit != 0)).any()
            glass += int(((g.albedo[..., 3] < 255) & (g.hit != 0)).sum())
    assert glass > 50


def test_picking_rays_hit_wherever_the_host_ray_cast_hits(V, L, O):
    """the lamp room has no zero-word leaves: every ray octree_ray_cast answers with a voxel has a guide hit (0 ghost-leaf rays)"""
    w = GW.world(V, "lamp")
    tex, dim = w.flatten()
    o, d = GW.picking_rays()
    cast, _ = w.ray_cast_many(tuple(float(v) for v in o), d)
    w.close()
    g = G.rays(L, O.make_scene(tex, dim, *GW.camera(V, "lamp")), o, d)
    assert (cast == 1).sum() > 250
    ghost = int(((cast == 1) & (g.hit == 0)).sum())
    assert ghost == 0
