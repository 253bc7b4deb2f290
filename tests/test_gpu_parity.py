"""Parity of the gfx950 kernels (through the C-ABI) against the CPU oracle and the committed golden frames.

Bit-exact bar: RGBA8 and RG32I outputs must be identical, pixel for pixel."""
import os

import numpy as np
import pytest

from conftest import MAPS

pytestmark = pytest.mark.gpu

import vrt_import

VARIANTS = vrt_import.vrt().available_variants()   # 0, 1, 4, 20, 22
# VRT_OPT_DISPLAY_KERNEL: 0 = two pixels per lane, each wave the cheaper of its two walks (shipped); 2 / 3 = one walk forced (the wave's common
# rows / every pixel its own box)
DISPLAY_KERNELS = (2, 3, 0)   # the shipped setting last: the shared context keeps it


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _setup(ctx, V, tex, dim, pose, W, H, highlighted=None):
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    ctx.upload_octree(tex, dim)
    ctx.set_camera(ip, iv, cp)
    p = ctx.default_params()
    if highlighted is not None:
        p.highlighted[:] = highlighted
    ctx.set_params(p)
    return ip, iv, cp


def _oracle_frame(O, tex, dim, cam, W, H, mode, highlighted=(-1, -1, -1)):
    s = O.make_scene(tex, dim, *cam, highlighted=highlighted)
    rgba, idd, _, st = O.render(s, W, H, mode)
    return rgba, idd, st


def _assert_same(got, ref, what):
    if not np.array_equal(got, ref):
        bad = np.argwhere(np.any(got != ref, axis=-1))
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} pixels differ; first at (x={x}, y={y}): got {got[y, x]} want {ref[y, x]}")


def test_arithmetic_contract_on_device(ctx):
    """'/', sqrt, floor, rint are correctly rounded and a*b+c is not fused: compared with numpy float32."""
    rng = np.random.default_rng(0)
    n = 1 << 16
    a = np.concatenate([rng.normal(size=n // 2) * 10.0 ** rng.integers(-30, 30, size=n // 2),
                        rng.uniform(-1100, 1100, size=n // 2)]).astype(np.float32)
    b = np.concatenate([rng.normal(size=n // 2) * 10.0 ** rng.integers(-30, 30, size=n // 2),
                        rng.uniform(-3, 3, size=n // 2)]).astype(np.float32)
    b[b == 0] = 1.0
    with np.errstate(all="ignore"):
        assert np.array_equal(ctx.debug_math(0, a, b).view(np.uint32), (a / b).astype(np.float32).view(np.uint32))
        pa = np.abs(a)
        assert np.array_equal(ctx.debug_math(1, pa, b).view(np.uint32), np.sqrt(pa).view(np.uint32))
        assert np.array_equal(ctx.debug_math(2, pa + np.float32(1e-30), b).view(np.uint32),
                              (np.float32(1.0) / np.sqrt(pa + np.float32(1e-30))).view(np.uint32))
        assert np.array_equal(ctx.debug_math(3, a, b).view(np.uint32), np.floor(a).view(np.uint32))
        assert np.array_equal(ctx.debug_math(4, a, b).view(np.uint32), np.rint(a).view(np.uint32))
        prod = (a * b).astype(np.float32)
        assert np.array_equal(ctx.debug_math(5, a, b).view(np.uint32), (prod + np.float32(1.0)).view(np.uint32))
        assert np.array_equal(ctx.debug_math(8, a, b).view(np.uint32), (a + b).view(np.uint32))
        assert np.array_equal(ctx.debug_math(9, a, b).view(np.uint32), prod.view(np.uint32))


def test_det_exp_matches_oracle(ctx, O):
    x = np.linspace(-90, 89, 20001).astype(np.float32)
    got = ctx.debug_math(6, x, x)
    ref = np.array([O.lib().o_det_expf(float(v)) for v in x], np.float32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_full_mode_math_conventions_match_oracle(ctx, O):
    """The polynomial sin/cos/pow standing in for GLSL's transcendentals, floor-to-int and rand()'s uint->float."""
    L = O.lib()
    phi = np.linspace(0.0, 6.2832, 30001).astype(np.float32)
    ref_s = np.array([L.o_det_sinf(float(v)) for v in phi], np.float32)
    ref_c = np.array([L.o_det_cosf(float(v)) for v in phi], np.float32)
    assert np.array_equal(ctx.debug_math(10, phi, phi).view(np.uint32), ref_s.view(np.uint32))
    assert np.array_equal(ctx.debug_math(11, phi, phi).view(np.uint32), ref_c.view(np.uint32))
    x = np.linspace(0.0, 1.0, 20001).astype(np.float32)
    five = np.full_like(x, 5.0)
    ref_p = np.array([L.o_det_powf(float(v), 5.0) for v in x], np.float32)
    assert np.array_equal(ctx.debug_math(12, x, five).view(np.uint32), ref_p.view(np.uint32))
    rng = np.random.default_rng(3)
    f = np.concatenate([rng.uniform(-1100, 1100, 50000), [-0.0, 0.0, -1e-40, 1e-40, -1.0, 1.0, -0.99999994, 1023.9999],
                        np.arange(-8, 8) + 1e-4, np.arange(-8, 8) - 1e-4]).astype(np.float32)
    assert np.array_equal(ctx.debug_math(13, f, f), np.floor(f).astype(np.int32).astype(np.float32))
    byte = np.arange(256, dtype=np.float32)   # colour/property bytes -> [0, 1] without a division (vrt_common.hip.h unorm_of)
    assert np.array_equal(ctx.debug_math(15, byte, byte).view(np.uint32), (byte / np.float32(255.0)).view(np.uint32))
    u = rng.integers(0, 2 ** 32, 50000, dtype=np.uint64).astype(np.uint32)
    u[:4] = [0, 0xffffffff, 0xffffff7f, 0x80000000]
    ref_u = (u.astype(np.float32) / np.float32(4294967296.0)).astype(np.float32)
    assert np.array_equal(ctx.debug_math(14, u.view(np.float32), u.view(np.float32)).view(np.uint32), ref_u.view(np.uint32))


@pytest.mark.parametrize("key", ["dragon_256x144/mode0", "dragon_256x144/mode1", "monu9_192x108/mode0",
                                 "monu9_192x108/mode1", "nature_200x112/mode0", "nature_200x112/mode1",
                                 "dragon_inside_101x67/mode0", "dragon_inside_101x67/mode1", "dragon_256x144/mode2",
                                 "monu9_192x108/mode2", "nature_200x112/mode2", "dragon_inside_101x67/mode2",
                                 "room_inside_256x144/mode0", "room_inside_256x144/mode1", "room_inside_256x144/mode2",
                                 "room_outside_256x144/mode0", "room_outside_256x144/mode1", "room_outside_256x144/mode2"])
def test_small_frames_vs_oracle_and_golden(ctx, V, O, golden, product_scenes, key):
    g = golden["frames"]["frames"][key]
    tex, dim = product_scenes[g["map"]]
    W, H = g["width"], g["height"]
    cam = _setup(ctx, V, tex, dim, g["pose"], W, H)
    ref_rgba, ref_id, _ = _oracle_frame(O, tex, dim, cam, W, H, g["mode"])
    for v in VARIANTS:
        ctx.set_variant(v)
        rgba, idd = ctx.dispatch(W, H, g["mode"])
        _assert_same(rgba, ref_rgba, f"{key} variant {v} rgba8")
        _assert_same(idd, ref_id, f"{key} variant {v} id/dist")
        assert "%016x" % V.fnv1a64(rgba) == g["rgba_fnv1a64"]
        assert "%016x" % V.fnv1a64(idd) == g["id_dist_fnv1a64"]
    ctx.set_variant(0)


@pytest.mark.parametrize("key", ["dragon_1080p/mode0", "dragon_1080p/mode1", "monu9_720p/mode0", "monu9_720p/mode1",
                                 "dragon_default_720p/mode0", "nature_4k/mode1", "dragon_720p_full/mode2",
                                 "dragon_1080p_full/mode2", "terrain_1080p/mode0", "terrain_1080p/mode1",
                                 "monu9_720p_full/mode2", "terrain_1080p_full/mode2", "nature_4k_full/mode2",
                                 "dragon_default_720p/mode1", "dragon_default_720p/mode2", "nature_4k/mode0",
                                 "room_inside_1080p/mode0", "room_inside_1080p/mode1", "room_inside_1080p_full/mode2",
                                 "room_inside_720p_full/mode2", "room_outside_1080p_full/mode2", "room_outside_720p_full/mode2"])
def test_full_size_frames_match_committed_hashes(ctx, V, golden, product_scenes, key):
    """BASELINE.json sizes: the oracle's frame hashes were committed by tests/golden/make_golden.py."""
    g = golden["frames"]["frames"][key]
    tex, dim = product_scenes[g["map"]]
    W, H = g["width"], g["height"]
    _setup(ctx, V, tex, dim, g["pose"], W, H)
    rgba, idd = ctx.dispatch(W, H, g["mode"])
    assert "%016x" % V.fnv1a64(rgba) == g["rgba_fnv1a64"], key
    assert "%016x" % V.fnv1a64(idd) == g["id_dist_fnv1a64"], key
    hits = int(np.count_nonzero(idd[..., 0]))
    # voxelID 0 is also a legal id for the voxel at the origin; a translucent first hit (the room's glass and jelly) counts as a
    # hit but leaves the id to the first OPAQUE surface behind it, if any (comp:539-544)
    assert hits <= g["hits"] and (g["map"] == "room" or hits >= g["hits"] - 4)
    if "shown_fnv1a64" in g:   # the frame the reference puts on screen: the display pass over the two images, three routes
        import importlib
        shd = importlib.import_module("voxel-raytracer_amd.sharding")
        assert "%016x" % V.fnv1a64(ctx.denoise(rgba, idd)) == g["shown_fnv1a64"], key + " display pass"
        assert "%016x" % V.fnv1a64(ctx.dispatch_frame(W, H, 2)[0]) == g["shown_fnv1a64"], key + " fused frame call"
        root = shd.ShownFramePipeline(ctx, W, H, 0, 4, 2, n_buf=2, group="in-process")
        ranks = [root] + [shd.ShownFramePipeline(ctx, W, H, r, 4, 2, n_buf=2, share=root) for r in range(1, 4)]
        try:
            for _ in range(3):
                for p in reversed(ranks):
                    p.step()
            assert all(p.drain(60.0) for p in ranks)
            assert "%016x" % V.fnv1a64(root.last_shown()) == g["shown_fnv1a64"], key + " four row bands with halos"
        finally:
            for p in reversed(ranks):
                p.close()


def test_degenerate_inputs(ctx, V, O, product_scenes):
    tex, dim = product_scenes["dragon"]
    # F8: camera exactly on voxel boundaries, axis-aligned middle row/column (zero-length steps until the cap)
    for pose, (W, H) in [((34.0, 60.0, 34.0, -90.0, 0.0), (64, 36)), ((20.0, 30.0, 20.0, 0.0, 0.0), (40, 40)),
                         ((63.5, 2000.0, 30.5, -90.0, -89.0), (32, 32)),   # camera outside the world (above)
                         ((-2000.5, 50.5, 30.5, 0.0, 0.0), (32, 18)),      # outside, looking in along +x
                         # outside, the first step lands outside too but within 1024 units of the eye (found by tests/fuzz/fuzz_parity.py
                         # seed 211: the v4 walk took such a point for one of wide root 0)
                         ((877.630258097967, 413.60274114898647, 1499.3121964738943, 32.390759674626054, 37.50787468408298), (47, 53)),
                         ((-919.1504641258679, -530.0652491118379, 1599.2008229520852, -90.0, -45.0), (96, 47)),
                         ((492.5792800470553, 1058.786681235461, -596.7419040459511, -180.0, 0.0), (46, 10)),
                         ((1102.7347442281894, 349.15493098196606, 58.2267500913418, 45.0, 87.46694058563853), (32, 19)),
                         ((63.5, 60.5, 140.5, -90.0, -10.0), (1, 1)), ((63.5, 60.5, 140.5, -90.0, -10.0), (13, 7))]:
        cam = _setup(ctx, V, tex, dim, pose, W, H)
        for mode in (0, 1, 2):
            ref_rgba, ref_id, _ = _oracle_frame(O, tex, dim, cam, W, H, mode)
            rgba, idd = ctx.dispatch(W, H, mode)
            _assert_same(rgba, ref_rgba, f"pose {pose} {W}x{H} mode {mode} rgba8")
            _assert_same(idd, ref_id, f"pose {pose} {W}x{H} mode {mode} id/dist")
    # empty world: every pixel is sky
    cam = _setup(ctx, V, np.zeros(0, np.uint8), 1, (10.5, 10.5, 10.5, -90.0, 0.0), 48, 24)
    ref_rgba, ref_id, _ = _oracle_frame(O, np.zeros(0, np.uint8), 1, cam, 48, 24, 1)
    rgba, idd = ctx.dispatch(48, 24, 1)
    _assert_same(rgba, ref_rgba, "empty world rgba8")
    _assert_same(idd, ref_id, "empty world id/dist")
    assert np.all(idd[..., 0] == 0) and np.all(idd[..., 1] == 2047)


def _tx(value, alpha):
    return [value & 255, (value >> 8) & 255, (value >> 16) & 255, alpha]


def test_custom_world_bounds_and_unit_internal_node(ctx, V, O):
    """Hand-written texel streams in a small world [0,8)^3 (u_worldBoundsMin/Max are uniforms):
    (a) a regular tree, (b) a tree whose unit cell [4,5)^3 is still an internal node -- never written
    by octree_texture(), outside the bit-indexed traversal's precondition, so the dispatcher must
    route it to the explicit-AABB kernels and still match the shader arithmetic."""
    leaf = [200, 40, 90, 255, 255, 0, 0, 255]
    regular = _tx(1, 0x81) + _tx(3 | 0x800000, 0) + _tx(5, 0) + leaf + _tx(6, 0x01) + _tx(7 | 0x800000, 0) + leaf
    unit = (_tx(1, 0x80) + _tx(2, 0) + _tx(3, 0x01) + _tx(4, 0) + _tx(5, 0x01) + _tx(6, 0) + _tx(7, 0x80) +
            _tx(8 | 0x800000, 0) + leaf)
    for name, stream in (("regular", regular), ("unit-internal", unit)):
        tex = np.array(stream, np.uint8)
        W, H = 64, 48
        ip, iv, cp, _ = V.camera_block((1.3, 2.1, 0.7), 52.0, 18.0, W, H)
        ctx.upload_octree(tex, 3)
        ctx.set_camera(ip, iv, cp)
        p = ctx.default_params()
        p.world_min[:] = (0, 0, 0)
        p.world_max[:] = (8, 8, 8)
        ctx.set_params(p)
        s = O.make_scene(tex, 3, ip, iv, cp)
        s.bounds_min[:] = (0, 0, 0)
        s.bounds_max[:] = (8, 8, 8)
        for mode in (0, 1, 2):
            ref_rgba, ref_id, _, st = O.render(s, W, H, mode)
            assert st["hits"] > 20, name
            for v in [v for v in (0, 1, 2, 13, 15, 20) if v in VARIANTS]:
                ctx.set_variant(v)
                rgba, idd = ctx.dispatch(W, H, mode)
                _assert_same(rgba, ref_rgba, f"{name} mode {mode} variant {v} rgba8")
                _assert_same(idd, ref_id, f"{name} mode {mode} variant {v} id/dist")
    ctx.set_variant(0)
    ctx.set_params(ctx.default_params())


def test_world_with_eight_wide_roots_and_a_refused_one(ctx, V, O):
    """World [-256,256)^3 (side 2^9): the eight octants are separate wide roots and rays cross between them.
    World [-64,192)^3: too many aligned sub-trees for the root table -> the dispatcher must fall back, silently exact."""
    from conftest import random_voxels
    rng = np.random.default_rng(4)
    xyz, rgba = random_voxels(rng, 5000, -60, 70)
    for wmin, wmax in [((-256,) * 3, (256,) * 3), ((-64,) * 3, (192,) * 3)]:
        w = V.World(world_min=wmin, world_max=wmax)
        w.insert_many(xyz, rgba)
        tex, dim = w.flatten()
        W, H = 128, 80
        ip, iv, cp, _ = V.camera_block((100.5, 90.5, 120.5), -130.0, -30.0, W, H)
        ctx.upload_octree(tex, dim)
        ctx.set_camera(ip, iv, cp)
        p = ctx.default_params()
        p.world_min[:] = wmin
        p.world_max[:] = wmax
        ctx.set_params(p)
        s = O.make_scene(tex, dim, ip, iv, cp)
        s.bounds_min[:] = wmin
        s.bounds_max[:] = wmax
        for mode in (0, 1, 2):
            ref_rgba, ref_id, _, st = O.render(s, W, H, mode)
            assert st["hits"] > 500
            for v in [v for v in (0, 1, 4, 13, 20) if v in VARIANTS]:
                ctx.set_variant(v)
                rgba_, idd = ctx.dispatch(W, H, mode)
                _assert_same(rgba_, ref_rgba, f"world {wmin} mode {mode} variant {v} rgba8")
                _assert_same(idd, ref_id, f"world {wmin} mode {mode} variant {v} id/dist")
    ctx.set_variant(0)
    ctx.set_params(ctx.default_params())


def test_procedural_terrain_config4(ctx, V, O, golden, product_scenes):
    """BASELINE config 4: the reference's terrain generator (src/main.cpp:487-503) over the height field its own
    FastNoiseLite.h produces (tests/golden/terrain.json; 7.6 M texels, close to the 2^23 pointer limit), small frame
    against the live oracle; the 1920x1080 frames are in test_full_size_frames_match_committed_hashes."""
    tex, dim = product_scenes["terrain"]
    t = golden["terrain"]
    assert tex.size // 4 == t["texels"] and dim == t["tex_dim"] and "%016x" % V.fnv1a64(tex) == t["fnv1a64"]
    assert 4_000_000 < tex.size // 4 < 2 ** 23
    W, H = 240, 136
    cam = _setup(ctx, V, tex, dim, t["pose"], W, H)
    for mode in (0, 1, 2):
        ref_rgba, ref_id, st = _oracle_frame(O, tex, dim, cam, W, H, mode)
        g = golden["frames"]["frames"][f"terrain_240x136/mode{mode}"]
        assert "%016x" % O.fnv1a64(ref_rgba) == g["rgba_fnv1a64"] and "%016x" % O.fnv1a64(ref_id) == g["id_dist_fnv1a64"]
        assert st["hits"] > 0.3 * W * H
        for v in (0, 1, 4, 20):
            ctx.set_variant(v)
            rgba, idd = ctx.dispatch(W, H, mode)
            _assert_same(rgba, ref_rgba, f"terrain mode {mode} variant {v} rgba8")
            _assert_same(idd, ref_id, f"terrain mode {mode} variant {v} id/dist")
    ctx.set_variant(0)
    # the texel limit itself is enforced
    with pytest.raises(V.VrtError, match="2\\^23"):
        ctx.upload_octree(np.zeros(4 * (2 ** 23 + 1), np.uint8), 204)


def test_terrain_config4_at_its_full_extent_through_records(ctx, V, golden):
    """BASELINE config 4 as named: the WHOLE 1024 x 1024 height field (24.07 M texels' worth, 8.5 M records) -- beyond what
    the reference's 23-bit pointer texels address, so the product takes it as records (vrth_world_records ->
    vrt_upload_records) and the oracle read it through its wide-pointer stream extension (tests/golden/make_golden.py,
    oracle.h); the frames must equal the oracle's committed hashes in all three modes, and the displayed frame too."""
    from conftest import terrain_world
    w = terrain_world(V, {"x0": 0, "z0": 0, "nx": 1024, "nz": 1024})
    assert w.texel_count() == 24071648 and w.texel_count() > 2 ** 23
    rec, dim = w.records()
    w.close()
    assert dim == 289
    ctx.set_params(ctx.default_params())
    ctx.upload_records(rec, dim)
    frames = golden["frames"]["frames"]
    for key in ("terrain_full_240x136/mode0", "terrain_full_240x136/mode1", "terrain_full_240x136/mode2",
                "terrain_full_1080p/mode0", "terrain_full_1080p/mode1", "terrain_full_1080p_full/mode2"):
        g = frames[key]
        W, H = g["width"], g["height"]
        ip, iv, cp, _ = V.camera_block(g["pose"][:3], g["pose"][3], g["pose"][4], W, H)
        ctx.set_camera(ip, iv, cp)
        for v in ((0, 1, 4, 20) if W < 1000 else (0,)):
            ctx.set_variant(v)
            rgba, idd = ctx.dispatch(W, H, g["mode"])
            assert "%016x" % V.fnv1a64(rgba) == g["rgba_fnv1a64"], (key, v)
            assert "%016x" % V.fnv1a64(idd) == g["id_dist_fnv1a64"], (key, v)
        ctx.set_variant(0)
        if "shown_fnv1a64" in g:
            assert "%016x" % V.fnv1a64(ctx.denoise(rgba, idd)) == g["shown_fnv1a64"], key + " display pass"
    assert ctx.scene_info()["n_records"] == rec.shape[0]


def test_denoise_pass_matches_quad_frag_restatement(ctx, V, O, product_scenes):
    """shaders/quad.frag (ID-aware box blur, up to 41x41 taps) on the outputs of the full path tracer."""
    for name, pose, (W, H) in [("dragon", (63.5, 60.5, 140.5, -90.0, -10.0), (256, 144)),
                                ("dragon", (60.3, 64.7, 75.2, -100.0, -25.0), (200, 120)),    # close-up: radius 20
                                ("nature", (60.5, 80.5, 330.5, -90.0, -12.0), (177, 99)),     # far: smaller radii, ragged size
                                ("monu9", (48.5, 60.5, 170.5, -90.0, -12.0), (64, 64))]:
        tex, dim = product_scenes[name]
        _setup(ctx, V, tex, dim, pose, W, H)
        rgba, idd = ctx.dispatch(W, H, 2)
        ref = O.denoise(rgba, idd)
        for dv in DISPLAY_KERNELS:                                                          # one, two pixels per lane
            ctx.set_denoise_variant(dv)
            got = ctx.denoise(rgba, idd)
            _assert_same(got, ref, f"denoise {name} {W}x{H} kernel {dv}")
        assert np.array_equal(got[idd[..., 0] == 0], rgba[idd[..., 0] == 0])      # sky passes through
        if name == "dragon":
            assert np.any(got != rgba)                                             # and it did blur something
    # synthetic ids: negative ids, id present only at the centre, every distance class
    rng = np.random.default_rng(9)
    W, H = 150, 90
    rgba = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    idd = np.zeros((H, W, 2), np.int32)
    idd[..., 0] = rng.integers(-3, 4, size=(H, W))
    idd[..., 1] = rng.choice([0, 1, 2, 50, 99, 100, 101, 400, 2047, 40000], size=(H, W))
    ref = O.denoise(rgba, idd)
    for dv in DISPLAY_KERNELS:
        ctx.set_denoise_variant(dv)
        _assert_same(ctx.denoise(rgba, idd), ref, f"denoise synthetic kernel {dv}")
    # the per-id row / column table of the tile (IdRows, 128 slots): every pixel its own id (the table overflows: whole windows),
    # ~100 ids per tile (long probe chains), ids that all hash to ONE slot, an id whose pixels lie far apart inside a window (the
    # walked rows and column segments are the union), ids that appear only in a tile's halo
    # (twice: a width that is not a multiple of four stages tap by tap, one that is stages four taps per 16-byte load)
    for (W, H) in [(131, 83), (132, 84)]:
        yy, xx = np.mgrid[0:H, 0:W]
        slot = lambda v: ((int(v) * 2654435761) & 0xffffffff) >> 25
        same_slot = [v for v in range(1, 400000) if slot(v) == 5][:40]
        fields = [1 + yy * W + xx, 1 + (yy // 2) * 16 + (xx // 3) % 16 + 1000 * (xx // 48), np.array(same_slot)[(yy // 4 * 7 + xx // 5) % 40],
                  np.where((xx % 37 < 2) | (yy % 29 < 2), 9, 1 + (xx // 9 + 11 * (yy // 7)) % 60), np.where(xx % 32 < 20, 0, 3 + yy // 6)]
        for k, ids in enumerate(fields):
            rgba = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
            idd = np.zeros((H, W, 2), np.int32)
            idd[..., 0] = ids
            idd[..., 1] = rng.choice([60, 100, 120, 400], size=(H, W)) if k % 2 else 100
            ref = O.denoise(rgba, idd)
            for dv in DISPLAY_KERNELS:
                ctx.set_denoise_variant(dv)
                _assert_same(ctx.denoise(rgba, idd), ref, f"denoise id table case {k} kernel {dv}")
    # radii that differ by one or by many inside a wave, image sizes off the 32 x 16 tile, one object id everywhere
    for (W, H) in [(67, 35), (130, 50), (128, 48)]:
        rgba = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
        idd = np.zeros((H, W, 2), np.int32)
        idd[..., 0] = 7
        idd[H // 3, W // 2, 0] = 0
        yy, xx = np.mgrid[0:H, 0:W]
        for dist in (100 + (xx + yy) // 3, 100 + 60 * ((xx // 5 + yy // 3) % 4), 90 + (xx * 37 + yy * 11) % 400):
            idd[..., 1] = dist
            ref = O.denoise(rgba, idd)
            for dv in DISPLAY_KERNELS:
                ctx.set_denoise_variant(dv)
                _assert_same(ctx.denoise(rgba, idd), ref, f"denoise radii {W}x{H} kernel {dv}")


def test_display_pass_with_feedback_scheduling(V, O, product_scenes):
    """The display pass under vrt_set_tile_scheduling (its tiles start heaviest first, from measured tile times): frames
    big enough to be scheduled, the order re-derived every one or two launches and gone stale when the image changes,
    a tile count that is no multiple of the group size. One frame against the oracle's quad.frag restatement, the
    others against the unscheduled pass (which the small-frame test above ties to the oracle)."""
    c = V.Context(0)
    try:
        tex, dim = product_scenes["dragon"]
        c.upload_octree(tex, dim)
        frames = []
        for (W, H), pose in [((1056, 544), (63.5, 60.5, 140.5, -90.0, -10.0)), ((1056, 544), (60.3, 64.7, 75.2, -100.0, -25.0)),
                             ((1920, 1080), (63.5, 60.5, 140.5, -90.0, -10.0))]:
            ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
            c.set_camera(ip, iv, cp)
            c.set_tile_scheduling(0)
            rgba, idd = c.dispatch(W, H, 2)
            frames.append((rgba, idd, c.denoise(rgba, idd)))
        _assert_same(frames[0][2], O.denoise(frames[0][0], frames[0][1]), "unscheduled display pass 1056x544 vs oracle")
        for period in (1, 2):
            c.set_tile_scheduling(period)
            for k in range(9):
                rgba, idd, ref = frames[(k // 2) % 2]          # same shape, the image changes every other call
                _assert_same(c.denoise(rgba, idd), ref, f"scheduled display pass period {period} call {k}")
            for k in range(3):
                _assert_same(c.denoise(frames[2][0], frames[2][1]), frames[2][2], f"scheduled display pass 1080p period {period} call {k}")
        # the fused frame call (trace + display pass on the context's stream, both scheduled)
        pose = (63.5, 60.5, 140.5, -90.0, -10.0)
        ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], 1920, 1080)
        c.set_camera(ip, iv, cp)
        for k in range(4):
            shown, rgba, idd = c.dispatch_frame(1920, 1080, 2)
            _assert_same(rgba, frames[2][0], f"fused frame {k} rgba8")
            _assert_same(shown, frames[2][2], f"fused frame {k} displayed")
    finally:
        c.close()


def test_record_upload_extension(ctx, V, O, product_scenes):
    """vrt_upload_records: same pixels as the texel path; and a scene beyond the stream's 2^23-texel limit, which
    the texel path must refuse, renders identically under the three traversals (no oracle exists for it)."""
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    rec, dim = w.records()
    tex, dim2 = product_scenes["dragon"]
    W, H = 200, 120
    ip, iv, cp, _ = V.camera_block((63.5, 60.5, 140.5), -90.0, -10.0, W, H)
    ctx.set_params(ctx.default_params())
    ctx.set_camera(ip, iv, cp)
    ctx.upload_octree(tex, dim2)
    ref = [ctx.dispatch(W, H, m) for m in (0, 1, 2)]
    ctx.upload_records(rec, dim)
    for m in (0, 1, 2):
        rgba, idd = ctx.dispatch(W, H, m)
        _assert_same(rgba, ref[m][0], f"records path mode {m} rgba8")
        _assert_same(idd, ref[m][1], f"records path mode {m} id/dist")
    with pytest.raises(V.VrtError, match="out of order|two parents"):
        bad = rec.copy()
        bad[0, 1] = 0  # root's children would start at the root itself
        ctx.upload_records(bad, dim)
    # 176^3 three-dimensional checkerboard: nothing merges, ~9.4 M texels
    n = 176
    g = np.indices((n, n, n)).reshape(3, -1).T
    g = g[(g.sum(axis=1) & 1) == 0].astype(np.int32)
    big = V.World()
    big.insert_many(g, np.where((g[:, 0] // 8 + g[:, 2] // 8) & 1, 0xc86432ff, 0x3296c8ff).astype(np.uint32))
    assert big.texel_count() > 2 ** 23
    rec, dim = big.records()
    btex, bdim = big.flatten()
    with pytest.raises(V.VrtError, match="2\\^23"):
        ctx.upload_octree(btex, bdim)
    ctx.upload_records(rec, dim)
    ip, iv, cp, _ = V.camera_block((300.5, 260.5, 330.5), -130.0, -30.0, W, H)
    ctx.set_camera(ip, iv, cp)
    for m in (0, 1):
        frames = []
        for v in (0, 1, 4, 20):
            ctx.set_variant(v)
            frames.append(ctx.dispatch(W, H, m))
        assert np.count_nonzero(frames[0][1][..., 0]) > 0.2 * W * H
        for k in (1, 2):
            _assert_same(frames[k][0], frames[0][0], f"big scene mode {m} traversal {k} rgba8")
            _assert_same(frames[k][1], frames[0][1], f"big scene mode {m} traversal {k} id/dist")
    ctx.set_variant(0)


def test_materials_highlight_and_translucent_fallback(ctx, V, O):
    """Emissive, translucent and highlighted voxels + a camera sitting inside a translucent medium."""
    w = V.World()
    rng = np.random.default_rng(5)
    for x in range(0, 24):
        for z in range(0, 24):
            w.insert(x, 0, z, 0xa0a0a0ff)                       # stone floor
    for _ in range(200):
        x, y, z = (int(v) for v in rng.integers(2, 22, size=3))
        kind = rng.integers(0, 4)
        if kind == 0:
            w.insert(x, y, z, 0xffd2d2ff, 3.0, 1.0, 0.0)        # light
        elif kind == 1:
            w.insert(x, y, z, 0x3c64dc96, 1.33, 0.0, 0.0)       # water (alpha 150)
        elif kind == 2:
            w.insert(x, y, z, 0xc8dcff50, 1.5, 0.0, 0.0)        # glass
        else:
            w.insert(x, y, z, 0x50b43cff)                       # grass
    for x in range(30, 36):
        for y in range(2, 8):
            for z in range(8, 14):
                w.insert(x, y, z, 0x3c64dc96, 1.33, 0.0, 0.0)   # a block of water to put the camera in
    for x in range(44, 50):
        for y in range(2, 8):
            for z in range(8, 14):
                w.insert(x, y, z, 0x3c64dc00, 1.33, 0.0, 0.0)   # alpha 0 but refraction 1.33: only startIOF sees it
    w.insert(10, 1, 10, 0x11223300, 2.0, 1.0, 0.5)               # a lone alpha-0 voxel with every property set
    tex, dim = w.flatten()
    for pose, hl in [((12.3, 14.2, 40.7, -90.0, -15.0), (-1, -1, -1)), ((12.3, 14.2, 40.7, -90.0, -15.0), (5, 0, 20)),
                     ((32.5, 4.5, 10.5, 180.0, 5.0), (-1, -1, -1)), ((46.5, 4.5, 10.5, 180.0, 5.0), (-1, -1, -1))]:
        W, H = 96, 64
        cam = _setup(ctx, V, tex, dim, pose, W, H, highlighted=hl)
        for mode in (0, 1, 2):
            ref_rgba, ref_id, _ = _oracle_frame(O, tex, dim, cam, W, H, mode, highlighted=hl)
            rgba, idd = ctx.dispatch(W, H, mode)
            _assert_same(rgba, ref_rgba, f"materials pose {pose} hl {hl} mode {mode} rgba8")
            _assert_same(idd, ref_id, f"materials pose {pose} hl {hl} mode {mode} id/dist")


def test_full_path_tracer_without_a_stack_for_opaque_scenes(V, O, golden, product_scenes):
    """VRT_OPT_FULL_OPAQUE: for a scene without translucent voxels seen from empty space VRT_MODE_FULL runs its two stages -- primary +
    shadow, then the one diffuse bounce -- without the ray stack: in one kernel (values 5, 6, 7; 6 is the default) or as two kernels
    with a 20-byte seed per pixel between them (value 1); 0 is the general kernel. Every frame must equal the oracle's -- whole
    frames, compact row shards with ragged tile counts, the three scheduling flavours, a highlighted voxel, emissive surfaces, two
    streams at once. Scenes with translucent voxels and eyes inside a medium take the general kernel whatever the option says
    (and must still match)."""
    import torch
    c = V.Context(0)
    c.set_option(V.OPT_FULL_OPAQUE, 1)
    try:
        # the general kernel (0) and the one-kernel forms (5, 6, 7: waves per SIMD it is built for)
        for form in (0, 5, 6, 7):
            c.set_option(V.OPT_FULL_OPAQUE, form)
            for name, key in (("dragon", "dragon_256x144/mode2"), ("nature", "nature_200x112/mode2"), ("dragon", "dragon_default_720p/mode2"),
                              ("room", "room_outside_256x144/mode2"), ("dragon", "dragon_1080p_full/mode2")):
                g = golden["frames"]["frames"][key]
                tex, dim = product_scenes[name]
                W, H = g["width"], g["height"]
                _setup(c, V, tex, dim, g["pose"], W, H)
                for _ in range(3):
                    rgba, idd = c.dispatch(W, H, 2)
                    assert "%016x" % V.fnv1a64(rgba) == g["rgba_fnv1a64"], (form, key)
                    assert "%016x" % V.fnv1a64(idd) == g["id_dist_fnv1a64"], (form, key)
        c.set_option(V.OPT_FULL_OPAQUE, 1)
        for name, key in (("dragon", "dragon_256x144/mode2"), ("monu9", "monu9_192x108/mode2"), ("nature", "nature_200x112/mode2"),
                          ("terrain", "terrain_240x136/mode2"), ("dragon", "dragon_inside_101x67/mode2"), ("room", "room_inside_256x144/mode2"),
                          ("dragon", "dragon_1080p_full/mode2"), ("nature", "nature_4k_full/mode2"), ("dragon", "dragon_default_720p/mode2")):
            g = golden["frames"]["frames"][key]
            tex, dim = product_scenes[name]
            W, H = g["width"], g["height"]
            _setup(c, V, tex, dim, g["pose"], W, H)
            for _ in range(3):   # plain, measuring, ordered launches of the shape
                rgba, idd = c.dispatch(W, H, 2)
                assert "%016x" % V.fnv1a64(rgba) == g["rgba_fnv1a64"], key
                assert "%016x" % V.fnv1a64(idd) == g["id_dist_fnv1a64"], key
            if "shown_fnv1a64" in g:
                assert "%016x" % V.fnv1a64(c.dispatch_frame(W, H, 2)[0]) == g["shown_fnv1a64"], key
        # a highlighted voxel on the surface, and one that only a bounce ray meets
        tex, dim = product_scenes["dragon"]
        W, H = 160, 90
        for hl in ((63, 45, 28), (70, 30, 30), (40, 20, 25)):
            cam = _setup(c, V, tex, dim, (63.5, 60.5, 140.5, -90.0, -10.0), W, H, highlighted=hl)
            ref_rgba, ref_id, _ = _oracle_frame(O, tex, dim, cam, W, H, 2, highlighted=hl)
            rgba, idd = c.dispatch(W, H, 2)
            _assert_same(rgba, ref_rgba, f"two-pass highlighted {hl} rgba8")
            _assert_same(idd, ref_id, f"two-pass highlighted {hl} id/dist")
        # emissive and opaque voxels only (two passes), then the same world with one glass voxel (one kernel): both vs the oracle
        rng = np.random.default_rng(21)
        w = V.World()
        for x in range(0, 32):
            for z in range(0, 32):
                w.insert(x, 0, z, 0xa0a0a0ff)
        for _ in range(300):
            x, y, z = (int(v) for v in rng.integers(1, 30, size=3))
            if rng.integers(0, 3) == 0:
                w.insert(x, y, z, 0xffd2d2ff, 3.0, 1.0, 0.0)
            else:
                w.insert(x, y, z, 0x50b43cff if y & 1 else 0x644628ff, 2.0 if x & 1 else 3.0, 0.0, 0.3)
        for glass in (False, True):
            if glass:
                w.insert(15, 6, 15, 0xc8dcff50, 1.5, 0.0, 0.0)
            tex, dim = w.flatten()
            for pose in ((16.3, 22.2, 60.7, -90.0, -20.0), (2.5, 9.5, 2.5, 45.0, -10.0), (16.0, 10.0, 16.0, 0.0, 0.0)):
                cam = _setup(c, V, tex, dim, pose, 96, 64)
                ref_rgba, ref_id, _ = _oracle_frame(O, tex, dim, cam, 96, 64, 2)
                rgba, idd = c.dispatch(96, 64, 2)
                _assert_same(rgba, ref_rgba, f"two-pass emissive world glass={glass} pose {pose} rgba8")
                _assert_same(idd, ref_id, f"two-pass emissive world glass={glass} pose {pose} id/dist")
        # compact row shards with ragged tile counts, on two streams at once
        tex, dim = product_scenes["monu9"]
        W, H = 203, 117
        cam = _setup(c, V, tex, dim, (48.5, 60.5, 170.5, -90.0, -12.0), W, H)
        ref_rgba, ref_id, _ = _oracle_frame(O, tex, dim, cam, W, H, 2)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for n_shards in (2, 3):
            bufs = []
            for s_ in range(n_shards):
                rows = V.shard_rows(H, 5, s_, n_shards)
                bufs.append((torch.zeros(rows * W, dtype=torch.int32, device="cuda"), torch.zeros(rows * W * 2, dtype=torch.int32, device="cuda")))
            torch.cuda.synchronize()   # the zero fills run on the default stream: done before the side streams write
            for s_ in range(n_shards):
                c.dispatch_shard(W, H, 5, s_, n_shards, 2, bufs[s_][0].data_ptr(), bufs[s_][1].data_ptr(), streams[s_ & 1].cuda_stream)
            torch.cuda.synchronize()
            for s_ in range(n_shards):
                rows = V.shard_row_indices(H, 5, s_, n_shards)
                assert np.array_equal(bufs[s_][0].cpu().numpy().view(np.uint8).reshape(-1, W, 4), ref_rgba[rows]), (n_shards, s_)
                assert np.array_equal(bufs[s_][1].cpu().numpy().reshape(-1, W, 2), ref_id[rows]), (n_shards, s_)
    finally:
        c.close()


def test_row_sharding_properties_at_full_size(ctx, V, golden, product_scenes):
    """N-shard result == 1-GPU result byte for byte (virtual shards on one device), at 1920x1080."""
    import torch
    g = golden["frames"]["frames"]["dragon_1080p/mode1"]
    tex, dim = product_scenes["dragon"]
    W, H = g["width"], g["height"]
    _setup(ctx, V, tex, dim, g["pose"], W, H)
    full_rgba, full_id = ctx.dispatch(W, H, 1)
    assert "%016x" % V.fnv1a64(full_rgba) == g["rgba_fnv1a64"]
    dev = torch.device("cuda:0")
    # contiguous row blocks written in place
    d_rgba = torch.zeros((H, W), dtype=torch.int32, device=dev)
    d_id = torch.zeros((H, W, 2), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # the fills run on torch's stream, the dispatch on the context's own
    for r0, r1 in [(0, 135), (135, 541), (541, 1079), (1079, 1080)]:
        ctx.dispatch_rows(W, H, r0, r1, 1, d_rgba.data_ptr(), d_id.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_rgba.cpu().numpy().view(np.uint8).reshape(H, W, 4), full_rgba)
    assert np.array_equal(d_id.cpu().numpy(), full_id)
    # interleaved 8-row tiles, compact shard buffers, 8 shards (and a ragged 3-shard / 5-row-tile split)
    for tile_rows, n_shards in [(8, 8), (5, 3), (1080, 2)]:
        out_rgba = np.zeros_like(full_rgba)
        out_id = np.zeros_like(full_id)
        for s in range(n_shards):
            rows = V.shard_row_indices(H, tile_rows, s, n_shards)
            assert len(rows) == V.shard_rows(H, tile_rows, s, n_shards)
            if not rows:
                continue
            sr = torch.zeros((len(rows), W), dtype=torch.int32, device=dev)
            si = torch.zeros((len(rows), W, 2), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()  # the fills run on torch's stream, the dispatch on the context's own
            ctx.dispatch_shard(W, H, tile_rows, s, n_shards, 1, sr.data_ptr(), si.data_ptr())
            ctx.synchronize()
            out_rgba[rows] = sr.cpu().numpy().view(np.uint8).reshape(len(rows), W, 4)
            out_id[rows] = si.cpu().numpy()
        assert np.array_equal(out_rgba, full_rgba) and np.array_equal(out_id, full_id), (tile_rows, n_shards)
    # idempotence: a second dispatch of the same frame is identical
    again_rgba, again_id = ctx.dispatch(W, H, 1)
    assert np.array_equal(again_rgba, full_rgba) and np.array_equal(again_id, full_id)


def test_async_host_dispatch_into_pinned_buffers(ctx, V, golden, product_scenes):
    """vrt_dispatch_async / vrt_dispatch_wait: two frames in flight, page-locked host buffers, tickets; frames of different
    cameras must not mix, a third call must wait for the oldest ticket by itself, pageable buffers work too."""
    g = golden["frames"]["frames"]["dragon_256x144/mode1"]
    tex, dim = product_scenes["dragon"]
    W, H = g["width"], g["height"]
    cam_a = _setup(ctx, V, tex, dim, g["pose"], W, H)
    want_a = ctx.dispatch(W, H, 1)
    pose_b = (60.3, 70.7, 120.2, -80.0, -15.0)
    cam_b = V.camera_block(pose_b[:3], pose_b[3], pose_b[4], W, H)[:3]
    ctx.set_camera(*cam_b)
    want_b = ctx.dispatch(W, H, 1)
    assert "%016x" % V.fnv1a64(want_a[0]) == g["rgba_fnv1a64"] and not np.array_equal(want_a[0], want_b[0])
    bufs = [(ctx.host_alloc((H, W, 4), np.uint8), ctx.host_alloc((H, W, 2), np.int32)) for _ in range(2)]
    try:
        for rep in range(5):   # A into lane 0, B into lane 1, alternating; the third call reuses lane 0 and must wait for it
            ctx.set_camera(*cam_a)
            t0 = ctx.dispatch_async(W, H, 1, *bufs[0])
            ctx.set_camera(*cam_b)
            t1 = ctx.dispatch_async(W, H, 1, *bufs[1])
            assert {t0, t1} == {0, 1}
            ctx.dispatch_wait(t0)
            _assert_same(bufs[0][0], want_a[0], "async lane A rgba8")
            _assert_same(bufs[0][1], want_a[1], "async lane A id/dist")
            ctx.dispatch_wait(t1)
            _assert_same(bufs[1][0], want_b[0], "async lane B rgba8")
            _assert_same(bufs[1][1], want_b[1], "async lane B id/dist")
        pageable = np.zeros((H, W, 4), np.uint8)
        t = ctx.dispatch_async(W, H, 1, pageable, None)
        ctx.dispatch_wait(t)
        ctx.dispatch_wait(t)   # idempotent
        _assert_same(pageable, want_b[0], "async into pageable memory")
    finally:
        for a_, b_ in bufs:
            ctx.host_free(a_)
            ctx.host_free(b_)


def test_tiles_into_one_frame_ipc_and_flags(ctx, V, golden, product_scenes):
    """vrt_dispatch_tiles: the shards of a frame written at their place in ONE full frame (what a peer GPU does through an
    xGMI mapping); device memory exported to another process and stored into from there (the one-process-per-GPU form:
    here both processes sit on the one GPU of the box); stream-ordered flags."""
    import subprocess
    import sys
    import textwrap
    from conftest import ROOT
    g = golden["frames"]["frames"]["dragon_256x144/mode1"]
    tex, dim = product_scenes["dragon"]
    W, H = g["width"], g["height"]
    _setup(ctx, V, tex, dim, g["pose"], W, H)
    want_rgba, want_id = ctx.dispatch(W, H, 1)
    assert "%016x" % V.fnv1a64(want_rgba) == g["rgba_fnv1a64"]
    d_rgba, d_id, d_flag = ctx.device_alloc(W * H * 4), ctx.device_alloc(W * H * 8), ctx.device_alloc(256)
    try:
        for tile_rows, n_shards in ((8, 3), (5, 4), (H, 2)):
            ctx.device_write(d_rgba, np.zeros(W * H, np.uint32))
            ctx.device_write(d_id, np.zeros(2 * W * H, np.int32))
            for s_ in range(n_shards):
                ctx.dispatch_tiles(W, H, tile_rows, s_, n_shards, 1, d_rgba, d_id)
            _assert_same(ctx.device_read(d_rgba, (H, W, 4), np.uint8), want_rgba, f"tiles {tile_rows}/{n_shards} rgba8")
            _assert_same(ctx.device_read(d_id, (H, W, 2), np.int32), want_id, f"tiles {tile_rows}/{n_shards} id/dist")
        # flags: a wait for a value the same stream wrote before it passes; values are kept
        ctx.stream_write_flag(d_flag, 7)
        ctx.stream_wait_flag(d_flag, 7)
        ctx.stream_wait_flag(d_flag, 3)
        ctx.synchronize()
        assert int(ctx.device_read(d_flag, (1,), np.uint32)[0]) == 7
        # another process maps the frame and traces the odd shards into it, then raises the flag
        ctx.device_write(d_rgba, np.zeros(W * H, np.uint32))
        ctx.device_write(d_id, np.zeros(2 * W * H, np.int32))
        ctx.device_write(d_flag, np.zeros(1, np.uint32))
        handles = [ctx.ipc_export(p).hex() for p in (d_rgba, d_id, d_flag)]
        child = textwrap.dedent(f"""
            import os, sys
            sys.path.insert(0, {ROOT!r})
            import numpy as np
            import vrt_import
            V = vrt_import.vrt()
            w = V.World(); assert w.load_vox(os.path.join({ROOT!r}, "tests/golden/maps/dragon.vox"))
            tex, dim = w.flatten()
            c = V.Context(0)
            c.upload_octree(tex, dim)
            ip, iv, cp, _ = V.camera_block({tuple(g["pose"][:3])!r}, {g["pose"][3]!r}, {g["pose"][4]!r}, {W}, {H})
            c.set_camera(ip, iv, cp)
            ptrs = [c.ipc_open(bytes.fromhex(h)) for h in {handles!r}]
            c.dispatch_tiles({W}, {H}, 8, 1, 2, 1, ptrs[0], ptrs[1])
            c.stream_write_flag(ptrs[2], 41)
            c.synchronize()
            for p in ptrs: c.ipc_close(p)
            c.close()
            print("child ok")
        """)
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        ctx.dispatch_tiles(W, H, 8, 0, 2, 1, d_rgba, d_id)     # this process: the even tiles
        ctx.synchronize()
        r = subprocess.run([sys.executable, "-c", child], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
        ctx.stream_wait_flag(d_flag, 41)
        _assert_same(ctx.device_read(d_rgba, (H, W, 4), np.uint8), want_rgba, "two processes, one frame: rgba8")
        _assert_same(ctx.device_read(d_id, (H, W, 2), np.int32), want_id, "two processes, one frame: id/dist")
    finally:
        for p in (d_rgba, d_id, d_flag):
            ctx.device_free(p)


def test_multi_gpu_boundary_rehearsed_on_one_device(V, golden, product_scenes):
    """vrt_create_multi / vrt_multi_dispatch (include/vrt.h): one context per listed device, the frame assembled on the
    first. The box has one GPU, so the device is listed one, two and three times: every context then shares device 0, which
    exercises everything but the xGMI hop itself (peer enabling is skipped for a repeated device)."""
    tex, dim = product_scenes["dragon"]
    for key in ("dragon_256x144/mode1", "dragon_256x144/mode2"):
        g = golden["frames"]["frames"][key]
        W, H = g["width"], g["height"]
        ip, iv, cp, _ = V.camera_block(g["pose"][:3], g["pose"][3], g["pose"][4], W, H)
        for devices in ([0], [0, 0], [0, 0, 0]):
            m = V.Multi(devices)
            try:
                m.upload_octree(tex, dim)
                m.set_camera(ip, iv, cp)
                d_rgba, d_id = m.frame_alloc(W, H)
                c0 = m.context(0)
                for delivery in (V.DELIVER_PEER_STORE, V.DELIVER_GATHER):
                    for tile_rows in (8, 5):
                        c0.device_write(d_rgba, np.zeros(W * H, np.uint32), m.stream())
                        for _ in range(3):   # back to back: the next frame's traces must wait for the previous frame's consumers
                            m.dispatch(W, H, tile_rows, g["mode"], delivery, d_rgba, d_id)
                        rgba = c0.device_read(d_rgba, (H, W, 4), np.uint8, m.stream())
                        idd = c0.device_read(d_id, (H, W, 2), np.int32, m.stream())
                        assert "%016x" % V.fnv1a64(rgba) == g["rgba_fnv1a64"], (key, devices, delivery, tile_rows)
                        assert "%016x" % V.fnv1a64(idd) == g["id_dist_fnv1a64"], (key, devices, delivery, tile_rows)
                if key.endswith("mode2"):
                    # vrt_multi_dispatch_frame: the DISPLAYED frame (trace + display pass in one row band per device, 20-row
                    # halos) against the single-context route dispatch -> vrt_denoise, which other tests tie to the oracle
                    ref_rgba, ref_id = c0.dispatch(W, H, 2)
                    want = c0.denoise(ref_rgba, ref_id)
                    for _ in range(3):
                        m.dispatch_frame(W, H, 2, d_rgba)
                    shown = c0.device_read(d_rgba, (H, W, 4), np.uint8, m.stream())
                    _assert_same(shown, want, f"vrt_multi_dispatch_frame over {len(devices)} device entries")
                m.synchronize()
                m.frame_free(d_rgba, d_id)
            finally:
                m.close()
    with pytest.raises(V.VrtError):
        V.Multi([0, 99])


def test_order_kernel_sorts_groups_and_counts_the_heavy_ones(V):
    """tile_order_kernel on synthetic ticks (test-support probe): the order is a permutation with the groups' maxima never rising along
    it beyond one of its 256 buckets, and the split count behind it is the number of groups above 3/4 of the heaviest (at most 64) -- only when the heaviest tile outlasts 3/4 of its even share of all ticks over the wave slots."""
    rng = np.random.default_rng(5)
    n = 2040
    def run(ticks, slots):
        order, split = V.test_tile_order(ticks, slots)
        assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32))
        gmax = ticks.reshape(n, 4).max(1).astype(np.int64)
        top = int(gmax.max())
        if top:
            shift = max(0, top.bit_length() - 8)
            b = gmax[order] >> shift
            assert np.all(b[:-1] >= b[1:])                       # heaviest bucket first
        return order, split, gmax
    light = rng.integers(1000, 3000, size=(n, 4)).astype(np.uint32)
    # ten heavy groups in a light frame on few slots' worth of work: a frame bound by its longest wave
    t = light.copy(); heavy = rng.choice(n, 10, replace=False); t[heavy, rng.integers(0, 4, 10)] = rng.integers(90000, 100000, 10)
    order, split, gmax = run(t, 5120)
    assert split == 10 and set(order[:10].tolist()) == set(heavy.tolist())
    # the same frame when the heaviest tile is short against its even share (many more ticks per slot): no split
    assert run(t, 16)[1] == 0
    # 100 heavy groups: the limit of 64 (the heaviest come first in the order)
    t = light.copy(); t[rng.choice(n, 100, replace=False), 0] = 99000
    assert run(t, 5120)[1] == 64
    # exactly at the bucket rule: groups in the buckets from 3/4 of the heaviest bucket up count, others do not
    t = light.copy(); t[5, 1] = 100000; t[6, 2] = 80000; t[7, 3] = 70000
    order, split, gmax = run(t, 5120)
    shift = max(0, (100000).bit_length() - 8)
    want = int(np.count_nonzero((gmax >> shift) >= (((100000 >> shift) * 3 + 3) // 4)))
    assert split == want == 2 and order[0] == 5
    # a frame of equal tiles, and a frame without ticks
    assert run(np.full((n, 4), 5000, np.uint32), 5120)[1] == 0
    assert run(np.zeros((n, 4), np.uint32), 5120)[1] == 0


def test_heaviest_tiles_as_part_tile_waves_never_change_pixels(V, golden, product_scenes):
    """VRT_OPT_HEAVY_TILES: once the scheduler has an order, the general VRT_MODE_FULL kernel traces the few heaviest groups of tiles as
    eight waves per tile. The reference's room (the frame is as long as its longest wave there) at four committed frames: every
    launch -- measuring, ordered, ordered with part-tile waves -- equals the oracle's hashes; the split engages on these frames (its
    count is read back), and the other modes, the option switched off and an opaque scene under either full kernel keep their pixels."""
    tex, dim = product_scenes["room"]
    for key in ("room_inside_1080p_full/mode2", "room_inside_720p_full/mode2", "room_outside_1080p_full/mode2", "room_outside_720p_full/mode2"):
        g = golden["frames"]["frames"][key]
        W, H = g["width"], g["height"]
        for on in (1, 0):
            c = V.Context(0)
            try:
                c.upload_octree(tex, dim)
                ip, iv, cp, _ = V.camera_block(g["pose"][:3], g["pose"][3], g["pose"][4], W, H)
                c.set_camera(ip, iv, cp)
                c.set_tile_scheduling(3)
                c.set_option(V.OPT_HEAVY_TILES, on)
                counts = []
                for k in range(7):
                    rgba, idd = c.dispatch(W, H, 2)
                    assert "%016x" % V.fnv1a64(rgba) == g["rgba_fnv1a64"], (key, on, k)
                    assert "%016x" % V.fnv1a64(idd) == g["id_dist_fnv1a64"], (key, on, k)
                    counts.append(c.sched_split_count())
                assert counts[0] == 0 and max(counts) <= 64
                assert max(counts) > 0, (key, counts)      # the order kernel names heavy groups on these frames
                g1 = golden["frames"]["frames"].get(key.replace("_full/mode2", "/mode1"))
                if g1:                                    # a launch of another mode on the same stream never reads them
                    rgba, idd = c.dispatch(W, H, 1)
                    assert "%016x" % V.fnv1a64(rgba) == g1["rgba_fnv1a64"]
            finally:
                c.close()
    # the same frame as two interleaved row shards on two streams (bench.py's pipeline): a scheduler state and a split count per stream
    # and shard, rows addressed through the shard's own row mapping
    import torch
    g = golden["frames"]["frames"]["room_inside_1080p_full/mode2"]
    W, H = g["width"], g["height"]
    c = V.Context(0)
    try:
        c.upload_octree(tex, dim)
        ip, iv, cp, _ = V.camera_block(g["pose"][:3], g["pose"][3], g["pose"][4], W, H)
        c.set_camera(ip, iv, cp)
        c.set_tile_scheduling(0)
        full_rgba, full_id = c.dispatch(W, H, 2)
        assert "%016x" % V.fnv1a64(full_rgba) == g["rgba_fnv1a64"]
        c.set_tile_scheduling(2)
        dev = torch.device("cuda:0")
        streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        rows = [V.shard_row_indices(H, 8, s, 2) for s in range(2)]
        bufs = [(torch.zeros((len(rows[s]), W), dtype=torch.int32, device=dev), torch.zeros((len(rows[s]), W, 2), dtype=torch.int32, device=dev))
                for s in range(2)]
        split_seen = 0
        for k in range(6):
            for s in range(2):
                bufs[s][0].zero_(); bufs[s][1].zero_()
                torch.cuda.synchronize()
                c.dispatch_shard(W, H, 8, s, 2, 2, bufs[s][0].data_ptr(), bufs[s][1].data_ptr(), streams[s].cuda_stream)
                torch.cuda.synchronize()
                assert np.array_equal(bufs[s][0].cpu().numpy().view(np.uint8).reshape(-1, W, 4), full_rgba[rows[s]]), (k, s)
                assert np.array_equal(bufs[s][1].cpu().numpy(), full_id[rows[s]]), (k, s)
                split_seen = max(split_seen, c.sched_split_count(streams[s].cuda_stream))
        assert split_seen > 0
    finally:
        c.close()
    # an opaque scene: the stack-free kernel has no part-tile waves; the general kernel (FULL_OPAQUE 0) may take them; pixels as committed
    g = golden["frames"]["frames"]["dragon_720p_full/mode2"]
    tex, dim = product_scenes["dragon"]
    c = V.Context(0)
    try:
        c.upload_octree(tex, dim)
        ip, iv, cp, _ = V.camera_block(g["pose"][:3], g["pose"][3], g["pose"][4], g["width"], g["height"])
        c.set_camera(ip, iv, cp)
        c.set_tile_scheduling(2)
        for full_opaque in (6, 0):
            c.set_option(V.OPT_FULL_OPAQUE, full_opaque)
            for k in range(5):
                rgba, idd = c.dispatch(g["width"], g["height"], 2)
                assert "%016x" % V.fnv1a64(rgba) == g["rgba_fnv1a64"], (full_opaque, k)
                assert "%016x" % V.fnv1a64(idd) == g["id_dist_fnv1a64"], (full_opaque, k)
    finally:
        c.close()


def test_feedback_tile_scheduling_never_changes_pixels(V, O, product_scenes):
    """vrt_set_tile_scheduling: launches that repeat a shape start their tiles in an order derived from measured tile
    times. Whatever that order is -- fresh, stale after the camera moved or the scene changed, re-derived on every
    launch -- each frame must equal the oracle's, and the order must be a permutation of the launch's workgroups.
    Covers the three scheduled kernel flavours (measure, ordered, ordered + measure), a tile count that is not a
    multiple of the workgroup's four tiles, both modes, a row shard and two streams with their own states."""
    import torch
    tex, dim = product_scenes["dragon"]
    c = V.Context(0)
    try:
        c.upload_octree(tex, dim)
        poses = [(63.5, 60.5, 140.5, -90.0, -10.0), (70.5, 58.5, 120.5, -95.0, -8.0), (20.5, 90.5, 100.5, -60.0, -30.0)]
        for (W, H), mode, period in [((1016, 520), 0, 2), ((1024, 512), 1, 3), ((1016, 520), 0, 1)]:
            n_wg = (((W + 7) // 8) * ((H + 7) // 8) + 3) // 4
            assert n_wg >= 2048
            c.set_tile_scheduling(period)
            seen_orders = []
            for k in range(7):
                pose = poses[(k // 2) % len(poses)]          # the camera moves every other frame: orders go stale
                ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
                c.set_camera(ip, iv, cp)
                rgba, idd = c.dispatch(W, H, mode)
                if k % 2 == 0:
                    ref_rgba, ref_id, _ = _oracle_frame(O, tex, dim, (ip, iv, cp), W, H, mode)
                _assert_same(rgba, ref_rgba, f"{W}x{H} mode {mode} period {period} frame {k} rgba8")
                _assert_same(idd, ref_id, f"{W}x{H} mode {mode} period {period} frame {k} id/dist")
                o = c.sched_order()
                if k == 0 and period > 1:
                    assert o.size == 0        # a shape's first launch is never the measured one (it may be cold)
                    continue
                assert o.size == n_wg and np.array_equal(np.sort(o), np.arange(n_wg, dtype=np.uint32)), (W, H, k)
                seen_orders.append(o)
            assert any(not np.array_equal(o, np.arange(n_wg)) for o in seen_orders)   # it does reorder
            # switched off: row-major starts again, same pixels
            c.set_tile_scheduling(0)
            rgba, idd = c.dispatch(W, H, mode)
            _assert_same(rgba, ref_rgba, "scheduling off rgba8")
            _assert_same(idd, ref_id, "scheduling off id/dist")
        # a scene edit under a live order: the stale order is still a permutation
        c.set_tile_scheduling(2)
        W, H = 1024, 512
        ip, iv, cp, _ = V.camera_block(poses[0][:3], poses[0][3], poses[0][4], W, H)
        c.set_camera(ip, iv, cp)
        for _ in range(3):
            c.dispatch(W, H, 0)
        tex2, dim2 = product_scenes["monu9"]
        c.upload_octree(tex2, dim2)
        ref_rgba, ref_id, _ = _oracle_frame(O, tex2, dim2, (ip, iv, cp), W, H, 0)
        for k in range(3):
            rgba, idd = c.dispatch(W, H, 0)
            _assert_same(rgba, ref_rgba, f"after scene change frame {k} rgba8")
            _assert_same(idd, ref_id, f"after scene change frame {k} id/dist")
        # more launch shapes than the scheduler keeps states for: the least recently used ones are recycled
        c.upload_octree(tex, dim)
        pose = poses[0]
        for k in range(20):
            W, H = 1024 + 8 * k, 520
            ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
            c.set_camera(ip, iv, cp)
            c.set_tile_scheduling(0)
            ref_rgba, ref_id = c.dispatch(W, H, 0)
            c.set_tile_scheduling(1)
            for _ in range(2):
                rgba, idd = c.dispatch(W, H, 0)
                _assert_same(rgba, ref_rgba, f"shape {k} rgba8")
                _assert_same(idd, ref_id, f"shape {k} id/dist")
        # two streams alternating frames of one shape (bench.py's pipeline) and a 2-way row shard: a state per stream
        c.upload_octree(tex, dim)
        W, H = 1920, 1080
        ip, iv, cp, _ = V.camera_block(poses[0][:3], poses[0][3], poses[0][4], W, H)
        c.set_camera(ip, iv, cp)
        c.set_tile_scheduling(0)
        full_rgba, full_id = c.dispatch(W, H, 1)
        c.set_tile_scheduling(2)
        dev = torch.device("cuda:0")
        streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        for n_shards in (1, 2):
            rows = [V.shard_row_indices(H, 8, s, n_shards) for s in range(n_shards)]
            bufs = [[(torch.zeros((len(rows[s]), W), dtype=torch.int32, device=dev),
                      torch.zeros((len(rows[s]), W, 2), dtype=torch.int32, device=dev)) for s in range(n_shards)] for _ in range(2)]
            torch.cuda.synchronize()
            for k in range(10):
                for s in range(n_shards):
                    r, i = bufs[k & 1][s]
                    c.dispatch_shard(W, H, 8, s, n_shards, 1, r.data_ptr(), i.data_ptr(), streams[k & 1].cuda_stream)
            torch.cuda.synchronize()
            for b in bufs:
                for s in range(n_shards):
                    assert np.array_equal(b[s][0].cpu().numpy().view(np.uint8).reshape(-1, W, 4), full_rgba[rows[s]]), (n_shards, s)
                    assert np.array_equal(b[s][1].cpu().numpy(), full_id[rows[s]]), (n_shards, s)
            for st in streams:
                o = c.sched_order(st.cuda_stream)
                assert o.size and np.array_equal(np.sort(o), np.arange(o.size, dtype=np.uint32))
    finally:
        c.close()


def test_error_behaviour(V):
    c = V.Context(0)
    with pytest.raises(V.VrtError, match="no octree"):
        c.dispatch(8, 8, 0)
    c.upload_octree(np.zeros(0, np.uint8), 1)
    with pytest.raises(V.VrtError, match="no camera"):
        c.dispatch(8, 8, 0)
    ip, iv, cp, _ = V.camera_block((1.5, 2.5, 3.5), -90.0, 0.0, 8, 8)
    c.set_camera(ip, iv, cp)
    with pytest.raises(V.VrtError):
        c.dispatch(0, 8, 0)
    with pytest.raises(V.VrtError):
        c.dispatch(8, 8, 7)
    with pytest.raises(V.VrtError):
        c.set_variant(2)
    with pytest.raises(V.VrtError):
        c.set_option(V.OPT_DISPLAY_KERNEL, 1)
    with pytest.raises(V.VrtError, match="multiple of 4"):
        c.upload_octree(np.zeros(7, np.uint8), 1)
    # a self-referencing header is rejected instead of being expanded forever
    cyc = np.array([1, 0, 0, 0xff] + [0, 0, 0, 0] * 8, np.uint8)
    with pytest.raises(V.VrtError, match="record limit"):
        c.upload_octree(cyc, 3)
    with pytest.raises(V.VrtError, match="period"):
        c.set_tile_scheduling(-1)
    c.set_tile_scheduling(0)
    c.set_tile_scheduling(16)
    assert c.sched_order().size == 0      # nothing large enough has been launched: no order yet
    c.close()


def test_cpp_frame_loop_example_matches_oracle(V, O):
    """examples/frame_main.cpp is the reference's frame loop (load, flatten, upload, pick ray, edit, re-upload,
    full-shader dispatch, display pass) written against include/ the way src/main.cpp is written against the
    reference's headers; its three per-frame hashes must be the oracle's for the same sequence."""
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "examples", "frame_main")
    assert os.path.exists(exe), "examples/frame_main was not built (make -C voxel-raytracer_amd/csrc)"
    W, H = 192, 108
    r = subprocess.run([exe, os.path.join(MAPS, "dragon.vox"), str(W), str(H)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("frame ")]
    assert len(lines) == 2
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    pos = (63.5, 60.5, 140.5)
    ip, iv, cp, front = V.camera_block(pos, -90.0, -10.0, W, H)
    for f, ln in enumerate(lines):
        hit = w.ray_cast(pos, front)
        hl = hit[0] if hit and hit[1] else (-1, -1, -1)
        if f == 1 and hit and hit[1]:
            w.remove(*hit[0])
            w.insert(60, 70, 40, 0xffd2d2ff, 3.0, 1.0, 0.0)
        tex, dim = w.flatten()
        rgba, idd, _ = _oracle_frame(O, tex, dim, (ip, iv, cp), W, H, 2, highlighted=hl)
        shown = O.denoise(rgba, idd)
        want = {"tex_dim": str(dim), "rgba": "%016x" % V.fnv1a64(rgba), "id": "%016x" % V.fnv1a64(idd),
                "shown": "%016x" % V.fnv1a64(shown)}
        got = {k: ln[ln.index(k) + 1] for k in want}
        assert [int(v) for v in ln[ln.index("highlighted") + 1: ln.index("highlighted") + 4]] == list(hl), (f, ln, hl)
        for k, v in want.items():
            assert got[k] == v, (f, k, got[k], v)


def test_seeded_random_scenes_uniforms_and_cameras(ctx, V, O):
    """A bounded random sweep: worlds of random clusters and slabs with random materials, random uniforms
    (globalLight, lightDir, voxelScale, highlighted voxel), random poses inside and outside the model, odd frame
    sizes; all three modes against the oracle, bit for bit."""
    rng = np.random.default_rng(20251)
    palette = [(0xa0a0a0ff, 3.0, 0.0, 0.0), (0x50b43cff, 3.0, 0.0, 0.0), (0xffd2d2ff, 3.0, 1.0, 0.0),
               (0x3c64dc96, 1.33, 0.0, 0.02), (0xc8dcff50, 1.5, 0.0, 0.0), (0xff3030ff, 3.0, 0.25, 0.0),
               (0x20202000, 1.2, 0.0, 0.0)]
    frames_with_hits = hit_pixels = 0
    for case in range(10):
        w = V.World()
        span = int(rng.choice([12, 40, 200]))
        pts = []
        for _ in range(int(rng.integers(1, 5))):                       # slabs
            y = int(rng.integers(0, span // 2 + 1))
            x0, z0 = (int(v) for v in rng.integers(-span // 4, span // 2, size=2))
            sx, sz = (int(v) for v in rng.integers(2, 14, size=2))
            m = palette[int(rng.integers(0, len(palette)))]
            xs, zs = np.meshgrid(np.arange(x0, x0 + sx), np.arange(z0, z0 + sz))
            xyz = np.stack([xs.ravel(), np.full(xs.size, y), zs.ravel()], axis=1)
            w.insert_many(xyz, np.full(len(xyz), m[0], np.uint32), m[1], m[2], m[3])
            pts.append(xyz)
        for _ in range(int(rng.integers(3, 9))):                       # clusters
            c = rng.integers(-span // 4, span, size=3)
            n = int(rng.integers(1, 60))
            xyz = (c + rng.integers(-3, 4, size=(n, 3))).astype(np.int32)
            m = palette[int(rng.integers(0, len(palette)))]
            w.insert_many(xyz, np.full(n, m[0], np.uint32), m[1], m[2], m[3])
            pts.append(xyz)
        pts = np.concatenate(pts)
        tex, dim = w.flatten()
        ctx.upload_octree(tex, dim)
        for _ in range(2):
            W, H = int(rng.integers(9, 90)), int(rng.integers(7, 60))
            target = pts[int(rng.integers(0, len(pts)))] + 0.5           # look at a voxel that exists
            away = rng.normal(size=3)
            away[1] = abs(away[1]) + 0.2
            pos = target + away / np.linalg.norm(away) * rng.choice([1.7, 6.0, span * 0.5, span * 1.5])
            d = target - pos
            yaw = float(np.degrees(np.arctan2(d[2], d[0])))
            pitch = float(np.clip(np.degrees(np.arctan2(d[1], np.hypot(d[0], d[2]))), -89.0, 89.0))
            ip, iv, cp, _ = V.camera_block(tuple(float(v) for v in pos), yaw, pitch, W, H)
            ctx.set_camera(ip, iv, cp)
            p = ctx.default_params()
            s = O.make_scene(tex, dim, ip, iv, cp)
            if rng.random() < 0.5:
                gl = rng.uniform(0.0, 1.5, size=4).astype(np.float32)
                p.global_light[:] = [float(v) for v in gl]
                s.global_light[:] = [float(v) for v in gl]
            if rng.random() < 0.5:
                ld = rng.normal(size=3)
                ld = (ld / np.linalg.norm(ld)).astype(np.float32)
                p.light_dir[:] = [float(v) for v in ld]
                s.light_dir[:] = [float(v) for v in ld]
            if rng.random() < 0.3:
                vs = float(np.float32(rng.choice([0.5, 2.0, 1.25])))
                p.voxel_scale = vs
                s.voxel_scale = vs
            if rng.random() < 0.5:
                hl = [int(v) for v in rng.integers(-2, span // 2, size=3)]
                p.highlighted[:] = hl
                s.highlighted[:] = hl
            ctx.set_params(p)
            for mode in (0, 1, 2):
                ref_rgba, ref_id, _, _ = O.render(s, W, H, mode)
                rgba, idd = ctx.dispatch(W, H, mode)
                what = f"random case {case} {W}x{H} pos {np.round(pos, 2)} mode {mode}"
                _assert_same(rgba, ref_rgba, what + " rgba8")
                _assert_same(idd, ref_id, what + " id/dist")
                _assert_same(ctx.denoise(rgba, idd), O.denoise(rgba, idd), what + " display pass")
            n_hit = int(np.count_nonzero(ref_id[..., 0]))
            frames_with_hits += n_hit > 0
            hit_pixels += n_hit
    ctx.set_params(ctx.default_params())
    assert frames_with_hits >= 15 and hit_pixels > 5000, (frames_with_hits, hit_pixels)   # the sweep looked at geometry


def test_ray_generation_tables_in_range_math_and_host_light_setup(ctx, V, O, product_scenes):
    """The prologue in its two forms (View::gen_fast: per-column / per-row tables from the dispatcher + in-range 1/x and
    sqrt; otherwise the shader's operations one by one) and the shadow ray's set-up made by the dispatcher:
      * rcp_inrange / sqrt_inrange against correctly rounded values over their whole stated ranges;
      * standard projections: tables on == tables off == oracle, all modes, ragged frame sizes (odd and even: an even size
        has a column / row with u = 0 or v = 0, where the sign of a zero term decides);
      * projections the table builder must refuse (sheared, off-centre with a u-dependent w, y flipped: the v = 0 row's
        zero would change sign with the column) and an inverse view matrix out of range (scaled 1e-25): still the oracle's
        frames, through the shader's own prologue;
      * light directions with zero, negative and unnormalised components, primary + shadow."""
    rng = np.random.default_rng(77)
    # in-range math, bit for bit: numpy's float32 division and sqrt are correctly rounded
    e = rng.uniform(-94.9, 125.9, size=400000)
    x = (np.exp2(e) * rng.choice([-1.0, 1.0], size=e.size)).astype(np.float32)
    x = np.concatenate([x, np.float32([2.0 ** -95, -2.0 ** -95, 2.0 ** 125, 1.0, -1.0, 3.0, 1e-8, 0.99999994, 1.0000001,
                                       np.nextafter(np.float32(2.0 ** 126), np.float32(0))])]).astype(np.float32)
    def same_bits(got, want, arg, what):
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, f"{what}: {bad.size} of {arg.size} differ; first: f({arg[bad[0]]!r}) = {got[bad[0]]!r}, want {want[bad[0]]!r}; " \
                              f"arguments {[float(v) for v in arg[bad[:8]]]}"
    got = ctx.debug_math(30, x, x)
    same_bits(got, np.float32(1.0) / x, x, "rcp_inrange vs 1/x")
    e = rng.uniform(-95.9, 127.9, size=400000)
    y = np.exp2(e).astype(np.float32)
    y = np.concatenate([y, np.float32([2.0 ** -96, 1.0, 2.0, 3.0, 4.0, 0.99999994, 1.0000001, 3.4028235e38, 2.0 ** -95, 2.0 ** -94])]).astype(np.float32)
    got = ctx.debug_math(31, y, y)
    same_bits(got, np.sqrt(y), y, "sqrt_inrange vs sqrt")
    # x / PI with the denominator known at compile time: every mantissa at one exponent, random values over the range it is
    # used in (2^-100 .. 2^96), zero
    z = np.concatenate([(np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3f800000)).view(np.float32),
                        np.exp2(rng.uniform(-100.0, 96.0, size=400000)).astype(np.float32), np.float32([0.0, 1.0, 3.14159265359, 2.0 ** 96])])
    got = ctx.debug_math(32, z, z)
    same_bits(got, z / np.float32(3.14159265359), z, "div_pi_inrange vs x / PI")

    tex, dim = product_scenes["dragon"]
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    pose = (63.5, 60.5, 140.5, -90.0, -10.0)
    try:
        for (W, H) in [(96, 54), (97, 55), (64, 64), (33, 20)]:
            ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
            assert V.ray_table(ip, W, H) is not None and V.view_in_range(iv)
            ctx.set_camera(ip, iv, cp)
            for mode in (0, 1, 2):
                ref_rgba, ref_id, _ = _oracle_frame(O, tex, dim, (ip, iv, cp), W, H, mode)
                for tables in (True, False):
                    ctx.set_ray_tables(tables)
                    rgba, idd = ctx.dispatch(W, H, mode)
                    _assert_same(rgba, ref_rgba, f"{W}x{H} mode {mode} tables {tables} rgba8")
                    _assert_same(idd, ref_id, f"{W}x{H} mode {mode} tables {tables} id/dist")
        ctx.set_ray_tables(True)
        W, H = 96, 54
        ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
        exotic = []
        m = np.array(ip, np.float32).copy(); m[4] = 0.05; exotic.append(("sheared", m, iv))                 # x depends on v
        m = np.array(ip, np.float32).copy(); m[3] = 0.01; exotic.append(("w depends on u", m, iv))
        m = np.array(ip, np.float32).copy(); m[5] = -m[5]; exotic.append(("y flipped", m, iv))             # zero of the v = 0 row changes sign
        small = np.array(iv, np.float32).copy(); small[:12] *= np.float32(1e-25); exotic.append(("tiny view matrix", np.array(ip, np.float32), small))
        for name, m, view in exotic:
            if name == "tiny view matrix":
                assert not V.view_in_range(view)
            else:
                assert V.ray_table(m, W, H) is None, name
            ctx.set_camera(m, view, cp)
            for mode in (0, 1):
                ref_rgba, ref_id, _ = _oracle_frame(O, tex, dim, (m, view, cp), W, H, mode)
                rgba, idd = ctx.dispatch(W, H, mode)
                _assert_same(rgba, ref_rgba, f"{name} mode {mode} rgba8")
                _assert_same(idd, ref_id, f"{name} mode {mode} id/dist")
            assert np.count_nonzero(ref_id[..., 0]) > 200 or name == "tiny view matrix", name
        # the shadow ray's set-up on the host
        ctx.set_camera(ip, iv, cp)
        for ld in [(0.0, 1.0, 0.0), (0.0, 0.5, -2.0), (-3.0, 4.0, 0.0), (1e-9, 0.7, 0.7), (-0.3, -0.9, 0.2), (0.5, 0.5, 0.5)]:
            p = ctx.default_params()
            p.light_dir[:] = [float(np.float32(v)) for v in ld]
            ctx.set_params(p)
            s = O.make_scene(tex, dim, ip, iv, cp)
            s.light_dir[:] = [float(np.float32(v)) for v in ld]
            ref_rgba, ref_id, _, _ = O.render(s, W, H, 1)
            rgba, idd = ctx.dispatch(W, H, 1)
            _assert_same(rgba, ref_rgba, f"light {ld} rgba8")
            _assert_same(idd, ref_id, f"light {ld} id/dist")
    finally:
        ctx.set_ray_tables(True)
        ctx.set_params(ctx.default_params())


def test_rays_leaving_the_only_occupied_cube(ctx, V, O, product_scenes):
    """KArgs::root0_only (the dispatcher found the tree empty outside wide root 0): a ray that has been inside that cube
    and left it misses at once instead of walking the empty octants' records. Same frames with the shortcut, without it
    (vrt_set_option(VRT_OPT_EMPTY_OCTANTS, 0)) and from the oracle, for eyes inside the cube, in another octant of the world (negative
    coordinates: those rays must still find their way IN), on the cube's faces and outside the world; all modes."""
    tex, dim = product_scenes["dragon"]
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    poses = [(63.5, 60.5, 140.5, -90.0, -10.0), (63.5, 60.5, -140.5, 90.0, -10.0), (-40.5, 30.5, -60.5, 40.0, 5.0),
             (-200.5, 300.5, 64.5, 0.0, -45.0), (0.0, 40.0, 64.0, 0.0, 0.0), (63.5, 1023.5, 64.5, -90.0, -89.0),
             (64.5, 50.5, 1500.5, -90.0, 0.0), (500.5, -1500.5, 500.5, 45.0, 60.0),
             # eyes INSIDE the model's base, rays leaving the cube through its floor: for them the empty octant below is a
             # change of medium, i.e. the hit (tests/fuzz/fuzz_parity.py seed 215)
             (28.89419336319311, 0.16499097268325547, 39.616358418920996, -133.7363734294383, 0.0),
             (14.728327898581782, 4.885433089213199, 24.668633731061217, -40.812579534368126, 45.72688971438939),
             (40.5, 0.5, 45.5, -90.0, -89.0)]
    try:
        for pose in poses:
            for (W, H) in [(64, 40), (33, 17)]:
                ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
                ctx.set_camera(ip, iv, cp)
                for mode in (0, 1, 2):
                    ref_rgba, ref_id, _ = _oracle_frame(O, tex, dim, (ip, iv, cp), W, H, mode)
                    for on in (True, 2, False):   # with the tightest valid root 0, with build_wide()'s, without the shortcut
                        ctx.set_root0_only(on)
                        rgba, idd = ctx.dispatch(W, H, mode)
                        _assert_same(rgba, ref_rgba, f"pose {pose} {W}x{H} mode {mode} shortcut {on} rgba8")
                        _assert_same(idd, ref_id, f"pose {pose} {W}x{H} mode {mode} shortcut {on} id/dist")
    finally:
        ctx.set_root0_only(True)


def test_complete_frame_in_row_bands_with_halo(V, O, product_scenes):
    """sharding.ShownFramePipeline: the reference's whole frame -- full path tracer, then the display pass -- cut into N
    row bands, each traced with a 20-row halo, filtered as a sub-image and its displayed rows copied into rank 0's frame.
    The ranks run here as objects of one process on one GPU (same kernels, copies and stream flags; no IPC): the
    assembled frame must equal the oracle's display pass over the oracle's full frame, for band counts that leave
    ragged bands and halos clipped by the image, several frames in flight."""
    import importlib
    import torch
    shd = importlib.import_module("voxel-raytracer_amd.sharding")
    tex, dim = product_scenes["dragon"]
    c = V.Context(0)
    try:
        c.upload_octree(tex, dim)
        for (W, H), world in [((96, 88), 3), ((64, 40), 1), ((72, 120), 5)]:
            ip, iv, cp, _ = V.camera_block((63.5, 60.5, 140.5), -90.0, -10.0, W, H)
            c.set_camera(ip, iv, cp)
            ref_rgba, ref_id, _ = _oracle_frame(O, tex, dim, (ip, iv, cp), W, H, 2)
            want = O.denoise(ref_rgba, ref_id)
            root = shd.ShownFramePipeline(c, W, H, 0, world, 2, n_buf=2, group="in-process")
            ranks = [root] + [shd.ShownFramePipeline(c, W, H, r, world, 2, n_buf=2, share=root) for r in range(1, world)]
            try:
                assert sum(p.b1 - p.b0 for p in ranks) == H and all(p.h0 <= p.b0 and p.b1 <= p.h1 for p in ranks)
                for _ in range(5):                      # more frames than slots: the slot-reuse flags are exercised
                    for p in reversed(ranks):           # the root last: its consumer waits for the others' arrivals
                        p.step()
                for p in ranks:
                    assert p.drain(30.0)
                _assert_same(root.last_shown(), want, f"{W}x{H} in {world} bands: displayed frame")
            finally:
                for p in reversed(ranks):
                    p.close()
    finally:
        c.close()


def test_fused_frame_call_equals_dispatch_then_display_pass(ctx, V, product_scenes):
    """vrt_dispatch_frame keeps the two intermediate images on the device; all three results must equal the
    two-call route, at a size off every tile edge."""
    tex, dim = product_scenes["monu9"]
    W, H = 203, 117
    _setup(ctx, V, tex, dim, (48.5, 60.5, 170.5, -90.0, -12.0), W, H)
    for mode in (0, 1, 2):
        rgba, idd = ctx.dispatch(W, H, mode)
        shown = ctx.denoise(rgba, idd)
        f_shown, f_rgba, f_id = ctx.dispatch_frame(W, H, mode)
        _assert_same(f_rgba, rgba, f"fused frame mode {mode} rgba8")
        _assert_same(f_id, idd, f"fused frame mode {mode} id/dist")
        _assert_same(f_shown, shown, f"fused frame mode {mode} shown")


def test_views_in_one_launch_equal_separate_dispatches(ctx, V, product_scenes):
    """vrt_dispatch_views: 1..4 cameras rendered by ONE launch (and by the per-view fallback of the other kernel
    variants) give the pixels of separate vrt_dispatch_shard calls, whole frame and as a row shard."""
    import torch
    tex, dim = product_scenes["dragon"]
    W, H = 200, 117
    poses = [(63.5, 60.5, 140.5, -90.0, -10.0), (20.5, 70.5, 120.5, -70.0, -20.0), (100.5, 30.5, 90.5, -120.0, 5.0),
             (63.5, 200.5, 30.5, -90.0, -80.0)]
    cams = [V.camera_block(p[:3], p[3], p[4], W, H)[:3] for p in poses]
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    for (shard, n_shards) in [(0, 1), (1, 3)]:
        rows = V.shard_rows(H, 8, shard, n_shards)
        for mode in (0, 1, 2):
            ref = []
            for cam in cams:
                ctx.set_camera(*cam)
                r = torch.zeros((rows, W), dtype=torch.int32, device="cuda")
                i = torch.zeros((rows, W, 2), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                ctx.dispatch_shard(W, H, 8, shard, n_shards, mode, r.data_ptr(), i.data_ptr())
                ctx.synchronize()
                ref.append((r.cpu().numpy(), i.cpu().numpy()))
            for variant in (0, 4):                                   # 4: record-array kernels -> one launch per view
                ctx.set_variant(variant)
                for n in (1, 2, 4):
                    outs = [(torch.zeros((rows, W), dtype=torch.int32, device="cuda"),
                             torch.zeros((rows, W, 2), dtype=torch.int32, device="cuda")) for _ in range(n)]
                    torch.cuda.synchronize()
                    ctx.dispatch_views(W, H, 8, shard, n_shards, mode,
                                       [cams[k] + (outs[k][0].data_ptr(), outs[k][1].data_ptr()) for k in range(n)])
                    ctx.synchronize()
                    for k in range(n):
                        assert np.array_equal(outs[k][0].cpu().numpy(), ref[k][0]), (shard, mode, variant, n, k)
                        assert np.array_equal(outs[k][1].cpu().numpy(), ref[k][1]), (shard, mode, variant, n, k)
            ctx.set_variant(0)
    with pytest.raises(V.VrtError):
        ctx.dispatch_views(W, H, 8, 0, 1, 0, [cams[0] + (0, 0)] * 5)


def test_box_edits_are_one_patch_and_equal_full_uploads(V, O):
    """vrt_patch_plan_box + vrth_world_box_records: a fill or a clearance of a whole box of voxels is ONE sub-tree patch (the
    reference re-flattens and re-uploads the world on every click, src/main.cpp:843-914). Aligned and unaligned boxes, boxes that
    cross the 64-unit anchors of the wide layout, boxes in empty space, boxes carved out of the model, a box of glass (the full
    path tracer then leaves its stack-free form); after every edit the patched context renders what a context with a full upload
    of the edited tree renders, and what the oracle renders."""
    rng = np.random.default_rng(5)
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    a, b = V.Context(0), V.Context(0)
    try:
        a.upload_octree(*w.flatten())
        W, H = 160, 90
        cams = [V.camera_block(p[:3], p[3], p[4], W, H)[:3] for p in ((63.5, 60.5, 140.5, -90.0, -10.0), (30.5, 70.5, 20.5, 45.0, -35.0))]
        boxes = [((64, 40, 16), 16, "fill", 0x3296c8ff, 3.0), ((50, 30, 20), 16, "clear", 0, 0.0), ((57, 59, 27), 16, "fill", 0xc86432ff, 3.0),
                 ((10, 80, 40), 4, "fill", 0xffd2d2ff, 3.0), ((120, 2, 50), 9, "fill", 0x50b43cff, 3.0), ((60, 20, 20), 7, "clear", 0, 0.0),
                 ((200, 200, 200), 16, "fill", 0xa0a0a0ff, 3.0), ((40, 60, 10), 5, "fill", 0xc8dcff50, 1.5), ((0, 0, 0), 32, "clear", 0, 0.0)]
        patched = 0
        for k, (lo, n, what, colour, refr) in enumerate(boxes):
            hi = tuple(v + n - 1 for v in lo)
            g = (np.indices((n, n, n)).reshape(3, -1).T + np.array(lo)).astype(np.int32)
            if what == "fill":
                keep = rng.random(len(g)) < (1.0 if k % 2 == 0 else 0.7)    # solid boxes merge into few leaves; ragged ones do not
                w.insert_many(g[keep], np.full(int(keep.sum()), colour, np.uint32), refr, 1.0 if colour == 0xffd2d2ff else 0.0, 0.0)
            else:
                for x, y, z in g:
                    w.remove(int(x), int(y), int(z))
            before = a.scene_info()["n_records"]
            depth = a.patch_box(w, lo, hi)
            if depth is None:
                a.upload_octree(*w.flatten())
            else:
                patched += 1
            tex, dim = w.flatten()
            b.upload_octree(tex, dim)
            info = a.scene_info()
            assert (info["n_texels"], info["tex_dim"]) == (len(tex) // 4, dim), (k, info, len(tex) // 4, dim)
            assert depth is None or info["n_records"] - before < 40000, (k, depth, info["n_records"] - before)
            for ci, cam in enumerate(cams):
                for variant, modes in ((0, (0, 1, 2)), (20, (1,)), (4, (1,))):
                    for mode in modes:
                        frames = []
                        for ctx_ in (a, b):
                            ctx_.set_variant(variant)
                            ctx_.set_camera(*cam)
                            frames.append(ctx_.dispatch(W, H, mode))
                        what_ = f"box {k} {what} {lo}+{n} pose {ci} variant {variant} mode {mode}"
                        _assert_same(frames[0][0], frames[1][0], what_ + " rgba8 (patched vs full upload)")
                        _assert_same(frames[0][1], frames[1][1], what_ + " id/dist (patched vs full upload)")
                        if variant == 0 and mode == 2:
                            ref_rgba, ref_id, _ = _oracle_frame(O, tex, dim, cam, W, H, mode)
                            _assert_same(frames[0][0], ref_rgba, what_ + " rgba8 vs oracle")
                            _assert_same(frames[0][1], ref_id, what_ + " id/dist vs oracle")
        assert patched >= 7, patched
        with pytest.raises(V.VrtError):
            a._chk(a._L.vrt_patch_plan_box(a._h, (__import__("ctypes").c_int32 * 3)(5, 5, 5), (__import__("ctypes").c_int32 * 3)(4, 9, 9), 15, __import__("ctypes").byref(V.Patch())))
    finally:
        a.close()
        b.close()


def test_voxel_edits_patched_on_device_equal_full_uploads(V, O):
    """vrt_patch_plan / vrt_patch_apply: after every build / destroy edit of the host octree, the context patched in
    place renders the frames of a context that received a full upload of the edited tree (wide, bit-indexed and
    explicit-AABB kernels; the display of the eye's medium reads the record array) and the oracle's."""
    rng = np.random.default_rng(77)
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    a, b = V.Context(0), V.Context(0)
    a.upload_octree(*w.flatten())
    W, H = 160, 90
    poses = [(63.5, 60.5, 140.5, -90.0, -10.0), (30.5, 70.5, 20.5, 45.0, -35.0)]
    cams = [V.camera_block(p[:3], p[3], p[4], W, H)[:3] for p in poses]
    patched = full = 0
    existing = []
    for step in range(60):
        kind = step % 6
        if kind in (0, 1):        # destroy something visible from a random direction
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            hit = w.ray_cast(tuple(np.array([63.0, 45.0, 28.0]) - d * 150.0), tuple(d))
            if not hit or not hit[1]:
                continue
            x, y, z = hit[0]
            w.remove(x, y, z)
        elif kind == 2 and existing:   # destroy something built earlier
            x, y, z = existing.pop(int(rng.integers(0, len(existing))))
            w.remove(x, y, z)
        elif kind == 3:            # build far from everything (new branches near the top of the tree)
            x, y, z = (int(v) for v in rng.integers(0, 1000, size=3))
            w.insert(x, y, z, 0xffd2d2ff, 3.0, 1.0, 0.0)
            existing.append((x, y, z))
        elif kind == 4:            # build outside the octant that holds the wide layout
            x, y, z = (int(v) for v in rng.integers(-900, -1, size=3))
            w.insert(x, y, z, 0x50b43cff)
            existing.append((x, y, z))
        else:                      # build next to the model: glass, water, stone
            x, y, z = int(rng.integers(0, 126)), int(rng.integers(0, 95)), int(rng.integers(0, 60))
            m = [(0xc8dcff50, 1.5, 0.0, 0.0), (0x3c64dc96, 1.33, 0.0, 0.02), (0xa0a0a0ff, 3.0, 0.0, 0.0)][step % 3]
            w.insert(x, y, z, *m)
            existing.append((x, y, z))
        depth = a.patch_voxel(w, x, y, z)
        if depth is None:
            a.upload_octree(*w.flatten())
            full += 1
        else:
            patched += 1
        if step % 5 == 4 or step == 59:
            tex, dim = w.flatten()
            b.upload_octree(tex, dim)
            info = a.scene_info()                       # the patches kept the stream's size and u_texDim current
            assert (info["n_texels"], info["tex_dim"]) == (len(tex) // 4, dim), (step, info, len(tex) // 4, dim)
            for ci, cam in enumerate(cams):
                for variant in (0, 20, 4, 1):
                    for mode in ((0, 1, 2) if variant == 0 else (1,)):
                        frames = []
                        for ctx_ in (a, b):
                            ctx_.set_variant(variant)
                            ctx_.set_camera(*cam)
                            ctx_.set_params(ctx_.default_params())
                            frames.append(ctx_.dispatch(W, H, mode))
                        what = f"edit {step} pose {ci} variant {variant} mode {mode}"
                        _assert_same(frames[0][0], frames[1][0], what + " rgba8 (patched vs full upload)")
                        _assert_same(frames[0][1], frames[1][1], what + " id/dist (patched vs full upload)")
                        if variant == 0 and mode == 1:
                            ref_rgba, ref_id, _ = _oracle_frame(O, tex, dim, cam, W, H, mode)
                            _assert_same(frames[0][0], ref_rgba, what + " rgba8 vs oracle")
                            _assert_same(frames[0][1], ref_id, what + " id/dist vs oracle")
    assert patched >= 25 and full >= 5, (patched, full)       # both routes were exercised
    grown = a.scene_info()["n_records"] - b.scene_info()["n_records"]
    assert 0 < grown < 60 * 400, grown          # replaced child blocks stay behind, but only the ones along each path
    # a long session on a small world: the garbage bound makes the plan ask for a full upload now and then
    w2 = V.World()
    for x in range(8):
        for z in range(8):
            w2.insert(x, 0, z, 0xa0a0a0ff)
    a.upload_octree(*w2.flatten())
    refused = batches = 0
    peak = 0
    step = 0
    while step < 4000:
        # every 7th round is a brush stroke: up to 12 edits between vrt_patch_begin and vrt_patch_end (one device update)
        stroke = 12 if (step // 50) % 7 == 3 else 1
        if stroke > 1:
            a.patch_begin()
            batches += 1
        for _ in range(stroke):
            x, y, z = (int(v) for v in rng.integers(0, 24, size=3))
            if step % 3 == 2:
                w2.remove(x, y, z)
            else:
                w2.insert(x, y, z, 0x50b43cff if step % 2 else 0xc8dcff50, 1.5 if step % 2 == 0 else 3.0, 0.0, 0.0)
            step += 1
            if a.patch_voxel(w2, x, y, z) is None:
                refused += 1
                if stroke > 1:
                    a.patch_end()
                a.upload_octree(*w2.flatten())
                if stroke > 1:
                    a.patch_begin()
        if stroke > 1:
            with pytest.raises(V.VrtError, match="batch is open"):
                a.dispatch(W, H, 0)
            if batches % 3 == 1:
                # nothing may re-lay the arrays the open batch indexes (records_before, rewritten records, repointed cells):
                # compaction, both uploads and a change of the world bounds are refused until vrt_patch_end
                with pytest.raises(V.VrtError, match="batch is open"):
                    a.compact()
                with pytest.raises(V.VrtError, match="batch is open"):
                    a.upload_octree(*w2.flatten())
                with pytest.raises(V.VrtError, match="batch is open"):
                    a.upload_records(*w2.records())
                p_ = a.default_params()
                p_.world_min[0] = -2047
                with pytest.raises(V.VrtError, match="batch is open"):
                    a.set_params(p_)
                a.set_params(a.default_params())   # the same bounds: not a change
            a.patch_end()
        peak = max(peak, a.scene_info()["n_records"])
    # what the patches leave behind is reclaimed by the library itself (vrt_compact from vrt_patch_plan): the arrays never
    # grow past about twice the live tree
    live = V.build_layout(w2.flatten()[0])[1].n_records
    assert batches >= 5 and peak < 3 * live + 8192 and a.scene_info()["n_records"] < 2 * live + 8192, (peak, live, refused)
    a.compact()
    assert a.scene_info()["n_records"] == live
    tex, dim = w2.flatten()
    b.upload_octree(tex, dim)
    info = a.scene_info()
    assert (info["n_texels"], info["tex_dim"]) == (len(tex) // 4, dim), (info, len(tex) // 4, dim)
    cam = V.camera_block((12.5, 30.5, 60.5), -90.0, -25.0, W, H)[:3]
    for ctx_ in (a, b):
        ctx_.set_variant(0)
        ctx_.set_camera(*cam)
        ctx_.set_params(ctx_.default_params())
    for mode in (0, 1, 2):
        fa, fb = a.dispatch(W, H, mode), b.dispatch(W, H, mode)
        _assert_same(fa[0], fb[0], f"long session mode {mode} rgba8")
        _assert_same(fa[1], fb[1], f"long session mode {mode} id/dist")
    a.close()
    b.close()
