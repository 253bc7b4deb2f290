"""vrt_shade_rays / vrt_shade_rays_device on the MI355X: pathTrace for the caller's own rays, byte for byte against the checker
(tests/oracle_rays.c) and against the frame paths. A frame's rays give the frame; arbitrary rays -- origins in empty space, in
glass, in solids, on faces, in the empty octants and outside the world, axis-parallel and un-normalised directions -- give the
checker's bytes in all three modes; sample ranges give the exact mean; every variant, dispatcher option, upload form, patch and
compaction gives the same bytes; nothing else of the context changes; the device form, the error codes and one batch with
unusable rays."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_rays
from conftest import MAPS, random_voxels
from test_gpu_accum_jitter import SCENES

pytestmark = pytest.mark.gpu
F = np.float32
MODES = (0, 1, 2)


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_rays"))


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _same(got, ref, what):
    if not np.array_equal(got, ref):
        bad = np.argwhere(np.any(got != ref, axis=-1))[:, 0]
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(ref)} rays differ; first ray {i}: got {got[i]} want {ref[i]}")


def _cam(V, pose=(63.5, 60.5, 140.5, -90.0, -10.0), W=64, H=64):
    return V.camera_block(pose[:3], pose[3], pose[4], W, H)[:3]


def _materials_world(V):
    """a floor, lights, water, glass and grass; a block of water and a block of glass to start rays in"""
    w = V.World()
    rng = np.random.default_rng(5)
    for x in range(0, 24):
        for z in range(0, 24):
            w.insert(x, 0, z, 0xa0a0a0ff)
    for _ in range(200):
        x, y, z = (int(v) for v in rng.integers(2, 22, size=3))
        kind = rng.integers(0, 4)
        if kind == 0:
            w.insert(x, y, z, 0xffd2d2ff, 3.0, 1.0, 0.0)        # emissive
        elif kind == 1:
            w.insert(x, y, z, 0x3c64dc96, 1.33, 0.0, 0.0)       # water
        elif kind == 2:
            w.insert(x, y, z, 0xc8dcff50, 1.5, 0.0, 0.0)        # glass
        else:
            w.insert(x, y, z, 0x50b43cff)
    for x in range(30, 36):
        for y in range(2, 8):
            for z in range(8, 14):
                w.insert(x, y, z, 0xc8dcff50, 1.5, 0.0, 0.0)    # a block of glass
    for x in range(30, 36):
        for y in range(2, 8):
            for z in range(16, 22):
                w.insert(x, y, z, 0x644628ff)                   # a solid block
    return w


def _ray_mix(rng, n, lo, hi, inside_glass, inside_solid):
    """n rays: every kind of origin and direction the entry point has to take; lo / hi: the box that holds the content"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    span = hi - lo
    o = np.empty((n, 3), np.float64)
    kind = rng.integers(0, 8, size=n)
    for i in range(n):
        k = kind[i]
        if k == 0:      # empty space around and inside the content
            o[i] = lo - 0.3 * span + rng.random(3) * 1.6 * span
        elif k == 1:    # inside glass
            o[i] = np.asarray(inside_glass[0]) + rng.random(3) * (np.asarray(inside_glass[1]) - np.asarray(inside_glass[0]))
        elif k == 2:    # inside an opaque voxel
            o[i] = np.asarray(inside_solid[0]) + rng.random(3) * (np.asarray(inside_solid[1]) - np.asarray(inside_solid[0]))
        elif k == 3:    # exactly on a voxel face
            o[i] = lo + rng.random(3) * span
            o[i, rng.integers(0, 3)] = float(rng.integers(int(lo[0]), int(hi[0]) + 1))
        elif k == 4:    # integer coordinates
            o[i] = rng.integers(int(lo.min()) - 2, int(hi.max()) + 3, size=3)
        elif k == 5:    # one of the other seven octants of the world
            sign = np.array([-1.0 if b else 1.0 for b in ((rng.integers(1, 8) >> np.arange(3)) & 1)])
            o[i] = sign * (5.0 + rng.random(3) * 400.0)
        elif k == 6:    # outside the world
            o[i] = (lo + hi) / 2 + (rng.integers(0, 2, size=3) * 2 - 1) * (1100.0 + rng.random(3) * 900.0) * (rng.random(3) < 0.6)
            if np.all(np.abs(o[i]) < 1024):
                o[i, 1] = 1500.0
        else:           # the far side of the occupied cube
            o[i] = hi + 2.0 + rng.random(3) * 200.0
    target = lo + rng.random((n, 3)) * span
    d = target - o
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)
    dk = rng.integers(0, 6, size=n)
    for i in range(n):
        if dk[i] == 0:      # axis-parallel
            a = rng.integers(0, 3)
            s = np.sign(d[i, a]) or 1.0
            d[i] = 0.0
            d[i, a] = s
        elif dk[i] == 1:    # a component in (-1e-8, 0]
            d[i, rng.integers(0, 3)] = rng.choice([-0.0, 0.0, -5e-9, -9.9e-9, -1e-12])
        elif dk[i] == 2:    # two zero components, one of them negative zero
            a = rng.integers(0, 3)
            d[i, (a + 1) % 3] = -0.0
            d[i, (a + 2) % 3] = 0.0
    d *= (10.0 ** rng.uniform(-3.0, 3.0, size=(n, 1)))   # un-normalised: lengths 1e-3 .. 1e3
    return o.astype(F), d.astype(F)


def _most_hit_voxels(ctx, o, d, k):
    """the k voxels the picking query (vrt_cast_rays) returns most often for these rays, most frequent first"""
    hit, coord, _, _, _ = ctx.cast_rays(o, d)
    uniq, counts = np.unique(coord[hit], axis=0, return_counts=True)
    return [tuple(int(v) for v in uniq[i]) for i in np.argsort(-counts)[:k]]


def _oracle_scene(O, V, tex, dim, scale=1.0, highlighted=(-1, -1, -1), bounds=None):
    s = O.make_scene(tex, dim, *_cam(V), highlighted=highlighted)
    s.voxel_scale = scale
    if bounds:
        s.bounds_min[:] = bounds[0]
        s.bounds_max[:] = bounds[1]
    return s


def _params(ctx, scale=1.0, highlighted=(-1, -1, -1), bounds=None):
    p = ctx.default_params()
    p.voxel_scale = scale
    p.highlighted[:] = highlighted
    if bounds:
        p.world_min[:] = bounds[0]
        p.world_max[:] = bounds[1]
    ctx.set_params(p)


def _check(ctx, R, s, o, d, what, widths=(None,), modes=MODES, sample=0):
    for mode in modes:
        for width in widths:
            ref_rgba, ref_id = oracle_rays.shade(R, s, o, d, mode, width, sample)
            rgba, idd = ctx.shade_rays(o, d, mode, width=width, first_sample=sample)
            _same(rgba, ref_rgba, f"{what} mode {mode} width {width} rgba8")
            _same(idd, ref_id, f"{what} mode {mode} width {width} id_dist")


# ---- 1. a frame's rays give the frame ----

@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_frames_rays_give_the_frame(ctx, V, O, R, product_scenes, name):
    m, W, H, pose = SCENES[name]
    tex, dim = product_scenes[m]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    ctx.upload_octree(tex, dim)
    ctx.set_camera(ip, iv, cp)
    ctx.set_params(ctx.default_params())
    s = O.make_scene(tex, dim, ip, iv, cp)
    o, d = oracle_rays.frame_rays(R, s, W, H)
    for mode in MODES:
        ref_rgba, ref_id, _, _ = O.render(s, W, H, mode)
        frame_rgba, frame_id = ctx.dispatch(W, H, mode)
        assert np.array_equal(frame_rgba, ref_rgba) and np.array_equal(frame_id, ref_id)
        for origins, how in ((o, "per-ray origins"), (o[0], "stride 0")):
            rgba, idd = ctx.shade_rays(origins, d, mode, width=W)
            _same(rgba, frame_rgba.reshape(-1, 4), f"{name} mode {mode} {how} rgba8")
            _same(idd, frame_id.reshape(-1, 2), f"{name} mode {mode} {how} id_dist")


@pytest.mark.parametrize("key", ["dragon_1080p/mode0", "dragon_1080p/mode1", "dragon_1080p_full/mode2"])
def test_the_1080p_dragon_frame_as_a_batch_matches_the_committed_hashes(ctx, V, O, R, golden, product_scenes, key):
    g = golden["frames"]["frames"][key]
    tex, dim = product_scenes[g["map"]]
    W, H = g["width"], g["height"]
    pose = g["pose"]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    o, d = oracle_rays.frame_rays(R, O.make_scene(tex, dim, ip, iv, cp), W, H)
    rgba, idd = ctx.shade_rays(o[0], d, g["mode"], width=W)
    assert "%016x" % V.fnv1a64(rgba) == g["rgba_fnv1a64"], key
    assert "%016x" % V.fnv1a64(idd) == g["id_dist_fnv1a64"], key


# ---- 2. arbitrary rays against the checker ----

def test_arbitrary_rays_on_the_dragon(ctx, V, O, R, product_scenes):
    tex, dim = product_scenes["dragon"]
    ctx.upload_octree(tex, dim)
    rng = np.random.default_rng(11)
    # dragon.vox has no glass: "inside glass" rays start inside the model's solid base as well
    o, d = _ray_mix(rng, 3000, (0, 0, 0), (126, 95, 60), ((40, 2, 20), (80, 6, 40)), ((50, 1, 25), (70, 4, 35)))
    hit = ctx.shade_rays(o, d, 0)[1][:, 0]
    assert np.count_nonzero(hit) > 300
    for scale in (1.0, 2.0):
        _params(ctx, scale)
        s = _oracle_scene(O, V, tex, dim, scale)
        _check(ctx, R, s, o if scale == 1.0 else o / F(scale), d, f"dragon scale {scale}", widths=(1, 7, 64, None))
    # a highlighted voxel that some rays hit: u_highlightedVoxel is compared with the hit's map position, so the candidates are
    # the voxels the picking query finds most often, and the first one that changes a ray is taken
    _params(ctx)
    plain = ctx.shade_rays(o, d, 1)[0]
    hl = None
    for cand in _most_hit_voxels(ctx, o, d, 40):
        _params(ctx, 1.0, cand)
        if not np.array_equal(plain, ctx.shade_rays(o, d, 1)[0]):
            hl = cand
            break
    assert hl is not None, "no ray hit a highlighted voxel"
    _check(ctx, R, _oracle_scene(O, V, tex, dim, 1.0, hl), o, d, f"dragon highlighted {hl}")
    _params(ctx)


def test_arbitrary_rays_in_the_room_and_a_world_with_glass_and_lights(ctx, V, O, R, product_scenes):
    rng = np.random.default_rng(12)
    tex, dim = product_scenes["room"]
    ctx.upload_octree(tex, dim)
    _params(ctx)
    o, d = _ray_mix(rng, 2500, (0, 0, 0), (120, 64, 120), ((10, 20, 10), (20, 40, 20)), ((0, 0, 0), (120, 1, 120)))
    _check(ctx, R, _oracle_scene(O, V, tex, dim), o, d, "room", widths=(7, None))
    w = _materials_world(V)
    tex, dim = w.flatten()
    w.close()
    ctx.upload_octree(tex, dim)
    o, d = _ray_mix(rng, 3000, (0, 0, 0), (50, 24, 24), ((30, 2, 8), (36, 8, 14)), ((30, 2, 16), (36, 8, 22)))
    for scale, hl in ((1.0, (-1, -1, -1)), (2.0, (5, 0, 20)), (1.0, (32, 4, 10))):
        _params(ctx, scale, hl)
        _check(ctx, R, _oracle_scene(O, V, tex, dim, scale, hl), o if scale == 1.0 else o / F(scale), d,
               f"materials scale {scale} hl {hl}", widths=(1, 7, 64, None))
    _params(ctx)


# ---- 3. samples ----

def test_sample_ranges_give_the_exact_mean(ctx, V, O, R, product_scenes):
    tex, dim = product_scenes["dragon"]
    ctx.upload_octree(tex, dim)
    _params(ctx)
    s = _oracle_scene(O, V, tex, dim)
    rng = np.random.default_rng(13)
    o, d = _ray_mix(rng, 1500, (0, 0, 0), (126, 95, 60), ((40, 2, 20), (80, 6, 40)), ((50, 1, 25), (70, 4, 35)))
    for first in (0, 5, 2 ** 32 - 3):
        for n in (1, 2, 9):
            ref_rgba, ref_id = oracle_rays.mean(R, s, o, d, 2, 64, first, n)
            rgba, idd = ctx.shade_rays(o, d, 2, width=64, first_sample=first, n_samples=n)
            _same(rgba, ref_rgba, f"first {first} n {n} rgba8")
            _same(idd, ref_id, f"first {first} n {n} id_dist")
    for mode in (0, 1):
        one = ctx.shade_rays(o, d, mode, width=64)
        nine = ctx.shade_rays(o, d, mode, width=64, first_sample=3, n_samples=9)
        assert np.array_equal(one[0], nine[0]) and np.array_equal(one[1], nine[1])


# ---- 4. every route ----

def test_every_variant_option_upload_form_patch_and_compaction(V, O, R, product_scenes):
    rng = np.random.default_rng(14)
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    tex, dim = w.flatten()
    c = V.Context(0)   # never has a camera set
    try:
        c.upload_octree(tex, dim)
        o, d = _ray_mix(rng, 2000, (0, 0, 0), (126, 95, 60), ((40, 2, 20), (80, 6, 40)), ((50, 1, 25), (70, 4, 35)))
        s = _oracle_scene(O, V, tex, dim)
        refs = {mode: oracle_rays.mean(R, s, o, d, mode, 64, 3, 2 if mode == 2 else 1) for mode in MODES}

        def check(what):
            for mode in MODES:
                rgba, idd = c.shade_rays(o, d, mode, width=64, first_sample=3, n_samples=2 if mode == 2 else 1)
                _same(rgba, refs[mode][0], f"{what} mode {mode} rgba8")
                _same(idd, refs[mode][1], f"{what} mode {mode} id_dist")

        for var in V.available_variants():
            c.set_variant(var)
            check(f"variant {var}")
        c.set_variant(0)
        defaults = {V.OPT_EMPTY_OCTANTS: 1, V.OPT_FULL_OPAQUE: 6, V.OPT_RAY_TABLES: 1}
        for opt, val in [(V.OPT_EMPTY_OCTANTS, 0), (V.OPT_EMPTY_OCTANTS, 2), (V.OPT_EMPTY_OCTANTS, 1), (V.OPT_FULL_OPAQUE, 0),
                         (V.OPT_FULL_OPAQUE, 1), (V.OPT_RAY_TABLES, 0), (V.OPT_RAY_TABLES, 1)]:
            c.set_option(opt, val)
            check(f"option {opt}={val}")
            c.set_option(opt, defaults[opt])
        c.upload_records(*w.records())
        check("records-only upload")
        # a voxel patch, then compaction: the result follows the edit
        c.upload_octree(tex, dim)
        before = c.shade_rays(o, d, 1)[0]
        for x, y, z in _most_hit_voxels(c, o, d, 30):
            w.remove(x, y, z)
            if c.patch_voxel(w, x, y, z) is None:
                c.upload_octree(*w.flatten())
        tex2, dim2 = w.flatten()
        s2 = _oracle_scene(O, V, tex2, dim2)
        refs = {mode: oracle_rays.mean(R, s2, o, d, mode, 64, 3, 2 if mode == 2 else 1) for mode in MODES}
        check("after a voxel patch")
        assert not np.array_equal(before, c.shade_rays(o, d, 1)[0]), "the edit changed no ray"
        c.compact()
        check("after compaction")
    finally:
        c.close()
        w.close()


def test_worlds_the_wide_layout_cannot_express(ctx, V, O, R):
    """test_gpu_parity's fixtures: eight wide roots (rays cross between them), a world the root table refuses (record-array
    kernels) and a unit-size internal node (explicit-AABB kernels)"""
    rng = np.random.default_rng(4)
    xyz, rgba = random_voxels(rng, 5000, -60, 70)
    try:
        for wmin, wmax in [((-256,) * 3, (256,) * 3), ((-64,) * 3, (192,) * 3)]:
            w = V.World(world_min=wmin, world_max=wmax)
            w.insert_many(xyz, rgba)
            tex, dim = w.flatten()
            w.close()
            ctx.upload_octree(tex, dim)
            _params(ctx, bounds=(wmin, wmax))
            s = _oracle_scene(O, V, tex, dim, bounds=(wmin, wmax))
            o, d = _ray_mix(np.random.default_rng(15), 2000, (-60, -60, -60), (70, 70, 70), ((-10, -10, -10), (10, 10, 10)),
                            ((-30, -30, -30), (-20, -20, -20)))
            for var in V.available_variants():
                ctx.set_variant(var)
                _check(ctx, R, s, o, d, f"world {wmin} variant {var}", widths=(7,))
        tx = lambda value, alpha: [value & 255, (value >> 8) & 255, (value >> 16) & 255, alpha]   # noqa: E731
        leaf = [200, 40, 90, 255, 255, 0, 0, 255]
        unit = (tx(1, 0x80) + tx(2, 0) + tx(3, 0x01) + tx(4, 0) + tx(5, 0x01) + tx(6, 0) + tx(7, 0x80) + tx(8 | 0x800000, 0) + leaf)
        tex = np.array(unit, np.uint8)
        ctx.set_variant(0)
        ctx.upload_octree(tex, 3)
        _params(ctx, bounds=((0, 0, 0), (8, 8, 8)))
        s = _oracle_scene(O, V, tex, 3, bounds=((0, 0, 0), (8, 8, 8)))
        o, d = _ray_mix(np.random.default_rng(16), 1000, (0, 0, 0), (8, 8, 8), ((4, 4, 4), (5, 5, 5)), ((4, 4, 4), (5, 5, 5)))
        _check(ctx, R, s, o, d, "unit internal node", widths=(7,))
    finally:
        ctx.set_variant(0)
        _params(ctx)


# ---- 5. isolation ----

def test_nothing_else_of_the_context_changes(ctx, V, O, R, product_scenes):
    m, W, H, pose = SCENES["room_inside"]
    tex, dim = product_scenes[m]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    ctx.upload_octree(tex, dim)
    ctx.set_camera(ip, iv, cp)
    _params(ctx)
    rng = np.random.default_rng(17)
    o, d = _ray_mix(rng, 1500, (0, 0, 0), (120, 64, 120), ((10, 20, 10), (20, 40, 20)), ((0, 0, 0), (120, 1, 120)))
    s = O.make_scene(tex, dim, ip, iv, cp)
    want = {mode: oracle_rays.shade(R, s, o, d, mode, 7) for mode in MODES}

    def shade_all():
        for mode in MODES:
            rgba, idd = ctx.shade_rays(o, d, mode, width=7)
            _same(rgba, want[mode][0], f"interleaved mode {mode} rgba8")
            _same(idd, want[mode][1], f"interleaved mode {mode} id_dist")

    frames = {mode: ctx.dispatch(W, H, mode) for mode in MODES}
    casts = ctx.cast_rays(o, d)
    # the reference run of the accumulation: lens, jitter and adaptive, 2 + 3 rounds, nothing in between
    ctx.set_lens(0.7, 30.0)
    try:
        ctx.accum_begin(W, H, 4, mode=2, jitter=True, adaptive=(2, 6, 3))
        assert ctx.accum_add(2) == 2 and ctx.accum_add(3) == 5
        ref_accum = ctx.accum_resolve()
        ref_counts = ctx.accum_counts()
        # the same with shade_rays calls between every step
        shade_all()
        ctx.accum_begin(W, H, 4, mode=2, jitter=True, adaptive=(2, 6, 3))
        shade_all()
        assert ctx.accum_add(2) == 2
        shade_all()
        assert ctx.accum_add(3) == 5, "accum_add after shade_rays restarted the accumulation"
        shade_all()
        got = ctx.accum_resolve()
        for a, b, what in zip(got, ref_accum, ("rgba8", "id_dist", "shown")):
            assert np.array_equal(a, b), f"accumulation {what} changed"
        counts = ctx.accum_counts()
        assert np.array_equal(counts[0], ref_counts[0]) and counts[1] == ref_counts[1]
    finally:
        ctx.set_lens(0.0, 1.0)
    for mode in MODES:
        rgba, idd = ctx.dispatch(W, H, mode)
        assert np.array_equal(rgba, frames[mode][0]) and np.array_equal(idd, frames[mode][1]), f"frame mode {mode} changed"
        shade_all()
    for a, b in zip(ctx.cast_rays(o, d), casts):
        assert np.array_equal(a, b)


def test_a_context_that_never_had_a_camera(V, O, R, product_scenes):
    tex, dim = product_scenes["monu9"]
    c = V.Context(0)
    try:
        c.upload_octree(tex, dim)
        o, d = _ray_mix(np.random.default_rng(18), 1000, (0, 0, 0), (100, 100, 100), ((40, 0, 40), (60, 4, 60)), ((40, 0, 40), (60, 4, 60)))
        _check(c, R, _oracle_scene(O, V, tex, dim), o, d, "no camera", widths=(64,))
    finally:
        c.close()


# ---- 6. the device form ----

def test_device_form_on_both_streams_and_after_a_patch(V, O, R):
    import torch
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    c = V.Context(0)
    c.upload_octree(*w.flatten())
    o, d = _ray_mix(np.random.default_rng(19), 4096, (0, 0, 0), (126, 95, 60), ((40, 2, 20), (80, 6, 40)), ((50, 1, 25), (70, 4, 35)))
    n = len(d)
    bufs = [c.device_alloc(o.nbytes), c.device_alloc(d.nbytes), c.device_alloc(n * 4), c.device_alloc(n * 8), c.device_alloc(4)]
    d_o, d_d, d_rgba, d_id, flag = bufs
    try:
        side = torch.cuda.Stream(device=0)
        sp = side.cuda_stream
        c.device_write(d_o, o)
        c.device_write(d_d, d)
        for mode, n_samples in ((0, 1), (1, 1), (2, 1), (2, 3)):
            want = c.shade_rays(o, d, mode, width=64, first_sample=2, n_samples=n_samples)
            want0 = c.shade_rays(o[0], d, mode, width=64, first_sample=2, n_samples=n_samples)
            for stream in (None, sp):
                for stride, ref in ((3, want), (0, want0)):
                    c.shade_rays_device(n, d_o, stride, d_d, d_rgba, d_id, mode=mode, width=64, first_sample=2, n_samples=n_samples,
                                        stream=stream)
                    rgba = c.device_read(d_rgba, (n, 4), np.uint8, stream=stream)
                    idd = c.device_read(d_id, (n, 2), np.int32, stream=stream)
                    _same(rgba, ref[0], f"device form mode {mode} stream {stream} stride {stride} rgba8")
                    _same(idd, ref[1], f"device form mode {mode} stream {stream} stride {stride} id_dist")
            # one output only
            c.device_write(d_id, np.zeros((n, 2), np.int32))
            c.shade_rays_device(n, d_o, 3, d_d, d_rgba, None, mode=mode, width=64, first_sample=2, n_samples=n_samples)
            assert not c.device_read(d_id, (n, 2), np.int32).any()
            _same(c.device_read(d_rgba, (n, 4), np.uint8), want[0], f"device form mode {mode} rgba8 only")
        # ordered after a patch enqueued before it
        before = c.shade_rays(o, d, 1)[0]
        for x in range(40, 90):
            for y in range(20, 60):
                w.remove(x, y, 30)
        if c.patch_box(w, (40, 20, 30), (89, 59, 30)) is None:
            c.upload_octree(*w.flatten())
        c._L.vrt_stream_write_flag(c._h, C.c_void_p(flag), 1, None)
        c._L.vrt_stream_wait_flag(c._h, C.c_void_p(flag), 1, C.c_void_p(sp))
        c.shade_rays_device(n, d_o, 3, d_d, d_rgba, d_id, mode=1, stream=sp)
        side.synchronize()
        rgba = c.device_read(d_rgba, (n, 4), np.uint8, stream=sp)
        tex2, dim2 = w.flatten()
        ref = oracle_rays.shade(R, _oracle_scene(O, V, tex2, dim2), o, d, 1)
        _same(rgba, ref[0], "device form after a patch")
        assert not np.array_equal(rgba, before), "the patch changed no ray"
    finally:
        for p in bufs:
            c.device_free(p)
        c.close()
        w.close()


# ---- 7. error codes ----

def test_error_codes(V, product_scenes):
    INVALID, STATE = -1, -5
    c = V.Context(0)
    L = c._L
    o = np.zeros((4, 3), F)
    d = np.ones((4, 3), F)
    rgba = np.zeros((4, 4), np.uint8)
    idd = np.zeros((4, 2), np.int32)
    op, dp, rp, ip = o.ctypes.data, d.ctypes.data, rgba.ctypes.data, idd.ctypes.data

    def host(n=4, origins=op, stride=3, dirs=dp, width=4, mode=2, first=0, n_samples=1, out_rgba=rp, out_id=ip):
        return L.vrt_shade_rays(c._h, n, origins, stride, dirs, width, mode, first, n_samples, out_rgba, out_id)

    def device(n=4, origins=op, stride=3, dirs=dp, width=4, mode=2, first=0, n_samples=1, out_rgba=rp, out_id=ip):
        return L.vrt_shade_rays_device(c._h, n, origins, stride, dirs, width, mode, first, n_samples, out_rgba, out_id, None)

    try:
        assert host() == STATE and device() == STATE                          # before any upload
        c.upload_octree(*product_scenes["monu9"])
        for call in (host, device):
            assert call(origins=None) == INVALID and call(dirs=None) == INVALID      # NULL inputs with n > 0
            assert call(out_rgba=None, out_id=None) == INVALID                       # both outputs NULL
            assert call(stride=1) == INVALID and call(stride=-3) == INVALID and call(stride=6) == INVALID
            assert call(mode=3) == INVALID and call(mode=-1) == INVALID and call(mode=6) == INVALID
            assert call(width=0) == INVALID and call(width=-5) == INVALID
            assert call(n_samples=0) == INVALID and call(n_samples=(1 << 24) + 1) == INVALID
            assert call(n=(1 << 30) + 1) == INVALID
            assert call(n=0) == 0 and call(n=0, origins=None, dirs=None) == 0        # n == 0 does nothing
        assert host(out_rgba=None) == 0 and host(out_id=None) == 0 and host(n_samples=1 << 24, mode=0) == 0
        assert host(width=2 ** 31 - 1) == 0
        assert b"shade_rays" in L.vrt_last_error(c._h)
        c.patch_begin()
        assert host() == STATE and device() == STATE                          # while a patch batch is open
        c.patch_end()
        assert host() == 0
        with pytest.raises(V.VrtError):
            c.shade_rays(o, d, mode=7)
    finally:
        c.close()


# ---- 8. unusable rays leave the others alone ----

def test_zero_nan_and_infinite_rays_change_no_other_ray(ctx, V, O, R, product_scenes):
    """Runs once. A zero, infinite or NaN direction or origin gives an unspecified result for that ray only: the call returns and
    every other ray of the batch has the bytes it has without them."""
    tex, dim = product_scenes["dragon"]
    ctx.upload_octree(tex, dim)
    _params(ctx)
    o, d = _ray_mix(np.random.default_rng(20), 1024, (0, 0, 0), (126, 95, 60), ((40, 2, 20), (80, 6, 40)), ((50, 1, 25), (70, 4, 35)))
    bad = np.arange(5, 1024, 37)
    ob, db = o.copy(), d.copy()
    poison = [(0.0, 0.0, 0.0), (np.nan, 1.0, 0.0), (np.inf, 0.0, 0.0), (-np.inf, np.inf, 1.0), (np.nan, np.nan, np.nan)]
    for j, i in enumerate(bad):
        if j % 2 == 0:
            db[i] = poison[(j // 2) % len(poison)]
        else:
            ob[i] = poison[1 + (j // 2) % (len(poison) - 1)]
    good = np.ones(1024, bool)
    good[bad] = False
    for mode, n_samples in ((0, 1), (1, 1), (2, 1), (2, 3)):
        want = ctx.shade_rays(o, d, mode, width=64, n_samples=n_samples)
        got = ctx.shade_rays(ob, db, mode, width=64, n_samples=n_samples)
        _same(got[0][good], want[0][good], f"mode {mode} x{n_samples} rgba8 of the usable rays")
        _same(got[1][good], want[1][good], f"mode {mode} x{n_samples} id_dist of the usable rays")
