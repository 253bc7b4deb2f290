"""vrt_shade_rays_hdr / vrt_shade_rays_hdr_device on the MI355X, bit for bit: the float mean, the tone-mapped bytes and id_dist
against the checker (tests/oracle_rays_hdr.c with tests/oracle_hdr.c's arithmetic) for arbitrary rays in three worlds, every
batch shape, and against the library itself -- vrt_shade_rays, the HDR accumulation's resolve, 3 + 5 samples through d_sums
against 8 at once; every route gives the same bits, nothing else of the context changes, the error codes, and one batch with
unusable rays."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_rays
import oracle_rays_hdr
from conftest import MAPS, random_voxels
from test_gpu_shade_rays import SCENES, _materials_world, _most_hit_voxels, _oracle_scene, _params, _ray_mix

pytestmark = pytest.mark.gpu
F = np.float32
MODES = (0, 1, 2)
WRAP = 2 ** 32 - 2
TONEMAPS = (("clamp", 1.0), ("clamp", 0.25), ("reinhard", 1.0), ("reinhard", 0.25))
DRAGON_MIX = ((0, 0, 0), (126, 95, 60), ((40, 2, 20), (80, 6, 40)), ((50, 1, 25), (70, 4, 35)))


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_rays"))


@pytest.fixture(scope="module")
def RH(tmp_path_factory):
    return oracle_rays_hdr.build(tmp_path_factory.mktemp("oracle_rays_hdr"))


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.dtype.kind == "f":
        got, ref = _bits(got), _bits(ref)
    if not np.array_equal(got, ref):
        bad = np.argwhere(np.any(got != ref, axis=-1))[:, 0]
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(ref)} rays differ; first ray {i}: got {got[i]} want {ref[i]}")


class Checker:
    """the checker's samples of one batch, each traced once, and what a call makes of them"""

    def __init__(self, RH, s, o, d, width):
        self.RH, self.s, self.o, self.d, self.width = RH, s, o, d, width
        self.memo = {}

    def sample(self, mode, k):
        key = (mode, k & 0xFFFFFFFF if mode == 2 else 0)
        if key not in self.memo:
            self.memo[key] = oracle_rays_hdr.shade(self.RH, self.s, self.o, self.d, mode, self.width, key[1])
        return self.memo[key]

    def call(self, mode, first, n, sums=None, n_prior=0):
        """-> (sums float64[n,3], mean float32[n,3], id_dist)"""
        RH = self.RH
        sums = np.zeros((len(self.d), 3), np.float64) if sums is None else sums.copy()
        if mode == 2:
            for k in range(n):
                rgb = self.sample(2, first + k)[0]
                RH.o_hdr_add(sums.ctypes.data, rgb.ctypes.data, None, rgb.size)
        else:
            rgb = self.sample(mode, 0)[0]
            sums = sums + np.array([RH.o_hdr_product(C.c_float(v.item()), n) for v in rgb.ravel()], np.float64).reshape(rgb.shape)
        counts = np.full(len(self.d), n_prior + n, np.uint32)
        mean = np.zeros(sums.shape, np.float32)
        RH.o_hdr_mean(sums.ctypes.data, counts.ctypes.data, counts.size, mean.ctypes.data)
        return sums, mean, self.sample(mode, first)[1]


def _check(ctx, ck, what, modes=MODES, counts=(1, 2, 5, 8), firsts=(0, WRAP), tonemaps=TONEMAPS, origins=None):
    peak = 0.0
    for mode in modes:
        for first in firsts:
            for n in counts:
                _, mean, idd = ck.call(mode, first, n)
                peak = max(peak, float(np.nanmax(mean)))
                for op, e in tonemaps:
                    rgb, rgba, got_id = ctx.shade_rays_hdr(ck.o if origins is None else origins, ck.d, mode, width=ck.width,
                                                           first_sample=first, n_samples=n, tonemap=op, exposure=e)
                    tag = f"{what} mode {mode} first {first} n {n} {op} x{e}"
                    _same(rgb, mean, tag + " rgb")
                    _same(rgba, oracle_rays_hdr.tonemap(ck.RH, mean, op, e), tag + " rgba8")
                    _same(got_id, idd, tag + " id_dist")
    return peak


# ---- 1. arbitrary rays against the checker ----

def test_arbitrary_rays_on_the_dragon(ctx, V, O, RH, product_scenes):
    tex, dim = product_scenes["dragon"]
    ctx.upload_octree(tex, dim)
    _params(ctx)
    o, d = _ray_mix(np.random.default_rng(31), 2500, *DRAGON_MIX)
    _check(ctx, Checker(RH, _oracle_scene(O, V, tex, dim), o, d, 64), "dragon")


def test_arbitrary_rays_in_the_room(ctx, V, O, RH, product_scenes):
    tex, dim = product_scenes["room"]
    ctx.upload_octree(tex, dim)
    _params(ctx)
    o, d = _ray_mix(np.random.default_rng(32), 2500, (0, 0, 0), (120, 64, 120), ((10, 20, 10), (20, 40, 20)), ((0, 0, 0), (120, 1, 120)))
    peak = _check(ctx, Checker(RH, _oracle_scene(O, V, tex, dim), o, d, 7), "room")
    assert peak > 1.0, "no mean above 1 in the room"


def test_arbitrary_rays_in_a_world_with_emitters_and_glass(ctx, V, O, RH):
    w = _materials_world(V)
    tex, dim = w.flatten()
    w.close()
    ctx.upload_octree(tex, dim)
    o, d = _ray_mix(np.random.default_rng(33), 3000, (0, 0, 0), (50, 24, 24), ((30, 2, 8), (36, 8, 14)), ((30, 2, 16), (36, 8, 22)))
    try:
        for scale, hl in ((1.0, (-1, -1, -1)), (2.0, (5, 0, 20))):
            _params(ctx, scale, hl)
            ck = Checker(RH, _oracle_scene(O, V, tex, dim, scale, hl), o if scale == 1.0 else o / F(scale), d, 64)
            peak = _check(ctx, ck, f"materials scale {scale}", counts=(1, 2, 5, 8) if scale == 1.0 else (5,))
            assert peak > 4.0, f"the emitters give no mean far above 1 (peak {peak})"
    finally:
        _params(ctx)


# ---- 2. batch shapes ----

def test_batch_shapes(ctx, V, O, R, RH, product_scenes):
    """lists of 1, 63, 64, 65, 1000 rays; images of 8 x 2 (the smallest on the tile path), 9 x 3 (partial tiles both ways), a
    96 x 64 frame, a width larger than n; both origin strides"""
    tex, dim = product_scenes["room"]
    m, _, _, pose = SCENES["room_outside"]
    ctx.upload_octree(tex, dim)
    _params(ctx)
    s = O.make_scene(tex, dim, *V.camera_block(pose[:3], pose[3], pose[4], 96, 64)[:3])
    fo, fd = oracle_rays.frame_rays(R, s, 96, 64)
    lo, ld = _ray_mix(np.random.default_rng(34), 1000, (0, 0, 0), (120, 64, 120), ((10, 20, 10), (20, 40, 20)), ((0, 0, 0), (120, 1, 120)))
    lists = [(lo[:n], ld[:n], w) for n, w in ((1, 1), (63, 63), (64, 7), (65, 65), (1000, 1), (1000, 5000))]
    images = [(fo[:16], fd[:16], 8), (fo[:27], fd[:27], 9), (fo[:30], fd[:30], 9), (fo, fd, 96)]
    for o, d, width in lists + images:
        _check(ctx, Checker(RH, s, o, d, width), f"{len(d)} rays width {width}", counts=(1, 3), firsts=(WRAP,), tonemaps=(("reinhard", 0.25),))
    for o, d, width in images:   # a frame's rays share their origin
        _check(ctx, Checker(RH, s, o, d, width), f"{len(d)} rays width {width} stride 0", counts=(1, 3), firsts=(0,),
               tonemaps=(("clamp", 1.0),), origins=o[0])
    for o, d, width in lists:    # a list from ONE origin is another batch: a checker of its own
        o0 = np.ascontiguousarray(np.tile(o[0], (len(d), 1)))
        _check(ctx, Checker(RH, s, o0, d, width), f"{len(d)} rays width {width} stride 0", counts=(1, 3), firsts=(0,),
               tonemaps=(("clamp", 1.0),), origins=o[0])


# ---- 3. against the library itself ----

def test_one_sample_without_a_tone_map_is_shade_rays(ctx, V, product_scenes):
    tex, dim = product_scenes["dragon"]
    ctx.upload_octree(tex, dim)
    _params(ctx)
    o, d = _ray_mix(np.random.default_rng(35), 2000, *DRAGON_MIX)
    n = len(d)
    for mode in MODES:
        for first in (0, 9, WRAP + 1):
            want = ctx.shade_rays(o, d, mode, width=64, first_sample=first)
            rgba, idd = np.zeros((n, 4), np.uint8), np.zeros((n, 2), np.int32)
            ctx._chk(ctx._L.vrt_shade_rays_hdr(ctx._h, n, o.ctypes.data, 3, d.ctypes.data, 64, mode, first, 1, None, None,
                                               rgba.ctypes.data, idd.ctypes.data))   # tm == NULL, no float output
            _same(rgba, want[0], f"mode {mode} first {first} rgba8")
            _same(idd, want[1], f"mode {mode} first {first} id_dist")
    for mode in (0, 1):
        one = ctx.shade_rays_hdr(o, d, mode, width=64)
        five = ctx.shade_rays_hdr(o, d, mode, width=64, first_sample=3, n_samples=5)
        for a, b, what in zip(one, five, ("rgb", "rgba8", "id_dist")):
            _same(a, b, f"mode {mode} 1 sample vs 5 {what}")


@pytest.mark.parametrize("name", ["dragon", "room_outside"])
def test_a_frames_rays_give_the_hdr_accumulations_resolve(ctx, V, O, R, product_scenes, name):
    m, _, _, pose = SCENES[name]
    W, H = 96, 64
    tex, dim = product_scenes[m]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    ctx.upload_octree(tex, dim)
    ctx.set_camera(ip, iv, cp)
    _params(ctx)
    o, d = oracle_rays.frame_rays(R, O.make_scene(tex, dim, ip, iv, cp), W, H)
    for mode in MODES:
        for first in (0, WRAP):
            ctx.accum_begin(W, H, first, mode=mode, hdr=True)
            assert ctx.accum_add(5) == 5
            for op, e in (("clamp", 1.0), ("reinhard", 0.25)):
                want_rgb, want_rgba, _ = ctx.accum_resolve_hdr(op, e)
                rgb, rgba, idd = ctx.shade_rays_hdr(o[0], d, mode, width=W, first_sample=first, n_samples=5, tonemap=op, exposure=e)
                _same(rgb, want_rgb.reshape(-1, 3), f"{name} mode {mode} first {first} rgb")
                _same(rgba, want_rgba.reshape(-1, 4), f"{name} mode {mode} first {first} {op} rgba8")
            _same(idd, ctx.accum_resolve()[1].reshape(-1, 2), f"{name} mode {mode} id_dist")


# ---- 4. progressive: 3 + 5 through d_sums is 8 at once ----

def test_three_plus_five_samples_through_the_sums_are_eight(V, O, RH):
    w = _materials_world(V)
    tex, dim = w.flatten()
    w.close()
    c = V.Context(0)
    o, d = _ray_mix(np.random.default_rng(36), 1500, (0, 0, 0), (50, 24, 24), ((30, 2, 8), (36, 8, 14)), ((30, 2, 16), (36, 8, 22)))
    n = len(d)
    bufs = [c.device_alloc(o.nbytes), c.device_alloc(d.nbytes), c.device_alloc(n * 24), c.device_alloc(n * 12), c.device_alloc(n * 4),
            c.device_alloc(n * 8)]
    d_o, d_d, d_sums, d_rgb, d_rgba, d_id = bufs
    try:
        c.upload_octree(tex, dim)
        c.device_write(d_o, o)
        c.device_write(d_d, d)
        ck = Checker(RH, _oracle_scene(O, V, tex, dim), o, d, 64)
        zero = np.zeros((n, 3), np.float64)
        for mode in MODES:
            for first in (4, WRAP):
                kw = dict(mode=mode, width=64, tonemap="reinhard", exposure=0.25)
                c.device_write(d_sums, zero)
                c.shade_rays_hdr_device(n, d_o, 3, d_d, d_rgb, d_rgba, d_id, d_sums, 0, first_sample=first, n_samples=8, **kw)
                whole = [c.device_read(d_sums, (n, 3), np.float64), c.device_read(d_rgb, (n, 3), F), c.device_read(d_rgba, (n, 4), np.uint8),
                         c.device_read(d_id, (n, 2), np.int32)]
                c.device_write(d_sums, zero)
                c.shade_rays_hdr_device(n, d_o, 3, d_d, None, None, None, d_sums, 0, first_sample=first, n_samples=3, **kw)   # the sums alone
                three = c.device_read(d_sums, (n, 3), np.float64)
                c.shade_rays_hdr_device(n, d_o, 3, d_d, d_rgb, d_rgba, d_id, d_sums, 3, first_sample=(first + 3) & 0xFFFFFFFF,
                                        n_samples=5, **kw)
                parts = [c.device_read(d_sums, (n, 3), np.float64), c.device_read(d_rgb, (n, 3), F), c.device_read(d_rgba, (n, 4), np.uint8),
                         c.device_read(d_id, (n, 2), np.int32)]
                tag = f"mode {mode} first {first}"
                for a, b, what in zip(parts, whole, ("sums", "rgb", "rgba8", "id_dist")):
                    _same(a, b, f"{tag} 3 + 5 vs 8 {what}")
                host = c.shade_rays_hdr(o, d, first_sample=first, n_samples=8, **kw)
                for a, b, what in zip(host, whole[1:], ("rgb", "rgba8", "id_dist")):
                    _same(a, b, f"{tag} host form {what}")
                s3, _, _ = ck.call(mode, first, 3)
                _same(three, s3, f"{tag} the checker's sums after 3")
                s8, m8, _ = ck.call(mode, first + 3, 5, sums=s3, n_prior=3)
                _same(parts[0], s8, f"{tag} the checker's sums after 3 + 5")
                _same(parts[1], m8, f"{tag} the checker's mean after 3 + 5")
                # without the sums the call starts at +0.0 and leaves the buffer alone
                c.shade_rays_hdr_device(n, d_o, 3, d_d, d_rgb, None, None, None, 0, first_sample=first, n_samples=8, **kw)
                _same(c.device_read(d_rgb, (n, 3), F), whole[1], f"{tag} no sums rgb")
                _same(c.device_read(d_sums, (n, 3), np.float64), parts[0], f"{tag} sums untouched")
    finally:
        for p in bufs:
            c.device_free(p)
        c.close()


# ---- 5. every route ----

def test_every_variant_option_upload_form_patch_and_compaction(V, O, RH, product_scenes):
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    tex, dim = w.flatten()
    c = V.Context(0)   # never has a camera set
    try:
        c.upload_octree(tex, dim)
        o, d = _ray_mix(np.random.default_rng(37), 1500, *DRAGON_MIX)
        counts = {0: 4, 1: 4, 2: 3}
        ck = Checker(RH, _oracle_scene(O, V, tex, dim), o, d, 64)
        refs = {mode: ck.call(mode, WRAP, counts[mode]) for mode in MODES}

        def check(what):
            for mode in MODES:
                rgb, rgba, idd = c.shade_rays_hdr(o, d, mode, width=64, first_sample=WRAP, n_samples=counts[mode], tonemap="reinhard")
                _same(rgb, refs[mode][1], f"{what} mode {mode} rgb")
                _same(rgba, oracle_rays_hdr.tonemap(RH, refs[mode][1], "reinhard", 1.0), f"{what} mode {mode} rgba8")
                _same(idd, refs[mode][2], f"{what} mode {mode} id_dist")
                one = c.shade_rays_hdr(o, d, mode, width=64, first_sample=WRAP)   # the one-sample kernels
                _same(one[0], ck.call(mode, WRAP, 1)[1], f"{what} mode {mode} one sample rgb")

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
        c.upload_octree(tex, dim)
        before = c.shade_rays_hdr(o, d, 1)[0]
        for x, y, z in _most_hit_voxels(c, o, d, 30):
            w.remove(x, y, z)
            if c.patch_voxel(w, x, y, z) is None:
                c.upload_octree(*w.flatten())
        tex2, dim2 = w.flatten()
        ck = Checker(RH, _oracle_scene(O, V, tex2, dim2), o, d, 64)
        refs = {mode: ck.call(mode, WRAP, counts[mode]) for mode in MODES}
        check("after a voxel patch")
        assert not np.array_equal(_bits(before), _bits(c.shade_rays_hdr(o, d, 1)[0])), "the edit changed no ray"
        c.compact()
        check("after compaction")
    finally:
        c.close()
        w.close()


def test_worlds_the_wide_layout_cannot_express(ctx, V, O, RH):
    """test_gpu_parity's fixtures: a world the root table refuses (record-array kernels) and a unit-size internal node
    (explicit-AABB kernels), under every variant"""
    xyz, rgba = random_voxels(np.random.default_rng(4), 5000, -60, 70)
    try:
        wmin, wmax = (-64,) * 3, (192,) * 3
        w = V.World(world_min=wmin, world_max=wmax)
        w.insert_many(xyz, rgba)
        tex, dim = w.flatten()
        w.close()
        ctx.upload_octree(tex, dim)
        _params(ctx, bounds=(wmin, wmax))
        o, d = _ray_mix(np.random.default_rng(38), 1500, (-60, -60, -60), (70, 70, 70), ((-10, -10, -10), (10, 10, 10)),
                        ((-30, -30, -30), (-20, -20, -20)))
        ck = Checker(RH, _oracle_scene(O, V, tex, dim, bounds=(wmin, wmax)), o, d, 7)
        for var in V.available_variants():
            ctx.set_variant(var)
            _check(ctx, ck, f"world {wmin} variant {var}", counts=(1, 3), firsts=(WRAP,), tonemaps=(("clamp", 1.0),))
        tx = lambda value, alpha: [value & 255, (value >> 8) & 255, (value >> 16) & 255, alpha]   # noqa: E731
        leaf = [200, 40, 90, 255, 255, 0, 0, 255]
        unit = (tx(1, 0x80) + tx(2, 0) + tx(3, 0x01) + tx(4, 0) + tx(5, 0x01) + tx(6, 0) + tx(7, 0x80) + tx(8 | 0x800000, 0) + leaf)
        tex = np.array(unit, np.uint8)
        ctx.set_variant(0)
        ctx.upload_octree(tex, 3)
        _params(ctx, bounds=((0, 0, 0), (8, 8, 8)))
        o, d = _ray_mix(np.random.default_rng(39), 1000, (0, 0, 0), (8, 8, 8), ((4, 4, 4), (5, 5, 5)), ((4, 4, 4), (5, 5, 5)))
        ck = Checker(RH, _oracle_scene(O, V, tex, 3, bounds=((0, 0, 0), (8, 8, 8))), o, d, 7)
        _check(ctx, ck, "unit internal node", counts=(1, 3), firsts=(WRAP,), tonemaps=(("clamp", 1.0),))
    finally:
        ctx.set_variant(0)
        _params(ctx)


# ---- 6. isolation ----

def test_nothing_else_of_the_context_changes(ctx, V, product_scenes):
    m, _, _, pose = SCENES["room_outside"]
    W, H = 96, 64
    tex, dim = product_scenes[m]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    ctx.upload_octree(tex, dim)
    ctx.set_camera(ip, iv, cp)
    _params(ctx)
    o, d = _ray_mix(np.random.default_rng(40), 1500, (0, 0, 0), (120, 64, 120), ((10, 20, 10), (20, 40, 20)), ((0, 0, 0), (120, 1, 120)))

    def hdr_batches():
        for mode, n in ((0, 4), (1, 1), (2, 1), (2, 3)):
            ctx.shade_rays_hdr(o, d, mode, width=7, first_sample=5, n_samples=n, tonemap="reinhard", exposure=0.25)

    frames = {mode: ctx.dispatch(W, H, mode) for mode in MODES}
    plain = {mode: ctx.shade_rays(o, d, mode, width=7, n_samples=3) for mode in MODES}
    ctx.accum_begin(W, H, 4, mode=2, hdr=True)
    assert ctx.accum_add(2) == 2 and ctx.accum_add(3) == 5
    ref = ctx.accum_resolve_hdr() + ctx.accum_resolve()
    hdr_batches()
    ctx.accum_begin(W, H, 4, mode=2, hdr=True)
    hdr_batches()
    assert ctx.accum_add(2) == 2
    hdr_batches()
    assert ctx.accum_add(3) == 5, "accum_add after shade_rays_hdr restarted the accumulation"
    hdr_batches()
    for a, b in zip(ctx.accum_resolve_hdr() + ctx.accum_resolve(), ref):
        _same(a.reshape(W * H, -1), b.reshape(W * H, -1), "the running HDR accumulation")
    for mode in MODES:
        rgba, idd = ctx.dispatch(W, H, mode)
        assert np.array_equal(rgba, frames[mode][0]) and np.array_equal(idd, frames[mode][1]), f"frame mode {mode} changed"
        hdr_batches()
        got = ctx.shade_rays(o, d, mode, width=7, n_samples=3)
        _same(got[0], plain[mode][0], f"vrt_shade_rays mode {mode} rgba8")
        _same(got[1], plain[mode][1], f"vrt_shade_rays mode {mode} id_dist")


def test_zero_nan_and_infinite_directions_change_no_other_ray(ctx, V, product_scenes):
    """Runs once. A zero, infinite or NaN direction gives an unspecified result for that ray only: the call returns and every
    other ray of the batch has the bits it has without them."""
    tex, dim = product_scenes["dragon"]
    ctx.upload_octree(tex, dim)
    _params(ctx)
    o, d = _ray_mix(np.random.default_rng(41), 1024, *DRAGON_MIX)
    bad = np.arange(5, 1024, 37)
    db = d.copy()
    poison = [(0.0, 0.0, 0.0), (np.nan, 1.0, 0.0), (np.inf, 0.0, 0.0), (-np.inf, np.inf, 1.0), (np.nan, np.nan, np.nan)]
    for j, i in enumerate(bad):
        db[i] = poison[j % len(poison)]
    good = np.ones(1024, bool)
    good[bad] = False
    for mode, n_samples in ((0, 1), (1, 4), (2, 1), (2, 3)):
        want = ctx.shade_rays_hdr(o, d, mode, width=64, n_samples=n_samples)
        got = ctx.shade_rays_hdr(o, db, mode, width=64, n_samples=n_samples)
        for a, b, what in zip(got, want, ("rgb", "rgba8", "id_dist")):
            _same(a[good], b[good], f"mode {mode} x{n_samples} {what} of the usable rays")


# ---- 7. error codes ----

def test_error_codes(V, product_scenes):
    INVALID, STATE = -1, -5
    c = V.Context(0)
    L = c._L
    o = np.zeros((4, 3), F)
    d = np.ones((4, 3), F)
    rgb = np.zeros((4, 3), F)
    rgba = np.zeros((4, 4), np.uint8)
    idd = np.zeros((4, 2), np.int32)
    op, dp, fp, rp, ip = o.ctypes.data, d.ctypes.data, rgb.ctypes.data, rgba.ctypes.data, idd.ctypes.data
    bufs = []

    def tm_of(op_, e):
        return C.byref(V.Tonemap(op_, e))

    def host(n=4, origins=op, stride=3, dirs=dp, width=4, mode=2, first=0, n_samples=1, tm=None, out_rgb=fp, out_rgba=rp, out_id=ip):
        return L.vrt_shade_rays_hdr(c._h, n, origins, stride, dirs, width, mode, first, n_samples, tm, out_rgb, out_rgba, out_id)

    try:
        assert host() == STATE                                                 # before any upload
        c.upload_octree(*product_scenes["monu9"])
        bufs = [c.device_alloc(48), c.device_alloc(48), c.device_alloc(96), c.device_alloc(48), c.device_alloc(16), c.device_alloc(32)]
        d_o, d_d, d_sums, d_rgb, d_rgba, d_id = bufs
        c.device_write(d_o, o)
        c.device_write(d_d, d)
        c.device_write(d_sums, np.zeros((4, 3), np.float64))

        def device(n=4, origins=d_o, stride=3, dirs=d_d, width=4, mode=2, first=0, n_samples=1, n_prior=0, sums=d_sums, tm=None,
                   out_rgb=d_rgb, out_rgba=d_rgba, out_id=d_id):
            return L.vrt_shade_rays_hdr_device(c._h, n, origins, stride, dirs, width, mode, first, n_samples, n_prior, sums, tm, out_rgb,
                                               out_rgba, out_id, None)

        for call in (host, device):
            assert call(origins=None) == INVALID and call(dirs=None) == INVALID      # NULL inputs with n > 0
            assert call(stride=1) == INVALID and call(stride=-3) == INVALID and call(stride=6) == INVALID
            assert call(mode=3) == INVALID and call(mode=-1) == INVALID and call(mode=6) == INVALID
            assert call(width=0) == INVALID and call(width=-5) == INVALID
            assert call(n_samples=0) == INVALID and call(n_samples=(1 << 24) + 1) == INVALID
            assert call(n=(1 << 30) + 1) == INVALID
            assert call(tm=tm_of(2, 1.0)) == INVALID and call(tm=tm_of(-1, 1.0)) == INVALID          # an unknown operator
            for e in (0.0, -1.0, float("nan"), float("inf")):
                assert call(tm=tm_of(0, e)) == INVALID and call(tm=tm_of(1, e)) == INVALID
            assert call(n=0) == 0 and call(n=0, origins=None, dirs=None) == 0        # n == 0 does nothing
            assert call(tm=tm_of(1, 0.25)) == 0 and call(n_samples=1 << 24, mode=0) == 0
            assert call(out_rgb=None, out_rgba=None) == 0 and call(out_rgba=None, out_id=None) == 0 and call(out_rgb=None, out_id=None) == 0
        assert host(out_rgb=None, out_rgba=None, out_id=None) == INVALID       # every output NULL
        assert device(out_rgb=None, out_rgba=None, out_id=None, sums=None) == INVALID
        assert device(out_rgb=None, out_rgba=None, out_id=None) == 0           # the sums alone are an output
        assert device(n_prior=1, sums=None) == INVALID                         # n_prior without sums
        assert device(n_prior=1 << 24) == INVALID and device(n_prior=(1 << 24) - 1, n_samples=2, mode=0) == INVALID
        assert device(n_prior=(1 << 24) - 2, n_samples=2, mode=0) == 0 and device(n_prior=0xFFFFFFFF, n_samples=1) == INVALID
        assert device(sums=None) == 0
        assert b"shade_rays_hdr" in L.vrt_last_error(c._h)
        c.device_read(d_rgba, (4, 4), np.uint8)                                # (waits for the calls enqueued above)
        c.patch_begin()
        assert host() == STATE and device() == STATE                           # while a patch batch is open
        c.patch_end()
        assert host() == 0
        with pytest.raises(V.VrtError):
            c.shade_rays_hdr(o, d, mode=7)
    finally:
        for p in bufs:
            c.device_free(p)
        c.close()
