"""Path depth (include/vrt.h vrt_set_path_depth) on the MI355X: the samples of VRT_MODE_FULL in accumulations and ray batches at
D in {1, 2, 3, 8}, byte for byte (HDR: bit for bit) against the checker (tests/oracle_paths.c through oracle_path_depth). Three worlds at 72 x 44 --
nine tiles across and a half tile at the bottom edge: the dragon (opaque: the two-pass routes), the room seen from inside (glass:
the general kernel) and the unit-internal stream (no wide layout: the record-array kernels). Every reference sample is computed
once per (world, ray source, D, sample) and shared."""
import os

import numpy as np
import pytest

import oracle_adaptive
import oracle_hdr
import oracle_lens
import oracle_path_depth as opd
import oracle_rays
from conftest import MAPS

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 72, 44
DEPTHS = (1, 2, 3, 8)
FIRST = 5
WORLDS = ("dragon", "room", "unit")
POSES = {"dragon": (63.5, 60.5, 140.5, -90.0, -10.0), "room": (14.5, 30.5, 16.5, 32.0, -10.0), "unit": (1.3, 2.1, 0.7, 52.0, 18.0)}
LENS = {"dragon": (0.8, 80.0), "room": (0.7, 30.0), "unit": (0.05, 3.0)}   # aperture, focus distance
SOURCES = {"corner": (False, False), "jitter": (True, False), "lens": (False, True), "lens+jitter": (True, True)}   # jitter, lens
UNIT_BOUNDS = ((0, 0, 0), (8, 8, 8))


def _tx(value, alpha):
    return [value & 255, (value >> 8) & 255, (value >> 16) & 255, alpha]


def _unit_stream():
    """test_gpu_parity's hand-written stream whose unit cell [4,5)^3 is still an internal node: no wide layout, the explicit-AABB kernels"""
    leaf = [200, 40, 90, 255, 255, 0, 0, 255]
    return np.array(_tx(1, 0x80) + _tx(2, 0) + _tx(3, 0x01) + _tx(4, 0) + _tx(5, 0x01) + _tx(6, 0) + _tx(7, 0x80) + _tx(8 | 0x800000, 0) + leaf,
                    np.uint8), 3


class Refs:
    """The checker's side: scenes, each sample's rays and each sample's result, computed once"""

    def __init__(self, tmp, O, V, product_scenes):
        self.P = opd.build(tmp)
        self.R = oracle_rays.build(tmp)
        self.LL = oracle_lens.build(tmp)
        self.HH = oracle_hdr.build(tmp)
        self.V = V
        self.world = {}
        for name in WORLDS:
            tex, dim = _unit_stream() if name == "unit" else product_scenes[name]
            pose = POSES[name]
            ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
            s = O.make_scene(tex, dim, ip, iv, cp)
            if name == "unit":
                s.bounds_min[:] = UNIT_BOUNDS[0]
                s.bounds_max[:] = UNIT_BOUNDS[1]
            self.world[name] = (tex, dim, (ip, iv, cp), s)
        self._rays = {}
        self._samples = {}

    def rays(self, world, source, k):
        """the rays of sample k of the accumulation's source: the frame's from the corner, oracle_lens's otherwise"""
        jitter, lens = SOURCES[source]
        key = (world, source, k if (jitter or lens) else 0)
        if key not in self._rays:
            s = self.world[world][3]
            if not jitter and not lens:
                self._rays[key] = oracle_rays.frame_rays(self.R, s, W, H)
            else:
                ap, fo = LENS[world] if lens else (0.0, 1.0)
                o = np.zeros((H * W, 3), F)
                d = np.zeros((H * W, 3), F)
                for py in range(H):
                    for px in range(W):
                        _, o[py * W + px], d[py * W + px] = oracle_lens.ray(self.LL, s, W, H, px, py, k, ap, fo, jitter)
                self._rays[key] = (o, d)
        return self._rays[key]

    def sample(self, world, source, D, k):
        """-> (rgba8[H*W,4], id_dist[H*W,2], rgb float32[H*W,3]) of sample k"""
        key = (world, source, D, k)
        if key not in self._samples:
            o, d = self.rays(world, source, k)
            self._samples[key] = opd.shade(self.P, self.world[world][3], o, d, D, width=W, sample=k)
        return self._samples[key]

    def mean(self, world, source, D, first, n):
        total = sum(self.sample(world, source, D, first + k)[0].astype(np.uint64) for k in range(n))
        out = ((total + n // 2) // n).astype(np.uint8)
        out[:, 3] = 255
        return out.reshape(H, W, 4)

    def frame_id(self, world):
        """the resolved (voxel ID, dist): the unjittered pinhole frame's, at any depth"""
        return self.sample(world, "corner", 1, 0)[1].reshape(H, W, 2)


@pytest.fixture(scope="module")
def refs(tmp_path_factory, O, V, product_scenes):
    return Refs(tmp_path_factory.mktemp("oracle_path_depth"), O, V, product_scenes)


def _load(c, refs, world, depth=None):
    tex, dim, cam, _ = refs.world[world]
    c.upload_octree(tex, dim)
    c.set_camera(*cam)
    p = c.default_params()
    if world == "unit":
        p.world_min[:] = UNIT_BOUNDS[0]
        p.world_max[:] = UNIT_BOUNDS[1]
    c.set_params(p)
    c.set_variant(0)
    c.set_lens(0.0, 1.0)
    if depth is not None:
        c.set_path_depth(depth)


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} against {ref.shape}"
    if not np.array_equal(got, ref):
        g, r = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
        bad = np.argwhere(np.any(g != r, axis=-1))[:, 0]
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(r)} differ; first at {i} (x {i % W}, y {i // W}): got {g[i]} want {r[i]}")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _begin(c, world, source, **kw):
    jitter, lens = SOURCES[source]
    c.set_lens(*(LENS[world] if lens else (0.0, 1.0)))
    c.accum_begin(W, H, FIRST, mode=2, jitter=jitter, **kw)


# ---- the accumulation ----

@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("world", WORLDS)
def test_accumulation_is_the_checkers_mean(ctx, refs, world, source, D):
    _load(ctx, refs, world, D)
    try:
        _begin(ctx, world, source)
        assert ctx.accum_add(1) == 1 and ctx.accum_add(3) == 4
        split = ctx.accum_resolve()
        _begin(ctx, world, source)
        assert ctx.accum_add(4) == 4
        once = ctx.accum_resolve()
        what = f"{world} {source} D={D}"
        _same(split[0], refs.mean(world, source, D, FIRST, 4), f"{what} add(1) + add(3) rgba8")
        _same(once[0], split[0], f"{what} add(4) against add(1) + add(3) rgba8")
        _same(split[1], refs.frame_id(world), f"{what} id_dist")
        _same(once[1], split[1], f"{what} add(4) id_dist")
    finally:
        ctx.set_lens(0.0, 1.0)
        ctx.set_path_depth(1)


@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_full_opaque_off_gives_the_same_bytes_on_the_dragon(ctx, V, refs, source, D):
    _load(ctx, refs, "dragon", D)
    try:
        out = {}
        for on in (1, 0):
            ctx.set_option(V.OPT_FULL_OPAQUE, 6 if on else 0)
            _begin(ctx, "dragon", source)
            ctx.accum_add(2)
            out[on] = ctx.accum_resolve()
        _same(out[1][0], refs.mean("dragon", source, D, FIRST, 2), f"{source} D={D} opaque route rgba8")
        _same(out[0][0], out[1][0], f"{source} D={D} VRT_OPT_FULL_OPAQUE off against on rgba8")
        _same(out[0][1], out[1][1], f"{source} D={D} VRT_OPT_FULL_OPAQUE off against on id_dist")
    finally:
        ctx.set_option(V.OPT_FULL_OPAQUE, 6)
        ctx.set_lens(0.0, 1.0)
        ctx.set_path_depth(1)


@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("world", WORLDS)
def test_every_variant_gives_the_same_bytes(ctx, V, refs, world, D):
    _load(ctx, refs, world, D)
    o, d = refs.rays(world, "corner", 0)
    try:
        for v in V.available_variants():
            ctx.set_variant(v)
            for source in ("corner", "lens+jitter"):
                _begin(ctx, world, source)
                ctx.accum_add(2)
                got = ctx.accum_resolve()
                _same(got[0], refs.mean(world, source, D, FIRST, 2), f"{world} D={D} variant {v} {source} rgba8")
                _same(got[1], refs.frame_id(world), f"{world} variant {v} {source} id_dist")
            rgba, idd = ctx.shade_rays(o, d, 2, width=W, first_sample=FIRST, n_samples=2)
            _same(rgba.reshape(H, W, 4), refs.mean(world, "corner", D, FIRST, 2), f"{world} D={D} variant {v} shade_rays rgba8")
            _same(idd.reshape(H, W, 2), refs.frame_id(world), f"{world} variant {v} shade_rays id_dist")
    finally:
        ctx.set_variant(0)
        ctx.set_lens(0.0, 1.0)
        ctx.set_path_depth(1)


def test_record_uploads_take_the_depth(V, refs):
    """vrt_upload_records: a context without the texel stream"""
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    c = V.Context(0)
    try:
        c.upload_records(*w.records())
        c.set_camera(*refs.world["dragon"][2])
        c.set_path_depth(3)
        c.accum_begin(W, H, FIRST, mode=2)
        c.accum_add(2)
        _same(c.accum_resolve()[0], refs.mean("dragon", "corner", 3, FIRST, 2), "record upload rgba8")
    finally:
        c.close()
        w.close()


@pytest.mark.parametrize("world,source", [("dragon", "corner"), ("dragon", "jitter"), ("room", "corner"), ("room", "lens"), ("unit", "corner")])
def test_adaptive_rounds_follow_the_rule_on_the_checkers_samples(ctx, refs, world, source):
    rule = (2, 6, 3)
    _load(ctx, refs, world, 3)
    try:
        _begin(ctx, world, source, adaptive=rule)
        assert ctx.accum_add(2) == 2 and ctx.accum_add(4) == 6
        got = ctx.accum_resolve()
        counts, active = ctx.accum_counts()
        st = oracle_adaptive.accumulate(lambda k: refs.sample(world, source, 3, k)[0].reshape(H, W, 4), H, W, FIRST, 6, rule, np.int64)
        assert np.array_equal(counts, st.counts()), f"{world} {source}: counts"
        assert active == int(st.active(rule).sum())
        assert counts.min() >= 2 and counts.max() <= 6
        _same(got[0], st.resolve(), f"{world} {source} adaptive rgba8")
        _same(got[1], refs.frame_id(world), f"{world} {source} adaptive id_dist")
    finally:
        ctx.set_lens(0.0, 1.0)
        ctx.set_path_depth(1)


@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("source", ("corner", "lens+jitter"))
@pytest.mark.parametrize("world", WORLDS)
def test_hdr_means_match_the_checkers_floats_bit_for_bit(ctx, refs, world, source, D):
    _load(ctx, refs, world, D)
    try:
        _begin(ctx, world, source, hdr=True)
        assert ctx.accum_add(1) == 1 and ctx.accum_add(2) == 3
        acc = oracle_hdr.Accum(refs.HH, H, W)
        for k in range(3):
            acc.add(refs.sample(world, source, D, FIRST + k)[2].reshape(H, W, 3))
        want = acc.mean()
        for op, e in (("clamp", 1.0), ("reinhard", 1.7)):
            rgb, rgba, _ = ctx.accum_resolve_hdr(op, e)
            _same(_bits(rgb), _bits(want), f"{world} {source} D={D} float mean ({op})")
            _same(rgba, oracle_hdr.tonemap(refs.HH, want, op, e), f"{world} {source} D={D} {op} bytes")
        _same(ctx.accum_resolve()[0], refs.mean(world, source, D, FIRST, 3), f"{world} {source} D={D} the bytes beside the floats")
    finally:
        ctx.set_lens(0.0, 1.0)
        ctx.set_path_depth(1)


@pytest.mark.parametrize("D", (3, 8))
@pytest.mark.parametrize("world,source", [("dragon", "corner"), ("dragon", "jitter"), ("dragon", "lens"), ("room", "corner"), ("room", "lens+jitter"),
                                          ("unit", "corner")])
def test_adaptive_hdr_accumulations_follow_the_same_pixels(ctx, refs, world, source, D):
    """adaptive and HDR together: the rule on the bytes, the float64 sums taking the samples of the pixels the rule keeps active"""
    rule = (2, 5, 3)
    _load(ctx, refs, world, D)
    try:
        _begin(ctx, world, source, adaptive=rule, hdr=True)
        assert ctx.accum_add(2) == 2 and ctx.accum_add(3) == 5
        acc = oracle_hdr.Accum(refs.HH, H, W, rule)
        for k in range(5):
            acc.add(refs.sample(world, source, D, FIRST + k)[2].reshape(H, W, 3))
        counts, _ = ctx.accum_counts()
        assert np.array_equal(counts, acc.counts()), f"{world} {source} D={D}: counts"
        want = acc.mean()
        rgb, rgba, _ = ctx.accum_resolve_hdr("reinhard", 1.7)
        _same(_bits(rgb), _bits(want), f"{world} {source} D={D} adaptive float mean")
        _same(rgba, oracle_hdr.tonemap(refs.HH, want, "reinhard", 1.7), f"{world} {source} D={D} adaptive reinhard bytes")
        _same(ctx.accum_resolve()[0], acc.resolve_bytes(), f"{world} {source} D={D} adaptive bytes beside the floats")
    finally:
        ctx.set_lens(0.0, 1.0)
        ctx.set_path_depth(1)


@pytest.mark.parametrize("pose,size", [((34.0, 60.0, 34.0, -90.0, 0.0), (64, 36)), ((20.0, 30.0, 20.0, 0.0, 0.0), (40, 40))])
def test_axis_parallel_cameras_on_the_dragon(ctx, V, O, refs, pose, size):
    """test_gpu_parity's degenerate cameras -- on voxel boundaries, the middle row and column axis-parallel, zero-length steps and
    zero direction components at the depth-0 hit (the normal of comp:497) -- at D = 3 and 8, VRT_OPT_FULL_OPAQUE on against off"""
    w, h = size
    tex, dim = refs.world["dragon"][:2]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], w, h)
    s = O.make_scene(tex, dim, ip, iv, cp)
    o, d = oracle_rays.frame_rays(refs.R, s, w, h)
    _load(ctx, refs, "dragon")
    ctx.set_camera(ip, iv, cp)
    try:
        for D in (3, 8):
            ctx.set_path_depth(D)
            want, _ = opd.mean(refs.P, s, o, d, D, width=w, first_sample=FIRST, n_samples=2)
            for on in (1, 0):
                ctx.set_option(V.OPT_FULL_OPAQUE, 6 if on else 0)
                ctx.accum_begin(w, h, FIRST, mode=2)
                ctx.accum_add(2)
                got = ctx.accum_resolve()[0]
                assert np.array_equal(got, want.reshape(h, w, 4)), f"pose {pose} D={D} VRT_OPT_FULL_OPAQUE {on}"
    finally:
        ctx.set_option(V.OPT_FULL_OPAQUE, 6)
        ctx.set_path_depth(1)


# ---- ray batches ----

def _arbitrary_rays(world, n=256):
    """origins in empty space, in glass and in solids, all inside the world; a third of the directions axis-parallel"""
    rng = np.random.default_rng(31)
    boxes = {"dragon": [((0, 0, 0), (126, 95, 60)), ((40, 2, 20), (80, 6, 40)), ((50, 1, 25), (70, 4, 35))],
             "room": [((1, 1, 1), (119, 63, 119)), ((10, 20, 10), (20, 40, 20)), ((0, 0, 0), (120, 1, 120))],
             "unit": [((0.1, 0.1, 0.1), (7.9, 7.9, 7.9)), ((4, 4, 4), (5, 5, 5)), ((4, 4, 4), (5, 5, 5))]}[world]
    o = np.empty((n, 3), np.float64)
    for i in range(n):
        lo, hi = (np.asarray(v, np.float64) for v in boxes[i % 3])
        o[i] = lo + rng.random(3) * (hi - lo)
    lo, hi = (np.asarray(v, np.float64) for v in boxes[0])
    d = lo + rng.random((n, 3)) * (hi - lo) - o
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)
    for i in range(0, n, 3):
        a = int(rng.integers(0, 3))
        s = np.sign(d[i, a]) or 1.0
        d[i] = 0.0
        d[i, a] = s
    return o.astype(F), d.astype(F)


@pytest.fixture(scope="module")
def batches(refs):
    """world -> (origins, dirs): the frame's rays, then 256 arbitrary ones; and the checker's samples of it per (D, k)"""
    out = {}
    for world in WORLDS:
        fo, fd = refs.rays(world, "corner", 0)
        ao, ad = _arbitrary_rays(world)
        out[world] = (np.concatenate([fo, ao]), np.concatenate([fd, ad]), {})
    return out


def _batch_sample(refs, batches, world, D, k):
    o, d, cache = batches[world]
    if (D, k) not in cache:
        cache[(D, k)] = opd.shade(refs.P, refs.world[world][3], o, d, D, width=W, sample=k)
    return cache[(D, k)]


def _batch_mean(refs, batches, world, D, first, n):
    total = sum(_batch_sample(refs, batches, world, D, first + k)[0].astype(np.uint64) for k in range(n))
    out = ((total + n // 2) // n).astype(np.uint8)
    out[:, 3] = 255
    return out


@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("world", WORLDS)
def test_ray_batches_host_and_device_forms(ctx, refs, batches, world, D):
    import torch
    _load(ctx, refs, world, D)
    o, d, _ = batches[world]
    n = o.shape[0]
    try:
        t_o = torch.from_numpy(o).cuda()
        t_d = torch.from_numpy(d).cuda()
        t_rgba = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
        t_id = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for ns in (1, 4):
            want = _batch_mean(refs, batches, world, D, FIRST, ns)
            want_id = _batch_sample(refs, batches, world, D, FIRST)[1]
            rgba, idd = ctx.shade_rays(o, d, 2, width=W, first_sample=FIRST, n_samples=ns)
            _same(rgba, want, f"{world} D={D} n_samples={ns} host rgba8")
            _same(idd, want_id, f"{world} D={D} n_samples={ns} host id_dist")
            ctx.shade_rays_device(n, t_o.data_ptr(), 3, t_d.data_ptr(), t_rgba.data_ptr(), t_id.data_ptr(), 2, width=W, first_sample=FIRST,
                                  n_samples=ns)
            ctx.synchronize()
            _same(t_rgba.cpu().numpy(), want, f"{world} D={D} n_samples={ns} device rgba8")
            _same(t_id.cpu().numpy(), want_id, f"{world} D={D} n_samples={ns} device id_dist")
    finally:
        ctx.set_path_depth(1)


@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("world", WORLDS)
def test_ray_batches_hdr_with_caller_sums(ctx, refs, batches, world, D):
    """3 + 5 samples through the caller's sums equal 8 in one call, bit for bit, and both equal the checker's floats summed in
    float64 in sample order (tests/oracle_hdr.c's arithmetic)"""
    import torch
    _load(ctx, refs, world, D)
    o, d, _ = batches[world]
    n = o.shape[0]
    try:
        sums = np.zeros((n, 3), np.float64)
        for k in range(8):
            rgb = np.ascontiguousarray(_batch_sample(refs, batches, world, D, FIRST + k)[2])
            refs.HH.o_hdr_add(sums.ctypes.data, rgb.ctypes.data, None, rgb.size)
        want = np.zeros((n, 3), F)
        counts = np.full(n, 8, np.uint32)
        refs.HH.o_hdr_mean(sums.ctypes.data, counts.ctypes.data, n, want.ctypes.data)
        t_o = torch.from_numpy(o).cuda()
        t_d = torch.from_numpy(d).cuda()
        got = {}
        for parts in ((3, 5), (8,)):
            t_sums = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
            t_rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
            t_rgba = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            prior = 0
            for ns in parts:
                ctx.shade_rays_hdr_device(n, t_o.data_ptr(), 3, t_d.data_ptr(), t_rgb.data_ptr(), t_rgba.data_ptr(), None, t_sums.data_ptr(),
                                          n_prior=prior, mode=2, width=W, first_sample=FIRST + prior, n_samples=ns, tonemap="reinhard",
                                          exposure=1.7)
                prior += ns
            ctx.synchronize()
            got[parts] = (t_sums.cpu().numpy(), t_rgb.cpu().numpy(), t_rgba.cpu().numpy())
        for parts, (g_sums, g_rgb, g_rgba) in got.items():
            _same(g_sums.view(np.uint64), sums.view(np.uint64), f"{world} D={D} {parts} float64 sums")
            _same(_bits(g_rgb), _bits(want), f"{world} D={D} {parts} float mean")
            _same(g_rgba, oracle_hdr.tonemap(refs.HH, want[None], "reinhard", 1.7)[0], f"{world} D={D} {parts} reinhard bytes")
        rgb, rgba, idd = ctx.shade_rays_hdr(o, d, 2, width=W, first_sample=FIRST, n_samples=8)
        _same(_bits(rgb), _bits(want), f"{world} D={D} host form float mean")
        _same(idd, _batch_sample(refs, batches, world, D, FIRST)[1], f"{world} D={D} host form id_dist")
    finally:
        ctx.set_path_depth(1)


@pytest.mark.parametrize("world", WORLDS)
def test_the_accumulations_lens_samples_are_shade_rays_on_the_same_rays(ctx, refs, world):
    _load(ctx, refs, world, 3)
    try:
        for k in (FIRST, FIRST + 2):
            o, d = refs.rays(world, "lens+jitter", k)
            ctx.set_lens(*LENS[world])
            ctx.accum_begin(W, H, k, mode=2, jitter=True)
            ctx.accum_add(1)
            acc = ctx.accum_resolve()[0]
            rgba, _ = ctx.shade_rays(o, d, 2, width=W, first_sample=k)
            _same(rgba.reshape(H, W, 4), acc, f"{world} lens sample {k}: shade_rays against the accumulation")
            _same(acc, refs.sample(world, "lens+jitter", 3, k)[0].reshape(H, W, 4), f"{world} lens sample {k} against the checker")
    finally:
        ctx.set_lens(0.0, 1.0)
        ctx.set_path_depth(1)


# ---- the setting itself ----

def _everything(c, refs, batches, world):
    """every output the depth reaches, at the context's current setting"""
    o, d, _ = batches[world]
    out = []
    for source in sorted(SOURCES):
        _begin(c, world, source)
        c.accum_add(2)
        out += list(c.accum_resolve())
    _begin(c, world, "corner", adaptive=(2, 4, 3))
    c.accum_add(4)
    out += list(c.accum_resolve()) + [c.accum_counts()[0]]
    _begin(c, world, "jitter", hdr=True)
    c.accum_add(2)
    out += [_bits(c.accum_resolve_hdr()[0])]
    c.set_lens(0.0, 1.0)
    out += list(c.shade_rays(o, d, 2, width=W, first_sample=FIRST, n_samples=1))
    out += list(c.shade_rays(o, d, 2, width=W, first_sample=FIRST, n_samples=3))
    rgb, rgba, idd = c.shade_rays_hdr(o, d, 2, width=W, first_sample=FIRST, n_samples=2)
    out += [_bits(rgb), rgba, idd]
    return out


@pytest.mark.parametrize("world", WORLDS)
def test_depth_1_set_explicitly_is_a_context_that_never_called_the_setter(V, refs, batches, world):
    fresh = V.Context(0)
    setter = V.Context(0)
    try:
        _load(fresh, refs, world)
        _load(setter, refs, world, 1)
        a = _everything(fresh, refs, batches, world)
        b = _everything(setter, refs, batches, world)
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            _same(y, x, f"{world} output {i} at D = 1 set explicitly")
        setter.set_path_depth(4)
        setter.set_path_depth(1)   # ... and after a detour
        for i, (x, y) in enumerate(zip(a, _everything(setter, refs, batches, world))):
            _same(y, x, f"{world} output {i} at D = 1 set again")
    finally:
        fresh.close()
        setter.close()


@pytest.mark.parametrize("world", WORLDS)
def test_frames_stay_the_shader(ctx, refs, world):
    _load(ctx, refs, world, 1)
    try:
        before = ctx.dispatch(W, H, 2)
        shown = ctx.dispatch_frame(W, H, 2)
        ctx.set_path_depth(3)
        after = ctx.dispatch(W, H, 2)
        _same(after[0], before[0], f"{world} vrt_dispatch mode 2 rgba8 after set_path_depth(3)")
        _same(after[1], before[1], f"{world} vrt_dispatch mode 2 id_dist after set_path_depth(3)")
        for x, y in zip(ctx.dispatch_frame(W, H, 2), shown):
            _same(x, y, f"{world} fused frame after set_path_depth(3)")
        _same(before[0], refs.sample(world, "corner", 1, 0)[0].reshape(H, W, 4), f"{world} the frame is the checker at D = 1, sample 0")
        # the consequence the header states: sample 0 of an unjittered accumulation at D > 1 is no longer the frame
        ctx.accum_begin(W, H, 0, mode=2)
        ctx.accum_add(1)
        s0 = ctx.accum_resolve()[0]
        _same(s0, refs.sample(world, "corner", 3, 0)[0].reshape(H, W, 4), f"{world} sample 0 at D = 3")
        if world != "unit":
            assert not np.array_equal(s0, before[0])
        for mode in (0, 1):   # the primary modes ignore the depth
            f = ctx.dispatch(W, H, mode)
            ctx.accum_begin(W, H, FIRST, mode=mode, jitter=False)
            ctx.accum_add(3)
            _same(ctx.accum_resolve()[0], f[0], f"{world} mode {mode} accumulation at D = 3")
    finally:
        ctx.set_path_depth(1)


@pytest.mark.parametrize("world,source", [("dragon", "corner"), ("dragon", "jitter"), ("room", "corner")])
def test_changing_the_depth_restarts_the_sums(ctx, refs, world, source):
    _load(ctx, refs, world, 2)
    try:
        _begin(ctx, world, source)
        assert ctx.accum_add(2) == 2
        ctx.set_path_depth(2)
        assert ctx.accum_add(1) == 3, "the same depth set again restarted the sums"
        _same(ctx.accum_resolve()[0], refs.mean(world, source, 2, FIRST, 3), f"{world} {source} D = 2")
        ctx.set_path_depth(3)
        assert ctx.accum_add(2) == 2, "a new depth did not restart the sums"
        got = ctx.accum_resolve()
        _same(got[0], refs.mean(world, source, 3, FIRST, 2), f"{world} {source} after the restart at D = 3")
        _begin(ctx, world, source)
        assert ctx.accum_add(2) == 2
        fresh = ctx.accum_resolve()
        _same(got[0], fresh[0], f"{world} {source} restart against a fresh accumulation rgba8")
        _same(got[1], fresh[1], f"{world} {source} restart against a fresh accumulation id_dist")
    finally:
        ctx.set_path_depth(1)


def test_the_primary_modes_accumulations_do_not_restart(ctx, refs):
    """the primary modes ignore the depth: a change leaves their sums alone"""
    _load(ctx, refs, "dragon", 1)
    try:
        for mode in (0, 1):
            ctx.accum_begin(W, H, FIRST, mode=mode, jitter=True)
            assert ctx.accum_add(2) == 2
            ctx.set_path_depth(5)
            assert ctx.accum_add(1) == 3, f"mode {mode}: a new depth restarted the sums"
            got = ctx.accum_resolve()[0]
            ctx.set_path_depth(1)
            ctx.accum_begin(W, H, FIRST, mode=mode, jitter=True)
            assert ctx.accum_add(3) == 3
            _same(got, ctx.accum_resolve()[0], f"mode {mode} across a change of the depth")
    finally:
        ctx.set_path_depth(1)


def test_depths_outside_1_to_8_are_refused_and_the_previous_one_holds(ctx, V, refs, batches):
    _load(ctx, refs, "dragon", 3)
    o, d, _ = batches["dragon"]
    try:
        for bad in (0, 9, -1, 1 << 20):
            r = ctx._L.vrt_set_path_depth(ctx._h, bad)
            assert r == -1, f"depth {bad}: {r}, not VRT_E_INVALID"
            with pytest.raises(V.VrtError):
                ctx.set_path_depth(bad)
            assert ctx.path_depth == 3
        assert ctx._L.vrt_set_path_depth(None, 2) == -1
        rgba, _ = ctx.shade_rays(o, d, 2, width=W, first_sample=FIRST)
        _same(rgba, _batch_sample(refs, batches, "dragon", 3, FIRST)[0], "the depth after the refused calls")
        for ok in (1, 8):
            ctx.set_path_depth(ok)
            assert ctx.path_depth == ok
    finally:
        ctx.set_path_depth(1)


def test_a_deep_ray_batch_takes_exactly_one_profiling_slot(ctx, refs, batches):
    o, d, _ = batches["dragon"]
    _load(ctx, refs, "dragon", 1)
    try:
        for D in (1, 3):
            ctx.set_path_depth(D)
            for ns in (1, 3):
                ctx.set_profiling(8)
                ctx.shade_rays(o, d, 2, width=W, first_sample=FIRST, n_samples=ns)
                ms = ctx.profile_read()
                assert len(ms) == 1 and ms[0] > 0.0, f"D={D} n_samples={ns}: {len(ms)} slots"
                ctx.set_profiling(0)
    finally:
        ctx.set_profiling(0)
        ctx.set_path_depth(1)
