"""Sun disc (include/vrt.h vrt_set_sun_disc) on the MI355X: the samples of VRT_MODE_FULL in accumulations and ray batches with a
sun of tan_radius 0.05 (and 1.0 once per world) at D in {1, 3}, byte for byte (HDR: bit for bit) against the checker
(tests/oracle_paths.c through oracle_sun), on test_gpu_path_depth.py's worlds at 72 x 44: the dragon (opaque: the two-pass and one-kernel routes), the
room seen from inside (glass: the general kernel) and the unit-internal stream (the record-array kernels). Every reference sample
is computed once per (world, ray source, D, radius, sample) and shared. Radius 0 is the parent: oracle_path_depth's bytes."""
import numpy as np
import pytest

import oracle_adaptive
import oracle_hdr
import oracle_lens
import oracle_path_depth as opd
import oracle_rays
import oracle_sun as osun
import sun_worlds as sw
from test_gpu_shade_rays import _ray_mix

pytestmark = pytest.mark.gpu
F = np.float32
W, H = sw.W, sw.H
WORLDS, LENS = sw.WORLDS, sw.LENS
DEPTHS = (1, 3)
R_SOFT, R_WIDE = 0.05, 1.0
FIRST = 5
SOURCES = {"corner": (False, False), "jitter": (True, False), "lens": (False, True), "lens+jitter": (True, True)}   # jitter, lens


class Refs:
    """The checker's side: scenes, each sample's rays and each sample's result, computed once"""

    def __init__(self, tmp, O, V, product_scenes):
        self.S = osun.build(tmp)
        self.P = opd.build(tmp)
        self.R = oracle_rays.build(tmp)
        self.LL = oracle_lens.build(tmp)
        self.HH = oracle_hdr.build(tmp)
        self.world = sw.scenes(O, V, product_scenes)
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

    def sample(self, world, source, D, radius, k):
        """-> (rgba8[H*W,4], id_dist[H*W,2], rgb float32[H*W,3]) of sample k"""
        key = (world, source, D, radius, k)
        if key not in self._samples:
            o, d = self.rays(world, source, k)
            self._samples[key] = osun.shade(self.S, self.world[world][3], o, d, D, radius, width=W, sample=k)
        return self._samples[key]

    def mean(self, world, source, D, radius, first, n):
        total = sum(self.sample(world, source, D, radius, first + k)[0].astype(np.uint64) for k in range(n))
        out = ((total + n // 2) // n).astype(np.uint8)
        out[:, 3] = 255
        return out.reshape(H, W, 4)

    def frame_id(self, world):
        """the resolved (voxel ID, dist): the unjittered pinhole frame's, at any depth and radius"""
        return self.sample(world, "corner", 1, R_SOFT, 0)[1].reshape(H, W, 2)


@pytest.fixture(scope="module")
def refs(tmp_path_factory, O, V, product_scenes):
    return Refs(tmp_path_factory.mktemp("oracle_sun"), O, V, product_scenes)


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _load(c, refs, world, depth=1, radius=0.0):
    tex, dim, cam, _ = refs.world[world]
    c.upload_octree(tex, dim)
    c.set_camera(*cam)
    p = c.default_params()
    if world == "unit":
        p.world_min[:] = sw.UNIT_BOUNDS[0]
        p.world_max[:] = sw.UNIT_BOUNDS[1]
    c.set_params(p)
    c.set_variant(0)
    c.set_lens(0.0, 1.0)
    c.set_path_depth(depth)
    c.set_sun_disc(radius)


def _reset(c):
    c.set_lens(0.0, 1.0)
    c.set_path_depth(1)
    c.set_sun_disc(0.0)


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


def _three_forms(c, refs, world, source, D, radius):
    """plain, adaptive and HDR accumulations of one (world, source, D, radius): first = 5, three samples added as 1 + 2"""
    what = f"{world} {source} D={D} radius {radius}"
    _begin(c, world, source)
    assert c.accum_add(1) == 1 and c.accum_add(2) == 3
    got = c.accum_resolve()
    _same(got[0], refs.mean(world, source, D, radius, FIRST, 3), f"{what} rgba8")
    _same(got[1], refs.frame_id(world), f"{what} id_dist")
    rule = (2, 4, 0)
    _begin(c, world, source, adaptive=rule)
    assert c.accum_add(1) == 1 and c.accum_add(3) == 4
    got = c.accum_resolve()
    counts, active = c.accum_counts()
    st = oracle_adaptive.accumulate(lambda k: refs.sample(world, source, D, radius, k)[0].reshape(H, W, 4), H, W, FIRST, 4, rule, np.int64)
    assert np.array_equal(counts, st.counts()), f"{what}: adaptive counts"
    assert active == int(st.active(rule).sum())
    _same(got[0], st.resolve(), f"{what} adaptive rgba8")
    _same(got[1], refs.frame_id(world), f"{what} adaptive id_dist")
    _begin(c, world, source, hdr=True)
    assert c.accum_add(1) == 1 and c.accum_add(2) == 3
    acc = oracle_hdr.Accum(refs.HH, H, W)
    for k in range(3):
        acc.add(refs.sample(world, source, D, radius, FIRST + k)[2].reshape(H, W, 3))
    want = acc.mean()
    for op, e in (("clamp", 1.0), ("reinhard", 1.7)):
        rgb, rgba, _ = c.accum_resolve_hdr(op, e)
        _same(_bits(rgb), _bits(want), f"{what} float mean ({op})")
        _same(rgba, oracle_hdr.tonemap(refs.HH, want, op, e), f"{what} {op} bytes")
    _same(c.accum_resolve()[0], refs.mean(world, source, D, radius, FIRST, 3), f"{what} the bytes beside the floats")


# ---- the accumulation ----

@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("world", WORLDS)
def test_accumulations_are_the_checkers_mean(ctx, refs, world, source, D):
    _load(ctx, refs, world, D, R_SOFT)
    try:
        _three_forms(ctx, refs, world, source, D, R_SOFT)
    finally:
        _reset(ctx)


@pytest.mark.parametrize("world", WORLDS)
def test_a_sun_as_wide_as_the_rule_allows(ctx, refs, world):
    """tan_radius 1: directions below a surface's horizon, shadow rays along every axis sign"""
    _load(ctx, refs, world, 3, R_WIDE)
    try:
        _three_forms(ctx, refs, world, "jitter" if world == "dragon" else "corner", 3, R_WIDE)
        if world == "dragon":
            _begin(ctx, world, "corner")
            ctx.accum_add(3)
            _same(ctx.accum_resolve()[0], refs.mean(world, "corner", 3, R_WIDE, FIRST, 3), "dragon corner radius 1 rgba8")
    finally:
        _reset(ctx)


@pytest.mark.parametrize("D", DEPTHS)
def test_every_opaque_route_gives_the_same_bytes_on_the_dragon(ctx, V, refs, D):
    _load(ctx, refs, "dragon", D, R_SOFT)
    try:
        for source in ("corner", "lens+jitter"):
            want = refs.mean("dragon", source, D, R_SOFT, FIRST, 2)
            for form in (0, 1, 5, 6, 7):
                ctx.set_option(V.OPT_FULL_OPAQUE, form)
                _begin(ctx, "dragon", source)
                ctx.accum_add(2)
                got = ctx.accum_resolve()
                _same(got[0], want, f"{source} D={D} VRT_OPT_FULL_OPAQUE {form} rgba8")
                _same(got[1], refs.frame_id("dragon"), f"{source} D={D} VRT_OPT_FULL_OPAQUE {form} id_dist")
    finally:
        ctx.set_option(V.OPT_FULL_OPAQUE, 6)
        _reset(ctx)


# ---- ray batches ----

@pytest.fixture(scope="module")
def batches(refs):
    """world -> (origins, dirs, cache): the frame's rays, then test_gpu_shade_rays.py's mix of arbitrary ones -- origins in
    glass, in solids, on faces, outside the world, un-normalised and axis-parallel directions"""
    boxes = {"dragon": ((0, 0, 0), (126, 95, 60), ((40, 2, 20), (80, 6, 40)), ((50, 1, 25), (70, 4, 35))),
             "room": ((0, 0, 0), (120, 64, 120), ((10, 20, 10), (20, 40, 20)), ((0, 0, 0), (120, 1, 120))),
             "unit": ((0, 0, 0), (8, 8, 8), ((4, 4, 4), (5, 5, 5)), ((4, 4, 4), (5, 5, 5)))}
    out = {}
    for i, world in enumerate(WORLDS):
        fo, fd = refs.rays(world, "corner", 0)
        ao, ad = _ray_mix(np.random.default_rng(41 + i), 400, *boxes[world])
        out[world] = (np.concatenate([fo, ao]), np.concatenate([fd, ad]), {})
    return out


def _batch_sample(refs, batches, world, D, radius, k, width=W):
    o, d, cache = batches[world]
    key = (D, radius, k, width)
    if key not in cache:
        cache[key] = osun.shade(refs.S, refs.world[world][3], o, d, D, radius, width=width, sample=k)
    return cache[key]


def _batch_mean(refs, batches, world, D, radius, first, n, width=W):
    total = sum(_batch_sample(refs, batches, world, D, radius, first + k, width)[0].astype(np.uint64) for k in range(n))
    out = ((total + n // 2) // n).astype(np.uint8)
    out[:, 3] = 255
    return out


@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("world", WORLDS)
def test_ray_batches_host_and_device_forms(ctx, refs, batches, world, D):
    import torch
    _load(ctx, refs, world, D, R_SOFT)
    o, d, _ = batches[world]
    n = o.shape[0]
    try:
        t_o = torch.from_numpy(o).cuda()
        t_d = torch.from_numpy(d).cuda()
        t_rgba = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
        t_id = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for ns in (1, 4):
            want = _batch_mean(refs, batches, world, D, R_SOFT, FIRST, ns)
            want_id = _batch_sample(refs, batches, world, D, R_SOFT, FIRST)[1]
            rgba, idd = ctx.shade_rays(o, d, 2, width=W, first_sample=FIRST, n_samples=ns)
            _same(rgba, want, f"{world} D={D} n_samples={ns} host rgba8")
            _same(idd, want_id, f"{world} D={D} n_samples={ns} host id_dist")
            ctx.shade_rays_device(n, t_o.data_ptr(), 3, t_d.data_ptr(), t_rgba.data_ptr(), t_id.data_ptr(), 2, width=W, first_sample=FIRST,
                                  n_samples=ns)
            ctx.synchronize()
            _same(t_rgba.cpu().numpy(), want, f"{world} D={D} n_samples={ns} device rgba8")
            _same(t_id.cpu().numpy(), want_id, f"{world} D={D} n_samples={ns} device id_dist")
    finally:
        _reset(ctx)


@pytest.mark.parametrize("width", (1, 7))
@pytest.mark.parametrize("world", ("dragon", "room"))
def test_ray_batches_at_other_widths(ctx, refs, batches, world, width):
    """a list of rays (width 1: every ray is pixel (0, i)) and rows of seven: the random numbers follow (i % width, i / width)"""
    _load(ctx, refs, world, 3, R_SOFT)
    o, d, _ = batches[world]
    try:
        for ns in (1, 4):
            rgba, idd = ctx.shade_rays(o, d, 2, width=width, first_sample=FIRST, n_samples=ns)
            _same(rgba, _batch_mean(refs, batches, world, 3, R_SOFT, FIRST, ns, width), f"{world} width {width} n_samples={ns} rgba8")
            _same(idd, _batch_sample(refs, batches, world, 3, R_SOFT, FIRST, width)[1], f"{world} width {width} n_samples={ns} id_dist")
    finally:
        _reset(ctx)


@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("world", WORLDS)
def test_ray_batches_hdr_with_caller_sums(ctx, refs, batches, world, D):
    """3 + 5 samples through the caller's sums equal 8 in one call, bit for bit, and both equal the checker's floats summed in
    float64 in sample order (tests/oracle_hdr.c's arithmetic)"""
    import torch
    _load(ctx, refs, world, D, R_SOFT)
    o, d, _ = batches[world]
    n = o.shape[0]
    try:
        sums = np.zeros((n, 3), np.float64)
        for k in range(8):
            rgb = np.ascontiguousarray(_batch_sample(refs, batches, world, D, R_SOFT, FIRST + k)[2])
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
        for ns in (1, 4):
            acc = np.zeros((n, 3), np.float64)
            for k in range(ns):
                rgb = np.ascontiguousarray(_batch_sample(refs, batches, world, D, R_SOFT, FIRST + k)[2])
                refs.HH.o_hdr_add(acc.ctypes.data, rgb.ctypes.data, None, rgb.size)
            m = np.zeros((n, 3), F)
            counts = np.full(n, ns, np.uint32)
            refs.HH.o_hdr_mean(acc.ctypes.data, counts.ctypes.data, n, m.ctypes.data)
            rgb, rgba, idd = ctx.shade_rays_hdr(o, d, 2, width=W, first_sample=FIRST, n_samples=ns)
            _same(_bits(rgb), _bits(m), f"{world} D={D} host form n_samples={ns} float mean")
            _same(idd, _batch_sample(refs, batches, world, D, R_SOFT, FIRST)[1], f"{world} D={D} host form id_dist")
    finally:
        _reset(ctx)


# ---- radius 0 is the parent ----

@pytest.mark.parametrize("world", WORLDS)
def test_radius_0_after_a_soft_run_is_oracle_path_depth(ctx, refs, batches, world):
    _load(ctx, refs, world, 1, R_SOFT)
    o, d, _ = batches[world]
    s = refs.world[world][3]
    try:
        ctx.shade_rays(o, d, 2, width=W, first_sample=FIRST)
        _begin(ctx, world, "corner")
        ctx.accum_add(1)
        ctx.set_sun_disc(0.0)
        assert ctx.sun_disc == 0.0
        fo, fd = refs.rays(world, "corner", 0)
        for D in DEPTHS:
            ctx.set_path_depth(D)
            want, _ = opd.mean(refs.P, s, o, d, D, width=W, first_sample=FIRST, n_samples=2)
            rgba, _ = ctx.shade_rays(o, d, 2, width=W, first_sample=FIRST, n_samples=2)
            _same(rgba, want, f"{world} D={D} shade_rays at radius 0")
            for source in ("corner", "lens+jitter"):
                ro, rd = zip(*(refs.rays(world, source, FIRST + k) for k in range(2)))
                total = sum(opd.shade(refs.P, s, ro[k], rd[k], D, width=W, sample=FIRST + k)[0].astype(np.uint64) for k in range(2))
                want = ((total + 1) // 2).astype(np.uint8)
                want[:, 3] = 255
                _begin(ctx, world, source)
                ctx.accum_add(2)
                _same(ctx.accum_resolve()[0], want.reshape(H, W, 4), f"{world} D={D} {source} accumulation at radius 0")
    finally:
        _reset(ctx)


@pytest.mark.parametrize("world", WORLDS)
def test_frames_and_the_primary_modes_ignore_the_sun_disc(ctx, refs, world):
    _load(ctx, refs, world, 1, 0.0)
    try:
        def outputs():
            out = []
            for mode in (0, 1, 2):
                out += list(ctx.dispatch(W, H, mode))
            out += list(ctx.dispatch_frame(W, H, 2))
            for mode in (0, 1):
                for jitter in (False, True):
                    ctx.accum_begin(W, H, FIRST, mode=mode, jitter=jitter)
                    ctx.accum_add(3)
                    out += list(ctx.accum_resolve())
            return out
        before = outputs()
        ctx.set_sun_disc(R_SOFT)
        for i, (x, y) in enumerate(zip(outputs(), before)):
            _same(x, y, f"{world} output {i} at radius {R_SOFT} against radius 0")
    finally:
        _reset(ctx)


# ---- the setting itself ----

@pytest.mark.parametrize("world,source", [("dragon", "corner"), ("dragon", "jitter"), ("room", "corner")])
def test_changing_the_radius_restarts_the_sums(ctx, refs, world, source):
    _load(ctx, refs, world, 1, R_SOFT)
    try:
        _begin(ctx, world, source)
        assert ctx.accum_add(2) == 2
        ctx.set_sun_disc(R_SOFT)
        assert ctx.accum_add(1) == 3, "the same radius set again restarted the sums"
        _same(ctx.accum_resolve()[0], refs.mean(world, source, 1, R_SOFT, FIRST, 3), f"{world} {source} radius {R_SOFT}")
        ctx.set_sun_disc(R_WIDE)
        assert ctx.accum_add(2) == 2, "a new radius did not restart the sums"
        _same(ctx.accum_resolve()[0], refs.mean(world, source, 1, R_WIDE, FIRST, 2), f"{world} {source} after the restart at radius {R_WIDE}")
    finally:
        _reset(ctx)


def test_the_primary_modes_accumulations_do_not_restart(ctx, refs):
    _load(ctx, refs, "dragon", 1, 0.0)
    try:
        for mode in (0, 1):
            ctx.accum_begin(W, H, FIRST, mode=mode, jitter=True)
            assert ctx.accum_add(2) == 2
            ctx.set_sun_disc(R_SOFT)
            assert ctx.accum_add(1) == 3, f"mode {mode}: a new radius restarted the sums"
            ctx.set_sun_disc(0.0)
    finally:
        _reset(ctx)


def test_radii_outside_0_to_1_are_refused_and_the_previous_one_holds(ctx, V, refs, batches):
    _load(ctx, refs, "dragon", 1, R_SOFT)
    o, d, _ = batches["dragon"]
    try:
        for bad in (-1.0, 1.5, float("nan"), float("inf")):
            r = ctx._L.vrt_set_sun_disc(ctx._h, bad)
            assert r == -1, f"radius {bad}: {r}, not VRT_E_INVALID"
            with pytest.raises(V.VrtError):
                ctx.set_sun_disc(bad)
            assert ctx.sun_disc == float(F(R_SOFT))
        assert ctx._L.vrt_set_sun_disc(None, 0.1) == -1
        rgba, _ = ctx.shade_rays(o, d, 2, width=W, first_sample=FIRST)
        _same(rgba, _batch_sample(refs, batches, "dragon", 1, R_SOFT, FIRST)[0], "the radius after the refused calls")
        for ok in (0.0, 1.0):
            ctx.set_sun_disc(ok)
            assert ctx.sun_disc == ok
    finally:
        _reset(ctx)


def test_profiling_slots_with_a_sun_disc(ctx, refs, batches):
    """one slot per ray-batch call, none for vrt_accum_add"""
    o, d, _ = batches["dragon"]
    _load(ctx, refs, "dragon", 1, R_SOFT)
    try:
        for D in DEPTHS:
            ctx.set_path_depth(D)
            for ns in (1, 3):
                ctx.set_profiling(8)
                ctx.shade_rays(o, d, 2, width=W, first_sample=FIRST, n_samples=ns)
                ms = ctx.profile_read()
                assert len(ms) == 1 and ms[0] > 0.0, f"D={D} n_samples={ns}: {len(ms)} slots"
                ctx.set_profiling(0)
            for source in ("corner", "jitter"):
                ctx.set_profiling(8)
                _begin(ctx, "dragon", source)
                ctx.accum_add(2)
                ctx.synchronize()
                assert len(ctx.profile_read()) == 0, f"D={D} {source}: vrt_accum_add took a slot"
                ctx.set_profiling(0)
    finally:
        ctx.set_profiling(0)
        _reset(ctx)
