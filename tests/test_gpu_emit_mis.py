"""Emitter MIS (include/vrt.h vrt_set_emitter_mis) on the MI355X: the kernels' own emit_mis_density() against the numpy restatement;
the samples of VRT_MODE_FULL in accumulations and ray batches with sampling on, VRT_EMIT_POWER and the flag set, at D in {1, 3} and
sun radius in {0, 0.05}, byte for byte (HDR: bit for bit) against the checker (tests/oracle_paths.c through oracle_emit_mis) in emit_mis_worlds.py's room
at 72 x 44: a merged lamp on the floor, singles against walls and ceiling, a black emitter, glass in front of the camera. Where the
flag is not read -- sampling off, VRT_EMIT_UNIFORM, a world without emitters -- flag 1 gives flag 0's bytes and does not restart.
Every reference sample is computed once per (mode, ray source, D, radius, sample) and shared."""
import ctypes as C

import numpy as np
import pytest

import emit_mis_worlds as mw
import emit_worlds as ew
import oracle_adaptive
import oracle_emit as oe
import oracle_emit_mis as om
import oracle_emit_power as op
import oracle_hdr
import oracle_lens
import oracle_rays
import oracle_sun as osun
import test_gpu_emitters as tge

pytestmark = pytest.mark.gpu
F = np.float32
W, H = mw.W, mw.H
DEPTHS = (1, 3)
RADII = (0.0, 0.05)
SOURCES = tge.SOURCES
RULE = tge.RULE
OFF, POWER, UNIFORM, MIS = False, True, "uniform", "mis"   # a reference sample's `on`
_same, _bits, _begin = tge._same, tge._bits, tge._begin
dragon = tge.dragon


class Refs(tge.Refs):
    """test_gpu_emitters.Refs whose samples are the MIS checker's: the list with its weights, and `on` naming mode and flag"""

    def __init__(self, libs, O, V, world, highlighted=None, pose=mw.POSE, lens=mw.LENS, W=W, H=H, bounds=()):
        """bounds: the (world_min, world_max) of a world that does not have the default ones"""
        super().__init__(libs[:5], O, V, world, pose=pose, lens=lens, W=W, H=H)
        self.M = libs[5]
        self.list, self.words = op.walk(world.records()[0], *bounds)
        self.weights = np.array(op.weights(self.list, self.words), np.uint64)
        self.highlighted = highlighted
        if highlighted is not None:
            self.scene.highlighted[:] = list(highlighted)

    def shade(self, o, d, D, radius, k, on, width):
        mode = op.UNIFORM if on == UNIFORM else op.POWER
        return om.shade(self.M, self.scene, o, d, D, radius, self.list if on else None, self.weights if on else None, mode, 1 if on == MIS else 0,
                        width=width, sample=k)

    def sample(self, source, D, radius, k, on=MIS):
        k &= 0xFFFFFFFF
        key = (source, D, radius, k, on)
        if key not in self._samples:
            o, d = self.rays(source, k)
            self._samples[key] = self.shade(o, d, D, radius, k, on, self.W)
        return self._samples[key]

    def mean(self, source, D, radius, first, n, on=MIS):
        return super().mean(source, D, radius, first, n, on)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("oracle_emit_mis")
    return oe.build(tmp), osun.build(tmp), oracle_rays.build(tmp), oracle_lens.build(tmp), oracle_hdr.build(tmp), om.build(tmp)


@pytest.fixture(scope="module")
def refs(libs, O, V):
    w = mw.room(V)
    r = Refs(libs, O, V, w)
    w.close()
    assert r.list.tolist() == mw.expected_list()
    return r


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _load(c, r, depth=1, radius=0.0, on=True, variant=0, mode=1, mis=1):
    tge._load(c, r, depth, radius, on, variant)
    if getattr(r, "highlighted", None) is not None:
        p = c.default_params()
        p.highlighted[:] = list(r.highlighted)
        c.set_params(p)
    c.set_emitter_importance(mode)
    c.set_emitter_mis(mis)


def _reset(c):
    tge._reset(c)
    c.set_emitter_importance(0)
    c.set_emitter_mis(0)


# ---- the density probe ----

def _probe(V, x, dirs, cs, inv, point, axis, cell, w0, w1):
    T = V.test_lib()
    T.vrt_test_emit_mis_density.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    T.vrt_test_emit_mis_density.restype = C.c_int
    n = len(cs)
    fin = np.zeros((n, 11), F)
    fin[:, 0:3], fin[:, 3:6], fin[:, 6], fin[:, 7], fin[:, 8:11] = x, dirs, cs, inv, point
    iin = np.zeros((n, 6), np.int32)
    iin[:, 0], iin[:, 1:4] = axis, cell
    iin[:, 4], iin[:, 5] = np.asarray(w0, np.uint32).view(np.int32), np.asarray(w1, np.uint32).view(np.int32)
    out = np.zeros((n, 2), F)
    assert T.vrt_test_emit_mis_density(0, fin.ctypes.data, iin.ctypes.data, out.ctypes.data, n) == 0
    return out


def test_density_probe_is_the_numpy_restatement(V):
    """the kernels' emit_mis_density() on 4096 cases around cells near coordinate 50 and in the negative octant -- x off each face, on
    a cell plane exactly, inside the cell's slab on every axis (m == 0) -- with cl == 0, w == 0 (a black voxel, and illumination 0),
    inv_power == 0 and negative cs among them: pl and pb bit for bit"""
    rng = np.random.default_rng(7)
    n = 4096
    cell = rng.integers(-60, 60, size=(n, 3)).astype(np.int32)
    cell[: n // 2] = rng.integers(44, 56, size=(n // 2, 3))
    x = (cell + rng.uniform(-3.0, 4.0, size=(n, 3))).astype(F)
    axis = rng.integers(0, 3, size=n).astype(np.int32)
    dirs = rng.normal(size=(n, 3)).astype(F)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True).astype(F)
    point = (cell + rng.uniform(0.0, 1.0, size=(n, 3))).astype(F)
    cs = rng.uniform(-0.3, 1.0, size=n).astype(F)
    w0 = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    w1 = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    inv = (1.0 / rng.integers(1, 1 << 40, size=n).astype(np.float64)).astype(F)
    i = np.arange(n)
    inside = i % 16 == 0          # m == 0
    x[inside] = (cell[inside] + rng.uniform(0.0, 1.0, size=(int(inside.sum()), 3))).astype(F)
    plane = i % 16 == 1           # x exactly on a cell plane: not visible on that axis
    x[plane, 0] = cell[plane, 0].astype(F)
    x[i % 16 == 2, 1] = (cell[i % 16 == 2, 1] + 1).astype(F)
    flat = i % 16 == 3            # cl == 0, both signs of zero
    dirs[flat, axis[flat]] = np.where(i[flat] % 32 == 3, F(0.0), F(-0.0))
    w0[i % 16 == 4] &= np.uint32(0xff000000)   # a black voxel
    w1[i % 16 == 5] &= np.uint32(0xffff00ff)   # illumination 0
    inv[i % 16 == 6] = F(0.0)
    cs[i % 16 == 7] = -np.abs(cs[i % 16 == 7]) - F(1e-3)
    cs[i % 16 == 8] = np.where(i[i % 16 == 8] % 32 == 8, F(0.0), F(-0.0))
    w = ((w1 >> 8) & 0xff).astype(np.int64) * ((w0 & 0xff).astype(np.int64) + ((w0 >> 8) & 0xff) + ((w0 >> 16) & 0xff))
    pl, pb, m = om.density(x, dirs, cs, point, axis, cell, w, inv)
    got = _probe(V, x, dirs, cs, inv, point, axis, cell, w0, w1)
    assert np.all(m[inside] == 0) and np.all(pl[inside] == 0) and np.all(pl[flat] == 0) and np.all(pb[i % 16 == 7] == 0)
    assert np.all(pl[(i % 16 == 4) | (i % 16 == 5) | (i % 16 == 6)] == 0) and set(np.unique(m).tolist()) == {0, 1, 2, 3}
    assert (pl > 0).sum() > n // 2
    bad = np.flatnonzero((got[:, 0].view(np.uint32) != pl.view(np.uint32)) | (got[:, 1].view(np.uint32) != pb.view(np.uint32)))
    assert len(bad) == 0, f"{len(bad)} of {n} differ; first at {bad[0]}: got {got[bad[0]]} want {(pl[bad[0]], pb[bad[0]])}"


# ---- the accumulation ----

@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_accumulations_are_the_checkers_mean(ctx, refs, source, D, radius):
    """corner, jitter and lens; plain (3 + 5 against 8), adaptive and HDR (test_gpu_emitters._forms)"""
    _load(ctx, refs, D, radius)
    try:
        tge._forms(ctx, refs, source, D, radius, MIS)
    finally:
        _reset(ctx)


@pytest.mark.parametrize("D, radius", ((1, 0.0), (3, 0.05)))
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_accumulations_of_the_record_array_kernels(ctx, refs, source, D, radius):
    """vrt_set_variant(1), the kernels over EmitMisPaths<v1::Trav>: the same forms against the same references"""
    _load(ctx, refs, D, radius, variant=1)
    try:
        tge._forms(ctx, refs, source, D, radius, MIS)
    finally:
        _reset(ctx)


def test_a_first_sample_other_than_0(ctx, refs):
    _load(ctx, refs, 3, 0.05)
    try:
        for source, first in (("corner", 7), ("jitter", (1 << 32) - 2)):
            _begin(ctx, refs, source, first=first)
            assert ctx.accum_add(3) == 3
            _same(ctx.accum_resolve()[0], refs.mean(source, 3, 0.05, first, 3), f"{source} first sample {first}")
        _begin(ctx, refs, "corner", first=7, hdr=True)
        assert ctx.accum_add(3) == 3
        acc = oracle_hdr.Accum(refs.HH, H, W)
        for k in range(3):
            acc.add(refs.sample("corner", 3, 0.05, 7 + k)[2].reshape(H, W, 3))
        _same(_bits(ctx.accum_resolve_hdr("clamp", 1.0)[0]), _bits(acc.mean()), "HDR float mean, first sample 7")
    finally:
        _reset(ctx)


@pytest.mark.parametrize("what", ("no pane", "highlighted emitter"))
def test_other_worlds(ctx, libs, O, V, what):
    """the fixture without its glass pane, and with the highlighted voxel set to a cell of the lamp"""
    w = mw.room(V, pane=what != "no pane")
    (lx, ly, lz), _, _ = mw.LAMP
    r = Refs(libs, O, V, w, highlighted=None if what == "no pane" else (lx, ly + 1, lz + 1))
    w.close()
    _load(ctx, r, 3, 0.05)
    try:
        for source in ("corner", "lens"):
            _begin(ctx, r, source)
            assert ctx.accum_add(3) == 3
            _same(ctx.accum_resolve()[0], r.mean(source, 3, 0.05, 0, 3), f"{what} {source} rgba8")
        _begin(ctx, r, "jitter", hdr=True)
        assert ctx.accum_add(2) == 2
        acc = oracle_hdr.Accum(r.HH, H, W)
        for k in range(2):
            acc.add(r.sample("jitter", 3, 0.05, k)[2].reshape(H, W, 3))
        _same(_bits(ctx.accum_resolve_hdr("clamp", 1.0)[0]), _bits(acc.mean()), f"{what} HDR float mean")
        o, d, _ = mw.all_rays()
        o = np.ascontiguousarray(np.broadcast_to(o, d.shape))
        rgba, _ = ctx.shade_rays(o, d, 2, width=1, first_sample=2)
        _same(rgba, r.shade(o, d, 3, 0.05, 2, MIS, 1)[0], f"{what} near and far rays")
    finally:
        _reset(ctx)
        ctx.set_params(ctx.default_params())


# ---- ray batches ----

@pytest.fixture(scope="module")
def batches(refs):
    """name -> (origins, dirs, cache): the frame's 3168 rays, the far set (emit_worlds.probe_rays()) and the near set"""
    fo, fd = refs.rays("corner", 0)
    o, dn = mw.near_rays()
    _, df = mw.far_rays()
    full = lambda d: np.ascontiguousarray(np.broadcast_to(o, d.shape))
    return {"frame": (fo, fd, {}), "far": (full(df), df, {}), "near": (full(dn), dn, {})}


def _width(name):
    return W if name == "frame" else 1


def _batch_sample(refs, batches, name, D, radius, k, on=MIS):
    o, d, cache = batches[name]
    key = (D, radius, k, on)
    if key not in cache:
        cache[key] = refs.shade(o, d, D, radius, k, on, _width(name))
    return cache[key]


def _batch_mean(refs, batches, name, D, radius, first, n, on=MIS):
    total = sum(_batch_sample(refs, batches, name, D, radius, first + k, on)[0].astype(np.uint64) for k in range(n))
    out = ((total + n // 2) // n).astype(np.uint8)
    out[:, 3] = 255
    return out


@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("D", DEPTHS)
def test_ray_batches_host_and_device_forms(ctx, refs, batches, D, radius, variant):
    import torch
    _load(ctx, refs, D, radius, variant=variant)
    try:
        for name in ("frame", "far", "near"):
            o, d, _ = batches[name]
            n, w = o.shape[0], _width(name)
            t_o = torch.from_numpy(o).cuda()
            t_d = torch.from_numpy(d).cuda()
            t_rgba = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
            t_id = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            for ns in (1, 4):
                what = f"{name} D={D} radius {radius} variant {variant} n_samples={ns}"
                want = _batch_mean(refs, batches, name, D, radius, 0, ns)
                want_id = _batch_sample(refs, batches, name, D, radius, 0)[1]
                rgba, idd = ctx.shade_rays(o, d, 2, width=w, first_sample=0, n_samples=ns)
                _same(rgba, want, f"{what} host rgba8")
                _same(idd, want_id, f"{what} host id_dist")
                ctx.shade_rays_device(n, t_o.data_ptr(), 3, t_d.data_ptr(), t_rgba.data_ptr(), t_id.data_ptr(), 2, width=w, first_sample=0,
                                      n_samples=ns)
                ctx.synchronize()
                _same(t_rgba.cpu().numpy(), want, f"{what} device rgba8")
                _same(t_id.cpu().numpy(), want_id, f"{what} device id_dist")
    finally:
        _reset(ctx)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("D", DEPTHS)
def test_ray_batches_hdr_with_caller_sums(ctx, refs, batches, D, radius):
    """3 + 5 samples through the caller's sums equal 8 in one call, bit for bit, and both equal the checker's floats summed in float64
    in sample order (tests/oracle_hdr.c's arithmetic); the host form at 1 and 4 samples"""
    import torch
    _load(ctx, refs, D, radius)
    try:
        for name in ("frame", "far", "near"):
            o, d, _ = batches[name]
            n, w = o.shape[0], _width(name)
            sums = np.zeros((n, 3), np.float64)
            for k in range(8):
                rgb = np.ascontiguousarray(_batch_sample(refs, batches, name, D, radius, k)[2])
                refs.HH.o_hdr_add(sums.ctypes.data, rgb.ctypes.data, None, rgb.size)
            want = np.zeros((n, 3), F)
            counts = np.full(n, 8, np.uint32)
            refs.HH.o_hdr_mean(sums.ctypes.data, counts.ctypes.data, n, want.ctypes.data)
            t_o = torch.from_numpy(o).cuda()
            t_d = torch.from_numpy(d).cuda()
            for parts in ((3, 5), (8,)):
                t_sums = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
                t_rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
                t_rgba = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                prior = 0
                for ns in parts:
                    ctx.shade_rays_hdr_device(n, t_o.data_ptr(), 3, t_d.data_ptr(), t_rgb.data_ptr(), t_rgba.data_ptr(), None, t_sums.data_ptr(),
                                              n_prior=prior, mode=2, width=w, first_sample=prior, n_samples=ns, tonemap="reinhard", exposure=1.7)
                    prior += ns
                ctx.synchronize()
                what = f"{name} D={D} radius {radius} {parts}"
                _same(t_sums.cpu().numpy().view(np.uint64), sums.view(np.uint64), f"{what} float64 sums")
                _same(_bits(t_rgb.cpu().numpy()), _bits(want), f"{what} float mean")
                _same(t_rgba.cpu().numpy(), oracle_hdr.tonemap(refs.HH, want[None], "reinhard", 1.7)[0], f"{what} reinhard bytes")
            for ns in (1, 4):
                acc = np.zeros((n, 3), np.float64)
                for k in range(ns):
                    rgb = np.ascontiguousarray(_batch_sample(refs, batches, name, D, radius, k)[2])
                    refs.HH.o_hdr_add(acc.ctypes.data, rgb.ctypes.data, None, rgb.size)
                m = np.zeros((n, 3), F)
                counts = np.full(n, ns, np.uint32)
                refs.HH.o_hdr_mean(acc.ctypes.data, counts.ctypes.data, n, m.ctypes.data)
                rgb, rgba, idd = ctx.shade_rays_hdr(o, d, 2, width=w, first_sample=0, n_samples=ns)
                _same(_bits(rgb), _bits(m), f"{name} D={D} radius {radius} host form n_samples={ns} float mean")
                _same(idd, _batch_sample(refs, batches, name, D, radius, 0)[1], f"{name} D={D} radius {radius} host form id_dist")
    finally:
        _reset(ctx)


def test_the_flag_changes_the_bytes_where_it_is_read(ctx, refs, batches):
    """the near rays' floats at flag 1 differ from flag 0's, and flag 0 is the power checker's"""
    _load(ctx, refs, 1, 0.0, mis=0)
    try:
        o, d, _ = batches["near"]
        a = ctx.shade_rays_hdr(o, d, 2, width=1, first_sample=0, n_samples=4)[0]
        ctx.set_emitter_mis(1)
        b = ctx.shade_rays_hdr(o, d, 2, width=1, first_sample=0, n_samples=4)[0]
        assert not np.array_equal(_bits(a), _bits(b))
        want = sum(_batch_sample(refs, batches, "near", 1, 0.0, k, POWER)[2].astype(np.float64) for k in range(4))
        assert np.allclose(a, want / 4, rtol=1e-5, atol=1e-6)
        rgba, _ = ctx.shade_rays(o, d, 2, width=1, first_sample=1)
        ctx.set_emitter_mis(0)
        _same(ctx.shade_rays(o, d, 2, width=1, first_sample=1)[0], _batch_sample(refs, batches, "near", 1, 0.0, 1, POWER)[0], "flag 0 is power")
        _same(rgba, _batch_sample(refs, batches, "near", 1, 0.0, 1, MIS)[0], "flag 1 is MIS")
    finally:
        _reset(ctx)


# ---- where the flag is not read ----

def _routes(ctx, r, rays):
    """every route's output at (D, radius) in ((1, 0), (3, 0.05)): the three ray sources, adaptive, HDR, ray batches plain and HDR"""
    out = []
    for D, radius in ((1, 0.0), (3, 0.05)):
        ctx.set_path_depth(D)
        ctx.set_sun_disc(radius)
        for source in sorted(SOURCES):
            _begin(ctx, r, source)
            ctx.accum_add(2)
            out += list(ctx.accum_resolve())
        _begin(ctx, r, "jitter", adaptive=RULE)
        ctx.accum_add(4)
        out += list(ctx.accum_resolve())
        _begin(ctx, r, "corner", hdr=True)
        ctx.accum_add(2)
        out += [_bits(ctx.accum_resolve_hdr("clamp", 1.0)[0])]
        out += list(ctx.shade_rays(*rays, 2, width=W, first_sample=1, n_samples=2))
        out += [_bits(ctx.shade_rays_hdr(*rays, 2, width=W, first_sample=1, n_samples=2)[0])]
    return out


def _no_restart(ctx, r, what):
    """toggling the flag in the middle of a full-mode accumulation: the sample count goes on"""
    ctx.set_path_depth(1)
    ctx.set_sun_disc(0.0)
    ctx.set_emitter_mis(0)
    _begin(ctx, r, "corner")
    assert ctx.accum_add(2) == 2
    ctx.set_emitter_mis(1)
    assert ctx.accum_add(1) == 3, f"{what}: setting the flag restarted the sums"
    ctx.set_emitter_mis(0)
    assert ctx.accum_add(1) == 4, f"{what}: clearing the flag restarted the sums"


@pytest.mark.parametrize("case", ("sampling off", "uniform"))
def test_flag_1_is_flag_0_where_it_is_not_read(ctx, refs, case):
    on, mode = (False, 1) if case == "sampling off" else (True, 0)
    _load(ctx, refs, on=on, mode=mode, mis=0)
    try:
        rays = refs.rays("corner", 0)
        before = _routes(ctx, refs, rays)
        ctx.set_emitter_mis(1)
        assert ctx.emitter_mis == 1
        for i, (x, y) in enumerate(zip(_routes(ctx, refs, rays), before)):
            _same(x, y, f"{case}: output {i} at flag 1 against flag 0")
        _no_restart(ctx, refs, case)
    finally:
        _reset(ctx)


def test_flag_1_is_flag_0_without_emitters(ctx, dragon):
    """the dragon has no emitter: sampling on, VRT_EMIT_POWER, and the flag changes nothing"""
    _load(ctx, dragon, on=True, mode=1, mis=0)
    try:
        assert len(ctx.emitters()) == 0
        before = _routes(ctx, dragon, dragon.rays)
        ctx.set_emitter_mis(1)
        for i, (x, y) in enumerate(zip(_routes(ctx, dragon, dragon.rays), before)):
            _same(x, y, f"dragon output {i} at flag 1 against flag 0")
        _no_restart(ctx, dragon, "no emitters")
    finally:
        _reset(ctx)


# ---- the restart rule ----

def test_changing_the_flag_restarts_a_full_accumulation_where_it_is_read(ctx, refs):
    _load(ctx, refs, 1, 0.0, mis=1)
    try:
        _begin(ctx, refs, "corner")
        assert ctx.accum_add(2) == 2
        ctx.set_emitter_mis(1)
        assert ctx.accum_add(1) == 3, "the same value set again restarted the sums"
        _same(ctx.accum_resolve()[0], refs.mean("corner", 1, 0.0, 0, 3), "MIS, 2 + 1")
        ctx.set_emitter_mis(0)
        assert ctx.accum_add(2) == 2, "clearing the flag did not restart the sums"
        _same(ctx.accum_resolve()[0], refs.mean("corner", 1, 0.0, 0, 2, POWER), "after the restart at flag 0")
        ctx.set_emitter_mis(1)
        assert ctx.accum_add(1) == 1, "setting the flag did not restart the sums"
        _same(ctx.accum_resolve()[0], refs.mean("corner", 1, 0.0, 0, 1), "after the restart at flag 1")
        for mode in (0, 1):   # the primary modes never restart
            ctx.accum_begin(W, H, 0, mode=mode, jitter=True)
            assert ctx.accum_add(2) == 2
            ctx.set_emitter_mis(0)
            assert ctx.accum_add(1) == 3, f"mode {mode}: the flag restarted the sums"
            ctx.set_emitter_mis(1)
            assert ctx.accum_add(1) == 4, f"mode {mode}: the flag restarted the sums"
    finally:
        _reset(ctx)


def test_frames_ignore_the_flag(ctx, refs):
    _load(ctx, refs, 1, 0.0, mis=0)
    try:
        def outputs():
            out = []
            for mode in (0, 1, 2):
                out += list(ctx.dispatch(W, H, mode))
            out += list(ctx.dispatch_frame(W, H, 2))
            return out
        before = outputs()
        ctx.set_emitter_mis(1)
        for i, (x, y) in enumerate(zip(outputs(), before)):
            _same(x, y, f"frame output {i} at flag 1 against flag 0")
    finally:
        _reset(ctx)


# ---- a patch changes Wtot ----

def test_a_patch_that_adds_an_emitter_changes_the_weights(ctx, libs, O, V):
    w = mw.room(V)
    try:
        r = Refs(libs, O, V, w)
        _load(ctx, r, 3, 0.0)
        _begin(ctx, r, "corner")
        assert ctx.accum_add(2) == 2
        _same(ctx.accum_resolve()[0], r.mean("corner", 3, 0.0, 0, 2), "before the patch")
        (ax, ay, az), ac, ai = mw.SPARE
        w.insert(ax, ay, az, ac, 3.0, ai / 255.0, 0.0)
        assert ctx.patch_voxel(w, ax, ay, az) is not None
        r1 = Refs(libs, O, V, w)
        assert len(r1.list) == mw.N_EMITTERS + 1 and int(r1.weights.sum()) > int(r.weights.sum())
        assert np.array_equal(ctx.emitters(), r1.list)
        assert ctx.accum_add(2) == 2, "the patch did not restart the sums"
        _same(ctx.accum_resolve()[0], r1.mean("corner", 3, 0.0, 0, 2), "the next add after the patch")
        o, d, _ = mw.all_rays()
        o = np.ascontiguousarray(np.broadcast_to(o, d.shape))
        _same(ctx.shade_rays(o, d, 2, width=1, first_sample=1)[0], r1.shade(o, d, 3, 0.0, 1, MIS, 1)[0], "a ray batch after the patch")
    finally:
        w.close()
        _reset(ctx)


# ---- errors ----

def test_errors(V):
    c = V.Context(0)
    try:
        for bad in (-1, 2):
            assert c._L.vrt_set_emitter_mis(c._h, bad) == -1
        assert c._L.vrt_set_emitter_mis(None, 1) == -1
        assert c._L.vrt_set_emitter_mis(c._h, 1) == 0 and c._L.vrt_set_emitter_mis(c._h, 0) == 0
        for bad in (2, -1):
            assert c._L.vrt_set_emitter_importance(c._h, bad) == -1, "vrt_set_emitter_importance keeps its 0 / 1 contract"
    finally:
        c.close()


def test_an_invalid_value_leaves_the_previous_one(ctx, refs):
    _load(ctx, refs, 1, 0.0, mis=1)
    try:
        for bad in (-1, 2, 7):
            assert ctx._L.vrt_set_emitter_mis(ctx._h, bad) == -1
        _begin(ctx, refs, "corner")
        assert ctx.accum_add(1) == 1
        _same(ctx.accum_resolve()[0], refs.mean("corner", 1, 0.0, 0, 1), "the flag still holds")
    finally:
        _reset(ctx)
