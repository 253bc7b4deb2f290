"""Emitter importance (include/vrt.h vrt_set_emitter_importance) on the MI355X: the kernels' own threshold search against the Python
rule on tables of 1 to 2^20 entries; the samples of VRT_MODE_FULL in accumulations and ray batches with sampling on and VRT_EMIT_POWER,
at D in {1, 3} and sun radius in {0, 0.05}, byte for byte (HDR: bit for bit) against the checker (tests/oracle_paths.c through oracle_emit_power) in
emit_power_worlds.py's room at 72 x 44: a merged lamp of size 4 and a panel of 256 dim singles, glass in front of the camera. Mode 1
without sampling or without emitters is mode 0; mode 0 with sampling is oracle_emit; the table after an upload, patches and a
compaction is the Python table of a fresh world. Every reference sample is computed once per (mode, ray source, D, radius, sample) and
shared."""
import ctypes as C

import numpy as np
import pytest

import emit_power_worlds as pw
import emit_worlds as ew
import oracle_adaptive
import oracle_emit as oe
import oracle_emit_power as op
import oracle_hdr
import oracle_lens
import oracle_rays
import oracle_sun as osun
import test_gpu_emitters as tge
from test_gpu_shade_rays import _ray_mix

pytestmark = pytest.mark.gpu
F = np.float32
W, H = pw.W, pw.H
DEPTHS = (1, 3)
RADII = (0.0, 0.05)
SOURCES = tge.SOURCES
RULE = tge.RULE
OFF, POWER, UNIFORM = False, True, "uniform"   # a reference sample's `on`: sampling off, VRT_EMIT_POWER, VRT_EMIT_UNIFORM
_same, _bits, _begin = tge._same, tge._bits, tge._begin
dragon = tge.dragon


class Refs(tge.Refs):
    """test_gpu_emitters.Refs whose samples are the power checker's: the list with its weights, and `on` naming the mode"""

    def __init__(self, libs, O, V, world):
        super().__init__(libs[:5], O, V, world, pose=pw.POSE, lens=pw.LENS)
        self.P = libs[5]
        self.list, words = op.walk(world.records()[0])
        self.weights = np.array(op.weights(self.list, words), np.uint64)
        self.cdf = np.array(op.thresholds(self.weights.tolist()), np.uint32)

    def shade(self, o, d, D, radius, k, on, width):
        mode = op.POWER if on is POWER else op.UNIFORM
        return op.shade(self.P, self.scene, o, d, D, radius, self.list if on else None, self.weights if on else None, mode, width=width, sample=k)

    def sample(self, source, D, radius, k, on=POWER):
        k &= 0xFFFFFFFF
        key = (source, D, radius, k, on)
        if key not in self._samples:
            o, d = self.rays(source, k)
            self._samples[key] = self.shade(o, d, D, radius, k, on, W)
        return self._samples[key]

    def mean(self, source, D, radius, first, n, on=POWER):
        return super().mean(source, D, radius, first, n, on)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("oracle_emit_power")
    return oe.build(tmp), osun.build(tmp), oracle_rays.build(tmp), oracle_lens.build(tmp), oracle_hdr.build(tmp), op.build(tmp)


@pytest.fixture(scope="module")
def refs(libs, O, V):
    w = pw.room(V)
    r = Refs(libs, O, V, w)
    w.close()
    assert len(r.list) == 257 and r.list[:, 3].max() == 4 and 2 * int(r.weights.max()) > int(r.weights.sum())
    return r


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _load(c, r, depth=1, radius=0.0, on=True, variant=0, mode=1):
    tge._load(c, r, depth, radius, on, variant)
    c.set_emitter_importance(mode)


def _reset(c):
    tge._reset(c)
    c.set_emitter_importance(0)


# ---- the selection probe ----

def _pick(V, cdf, u0):
    T = V.test_lib()
    T.vrt_test_emit_pick.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int]
    T.vrt_test_emit_pick.restype = C.c_int
    cdf, u0 = np.ascontiguousarray(cdf, np.uint32), np.ascontiguousarray(u0, F)
    out = np.zeros((len(u0), 2), np.uint32)
    assert T.vrt_test_emit_pick(0, cdf.ctypes.data, len(cdf), u0.ctypes.data, out.ctypes.data, len(u0)) == 0
    return out


@pytest.mark.parametrize("N", (1, 2, 3, 5, 257, 1 << 20))
def test_selection_probe_is_the_python_rule(V, N):
    """the kernels' emit_pick() on tables of N entries -- equal weights, and one weight that holds all but N - 1 ticks -- at u0 = 0,
    1.0f, the largest float below 1, and every threshold's T * 2^-24 with the float below it: j and ticks"""
    for what, wts in (("equal", [1] * N), ("one heavy", [0] * (N // 2) + [1] + [0] * (N - N // 2 - 1))):
        T = np.array(op.thresholds(wts), np.uint32)
        assert T[-1] == 1 << 24 and np.all(np.diff(T.astype(np.int64)) >= 1)
        at = (T.astype(np.float64) * 2.0 ** -24).astype(F)   # exact: T <= 2^24
        u0 = np.concatenate([np.array([0.0, 1.0, np.nextafter(F(1.0), F(0.0))], F), at, np.nextafter(at, F(0.0))])
        t = np.minimum((u0.astype(np.float64) * 16777216.0).astype(np.int64), 16777215)   # a power of two: exact in float32 too
        j = np.searchsorted(T, t, side="right")
        Tl = np.concatenate([[0], T.astype(np.int64)])
        ticks = Tl[j + 1] - Tl[j]
        got = _pick(V, T, u0)
        bad = np.flatnonzero((got[:, 0] != j) | (got[:, 1] != ticks))
        assert len(bad) == 0, f"N={N} {what}: {len(bad)} of {len(u0)} differ; first at u0 = {u0[bad[0]]!r}: got {got[bad[0]]} want {(j[bad[0]], ticks[bad[0]])}"
        assert j.min() == 0 and j.max() == N - 1


# ---- the accumulation ----

@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_accumulations_are_the_checkers_mean(ctx, refs, source, D, radius):
    """corner, jitter and lens; plain (3 + 5 against 8), adaptive and HDR (test_gpu_emitters._forms)"""
    _load(ctx, refs, D, radius)
    try:
        tge._forms(ctx, refs, source, D, radius, POWER)
    finally:
        _reset(ctx)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_accumulations_of_the_record_array_kernels(ctx, refs, source, D, radius):
    """vrt_set_variant(1), the kernels over EmitPowerPaths<v1::Trav>: the same forms over the same matrix, against the same references"""
    _load(ctx, refs, D, radius, variant=1)
    try:
        tge._forms(ctx, refs, source, D, radius, POWER)
    finally:
        _reset(ctx)


def test_the_record_array_kernels(ctx, refs):
    """vrt_set_variant(1): the kernels over EmitPowerPaths<v1::Trav>"""
    _load(ctx, refs, 3, 0.05, variant=1)
    try:
        for source in ("corner", "lens"):
            _begin(ctx, refs, source)
            assert ctx.accum_add(3) == 3
            _same(ctx.accum_resolve()[0], refs.mean(source, 3, 0.05, 0, 3), f"variant 1 {source} rgba8")
        _begin(ctx, refs, "jitter", adaptive=RULE)
        assert ctx.accum_add(6) == 6
        st = oracle_adaptive.accumulate(lambda k: refs.sample("jitter", 3, 0.05, k)[0].reshape(H, W, 4), H, W, 0, 6, RULE, np.int64)
        _same(ctx.accum_resolve()[0], st.resolve(), "variant 1 adaptive jitter rgba8")
        _begin(ctx, refs, "corner", hdr=True)
        assert ctx.accum_add(3) == 3
        acc = oracle_hdr.Accum(refs.HH, H, W)
        for k in range(3):
            acc.add(refs.sample("corner", 3, 0.05, k)[2].reshape(H, W, 3))
        _same(_bits(ctx.accum_resolve_hdr("clamp", 1.0)[0]), _bits(acc.mean()), "variant 1 HDR float mean")
    finally:
        _reset(ctx)


# ---- ray batches ----

@pytest.fixture(scope="module")
def batches(refs):
    """name -> (origins, dirs, cache): the frame's 3168 rays, and a list of 100 arbitrary ones (test_gpu_shade_rays.py's mix)"""
    fo, fd = refs.rays("corner", 0)
    ao, ad = _ray_mix(np.random.default_rng(43), 100, (ew.LO, ew.LO, ew.LO), (ew.HI + 1, ew.HI + 1, ew.HI + 1),
                      ((ew.PANE_X, ew.PANE_Y[0], ew.PANE_Z[0]), (ew.PANE_X + 1, ew.PANE_Y[1], ew.PANE_Z[1])),
                      ((ew.TABLE[0], ew.TABLE_Y, ew.TABLE[0]), (ew.TABLE[1], ew.TABLE_Y + 1, ew.TABLE[1])))
    return {"frame": (fo, fd, {}), "list": (ao, ad, {})}


def _width(name):
    return W if name == "frame" else 1


def _batch_sample(refs, batches, name, D, radius, k, on=POWER):
    o, d, cache = batches[name]
    key = (D, radius, k, on)
    if key not in cache:
        cache[key] = refs.shade(o, d, D, radius, k, on, _width(name))
    return cache[key]


def _batch_mean(refs, batches, name, D, radius, first, n, on=POWER):
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
        for name in ("frame", "list"):
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
    in sample order (tests/oracle_hdr.c's arithmetic)"""
    import torch
    _load(ctx, refs, D, radius)
    try:
        for name in ("frame", "list"):
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


# ---- the mode is read only where sampling is on and the list is not empty ----

def _routes(ctx, V, r, rays, opaque_forms=(6,)):
    """every route's output at (D, radius) in ((1, 0), (3, 0.05)): the three ray sources (per VRT_OPT_FULL_OPAQUE form), adaptive,
    HDR, ray batches plain and HDR"""
    out = []
    for D, radius in ((1, 0.0), (3, 0.05)):
        ctx.set_path_depth(D)
        ctx.set_sun_disc(radius)
        for form in opaque_forms:
            ctx.set_option(V.OPT_FULL_OPAQUE, form)
            for source in sorted(SOURCES):
                _begin(ctx, r, source)
                ctx.accum_add(2)
                out += list(ctx.accum_resolve())
        ctx.set_option(V.OPT_FULL_OPAQUE, 6)
        _begin(ctx, r, "jitter", adaptive=RULE)
        ctx.accum_add(4)
        out += list(ctx.accum_resolve())
        _begin(ctx, r, "corner", hdr=True)
        ctx.accum_add(2)
        out += [_bits(ctx.accum_resolve_hdr("clamp", 1.0)[0])]
        out += list(ctx.shade_rays(*rays, 2, width=W, first_sample=1, n_samples=2))
        out += [_bits(ctx.shade_rays_hdr(*rays, 2, width=W, first_sample=1, n_samples=2)[0])]
    return out


def test_mode_1_with_sampling_off_is_mode_0_on_every_route(ctx, V, refs):
    _load(ctx, refs, on=False, mode=0)
    try:
        before = _routes(ctx, V, refs, refs.rays("corner", 0))
        ctx.set_emitter_importance(1)
        assert ctx.emitter_importance == V.EMIT_POWER and ctx.emitter_sampling is False
        for i, (x, y) in enumerate(zip(_routes(ctx, V, refs, refs.rays("corner", 0)), before)):
            _same(x, y, f"output {i} at mode 1 against mode 0, sampling off")
    finally:
        ctx.set_option(V.OPT_FULL_OPAQUE, 6)
        _reset(ctx)


def test_mode_1_without_emitters_is_mode_0_on_every_route(ctx, V, dragon):
    """the dragon has no emitter: the opaque routes (VRT_OPT_FULL_OPAQUE forms), the general one and the ray batches give the bytes of
    mode 0, with sampling on"""
    _load(ctx, dragon, on=True, mode=0)
    try:
        assert len(ctx.emitters()) == 0 and len(ctx.emitter_cdf()) == 0
        before = _routes(ctx, V, dragon, dragon.rays, (0, 1, 6))
        ctx.set_emitter_importance(1)
        for i, (x, y) in enumerate(zip(_routes(ctx, V, dragon, dragon.rays, (0, 1, 6)), before)):
            _same(x, y, f"dragon output {i} at mode 1 against mode 0")
    finally:
        ctx.set_option(V.OPT_FULL_OPAQUE, 6)
        _reset(ctx)


def test_mode_0_with_sampling_on_is_oracle_emit(ctx, refs, batches, libs):
    """VRT_EMIT_UNIFORM, set explicitly after VRT_EMIT_POWER: the uniform rule's bytes, by oracle_emit itself"""
    _load(ctx, refs, 3, 0.05, mode=1)
    try:
        ctx.set_emitter_importance(0)
        o, d = refs.rays("corner", 0)
        for k in (0, 1):
            ref = oe.shade(libs[0], refs.scene, o, d, 3, 0.05, refs.list, width=W, sample=k)
            mine = refs.sample("corner", 3, 0.05, k, UNIFORM)
            assert np.array_equal(ref[0], mine[0]) and np.array_equal(_bits(ref[2]), _bits(mine[2])), "the two checkers at mode 0"
        for source in sorted(SOURCES):
            _begin(ctx, refs, source)
            assert ctx.accum_add(2) == 2
            _same(ctx.accum_resolve()[0], refs.mean(source, 3, 0.05, 0, 2, UNIFORM), f"{source} at mode 0")
        _begin(ctx, refs, "corner", hdr=True)
        assert ctx.accum_add(2) == 2
        acc = oracle_hdr.Accum(refs.HH, H, W)
        for k in range(2):
            acc.add(refs.sample("corner", 3, 0.05, k, UNIFORM)[2].reshape(H, W, 3))
        _same(_bits(ctx.accum_resolve_hdr("clamp", 1.0)[0]), _bits(acc.mean()), "HDR float mean at mode 0")
        fo, fd, _ = batches["frame"]
        rgba, _ = ctx.shade_rays(fo, fd, 2, width=W, first_sample=0, n_samples=2)
        _same(rgba, _batch_mean(refs, batches, "frame", 3, 0.05, 0, 2, UNIFORM), "shade_rays at mode 0")
    finally:
        _reset(ctx)


# ---- the restart rule ----

def test_changing_the_mode_restarts_a_full_accumulation_only(ctx, refs):
    _load(ctx, refs, 1, 0.0, mode=1)
    try:
        _begin(ctx, refs, "corner")
        assert ctx.accum_add(2) == 2
        ctx.set_emitter_importance(1)
        assert ctx.accum_add(1) == 3, "the same value set again restarted the sums"
        _same(ctx.accum_resolve()[0], refs.mean("corner", 1, 0.0, 0, 3), "power, 2 + 1")
        ctx.set_emitter_importance(0)
        assert ctx.accum_add(2) == 2, "switching to VRT_EMIT_UNIFORM did not restart the sums"
        _same(ctx.accum_resolve()[0], refs.mean("corner", 1, 0.0, 0, 2, UNIFORM), "after the restart at mode 0")
        ctx.set_emitter_importance(1)
        assert ctx.accum_add(1) == 1, "switching to VRT_EMIT_POWER did not restart the sums"
        _same(ctx.accum_resolve()[0], refs.mean("corner", 1, 0.0, 0, 1), "after the restart at mode 1")
        for mode in (0, 1):
            ctx.accum_begin(W, H, 0, mode=mode, jitter=True)
            assert ctx.accum_add(2) == 2
            ctx.set_emitter_importance(0)
            assert ctx.accum_add(1) == 3, f"mode {mode}: the importance mode restarted the sums"
            ctx.set_emitter_importance(1)
            assert ctx.accum_add(1) == 4, f"mode {mode}: the importance mode restarted the sums"
    finally:
        _reset(ctx)


def test_frames_and_the_primary_modes_ignore_the_mode(ctx, refs):
    _load(ctx, refs, 1, 0.0, on=True, mode=0)
    try:
        def outputs():
            out = []
            for mode in (0, 1, 2):
                out += list(ctx.dispatch(W, H, mode))
            out += list(ctx.dispatch_frame(W, H, 2))
            for mode in (0, 1):
                ctx.accum_begin(W, H, 0, mode=mode, jitter=True)
                ctx.accum_add(3)
                out += list(ctx.accum_resolve())
            return out
        before = outputs()
        ctx.set_emitter_importance(1)
        for i, (x, y) in enumerate(zip(outputs(), before)):
            _same(x, y, f"output {i} at mode 1 against mode 0")
    finally:
        _reset(ctx)


# ---- the table: upload, patch, batch end, compaction ----

def test_the_table_after_upload_patch_batch_and_compaction(ctx, libs, O, V):
    w = pw.room(V)
    try:
        r = Refs(libs, O, V, w)
        _load(ctx, r, 3, 0.0)
        assert np.array_equal(ctx.emitters(), r.list) and np.array_equal(ctx.emitter_cdf(), r.cdf) and len(r.cdf) == 257, "after the upload"
        ctx.set_emitter_sampling(0)
        ctx.set_emitter_importance(0)
        assert np.array_equal(ctx.emitter_cdf(), r.cdf), "independent of flag and mode"
        ctx.set_emitter_sampling(1)
        ctx.set_emitter_importance(1)
        # one patch on its own removes a panel voxel
        gx, gy, gz = pw.PANEL[0] + 5, pw.PANEL_Y, pw.PANEL[0] + 9
        w.remove(gx, gy, gz)
        ctx.patch_voxel(w, gx, gy, gz)
        r1 = Refs(libs, O, V, w)
        assert len(r1.cdf) == 256 and [gx, gy, gz, 1] not in r1.list.tolist()
        assert np.array_equal(ctx.emitters(), r1.list) and np.array_equal(ctx.emitter_cdf(), r1.cdf), "after the patch"
        # a batch adds an emitter elsewhere and recolours another
        (ax, ay, az), ac, ai = pw.SPARE
        ctx.patch_begin()
        w.insert(ax, ay, az, ac, 3.0, ai / 255.0, 0.0)
        ctx.patch_voxel(w, ax, ay, az)
        w.insert(pw.PANEL[0], pw.PANEL_Y, pw.PANEL[0], 0xffffffff, 3.0, 200 / 255.0, 0.0)
        ctx.patch_voxel(w, pw.PANEL[0], pw.PANEL_Y, pw.PANEL[0])
        with pytest.raises(V.VrtError):
            ctx.emitter_cdf()   # VRT_E_STATE while the batch is open
        assert ctx._L.vrt_emitter_cdf(ctx._h, None, 0) == -5
        ctx.patch_end()
        r2 = Refs(libs, O, V, w)
        assert len(r2.cdf) == 257 and [ax, ay, az, 1] in r2.list.tolist() and r2.cdf.tolist() != r.cdf.tolist()
        assert np.array_equal(ctx.emitters(), r2.list) and np.array_equal(ctx.emitter_cdf(), r2.cdf), "after the batch's end"
        _begin(ctx, r2, "corner")
        assert ctx.accum_add(2) == 2
        _same(ctx.accum_resolve()[0], r2.mean("corner", 3, 0.0, 0, 2), "an accumulation after the batch's end")
        rgba, _ = ctx.shade_rays(*r2.rays("corner", 0), 2, width=W, first_sample=1)
        _same(rgba, r2.sample("corner", 3, 0.0, 1)[0], "a ray batch after the batch's end")
        ctx.compact()
        assert np.array_equal(ctx.emitters(), r2.list) and np.array_equal(ctx.emitter_cdf(), r2.cdf), "after the compaction"
        assert ctx.accum_add(2) == 2, "the compaction did not restart the sums"
        _same(ctx.accum_resolve()[0], r2.mean("corner", 3, 0.0, 0, 2), "after the compaction")
        # the first min(N, cap) thresholds, and a NULL out with a capacity
        part = np.zeros(5, np.uint32)
        assert ctx._L.vrt_emitter_cdf(ctx._h, part.ctypes.data, 5) == 257 and part.tolist() == r2.cdf[:5].tolist()
        assert ctx._L.vrt_emitter_cdf(ctx._h, None, 5) == -1
    finally:
        w.close()
        _reset(ctx)


def test_state_errors_before_an_upload(V):
    c = V.Context(0)
    try:
        assert c._L.vrt_emitter_cdf(c._h, None, 0) == -5
        with pytest.raises(V.VrtError):
            c.emitter_cdf()
        assert c._L.vrt_emitter_cdf(None, None, 0) == -1
        for bad in (2, -1):
            assert c._L.vrt_set_emitter_importance(c._h, bad) == -1
        assert c._L.vrt_set_emitter_importance(None, 1) == -1
        assert c._L.vrt_set_emitter_importance(c._h, 1) == 0 and c._L.vrt_set_emitter_importance(c._h, 0) == 0
        for bad in (2, -1):
            assert c._L.vrt_set_emitter_sampling(c._h, bad) == -1, "vrt_set_emitter_sampling keeps its 0 / 1 contract"
    finally:
        c.close()


def test_an_invalid_mode_leaves_the_previous_one(ctx, refs):
    _load(ctx, refs, 1, 0.0, mode=1)
    try:
        assert ctx._L.vrt_set_emitter_importance(ctx._h, 7) == -1
        _begin(ctx, refs, "corner")
        assert ctx.accum_add(1) == 1
        _same(ctx.accum_resolve()[0], refs.mean("corner", 1, 0.0, 0, 1), "VRT_EMIT_POWER still holds")
    finally:
        _reset(ctx)


# ---- the profiler ----

def test_profiling_slots_at_mode_1(ctx, refs, batches):
    """as the uniform launches: one slot per ray-batch call, none for vrt_accum_add"""
    o, d, _ = batches["frame"]
    _load(ctx, refs, 3, 0.0)
    try:
        for ns in (1, 3):
            ctx.set_profiling(8)
            ctx.shade_rays(o, d, 2, width=W, first_sample=0, n_samples=ns)
            ms = ctx.profile_read()
            assert len(ms) == 1 and ms[0] > 0.0, f"n_samples={ns}: {len(ms)} slots"
            ctx.shade_rays_hdr(o, d, 2, width=W, first_sample=0, n_samples=ns)
            assert len(ctx.profile_read()) == 1, f"HDR n_samples={ns}"
            ctx.set_profiling(0)
        ctx.set_profiling(8)
        _begin(ctx, refs, "corner")
        ctx.accum_add(2)
        ctx.synchronize()
        assert len(ctx.profile_read()) == 0, "vrt_accum_add took a slot"
    finally:
        ctx.set_profiling(0)
        _reset(ctx)
