"""Emitter sampling (include/vrt.h vrt_set_emitter_sampling) on the MI355X: the samples of VRT_MODE_FULL in accumulations and ray
batches with sampling on, at D in {1, 3} and sun radius in {0, 0.05}, byte for byte (HDR: bit for bit) against the checker
(tests/oracle_paths.c through oracle_emit) in the lamp room with its pane at 72 x 44: a merged lamp and three single emitters, glass in front of the
camera. The list itself against a Python walk after an upload, a patch and a compaction; sampling off, and sampling on in a world
without emitters (the dragon), against oracle_sun's checker and against sampling off. Every reference sample is computed once per
(list, ray source, D, radius, sample) and shared."""
from functools import partial

import numpy as np
import pytest

import emit_worlds as ew
import oracle_adaptive
import oracle_emit as oe
import oracle_hdr
import oracle_lens
import oracle_rays
import oracle_sun as osun
from test_gpu_shade_rays import _ray_mix

pytestmark = pytest.mark.gpu
F = np.float32
W, H = ew.W, ew.H
DEPTHS = (1, 3)
RADII = (0.0, 0.05)
SOURCES = {"corner": (False, False), "jitter": (True, False), "lens": (False, True)}   # jitter, lens
ALL_SOURCES = dict(SOURCES, **{"jitter+lens": (True, True)})   # what Refs and _begin take; the tests here run SOURCES
RULE = (2, 6, 8)   # adaptive: min, max, tolerance


class Refs:
    """The checker's side for one world: its scene, its list, each sample's rays and each sample's result, computed once"""

    def __init__(self, libs, O, V, world, pose=ew.POSE, lens=ew.LENS, W=W, H=H):
        self.E, self.S, self.R, self.LL, self.HH = libs
        self.W, self.H = W, H
        self.tex, self.dim = world.flatten()
        ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
        self.cam = (ip, iv, cp)
        self.scene = O.make_scene(self.tex, self.dim, ip, iv, cp)
        self.list = oe.walk(world.records()[0])
        self.lens = lens
        self._rays = {}
        self._samples = {}

    def rays(self, source, k):
        W, H = self.W, self.H
        jitter, lens = ALL_SOURCES[source]
        key = (source, k if (jitter or lens) else 0)
        if key not in self._rays:
            if not jitter and not lens:
                self._rays[key] = oracle_rays.frame_rays(self.R, self.scene, W, H)
            else:
                ap, fo = self.lens if lens else (0.0, 1.0)
                o = np.zeros((H * W, 3), F)
                d = np.zeros((H * W, 3), F)
                for py in range(H):
                    for px in range(W):
                        _, o[py * W + px], d[py * W + px] = oracle_lens.ray(self.LL, self.scene, W, H, px, py, k, ap, fo, jitter)
                self._rays[key] = (o, d)
        return self._rays[key]

    def sample(self, source, D, radius, k, on=True):
        """-> (rgba8[H*W,4], id_dist[H*W,2], rgb float32[H*W,3]) of sample k (an index modulo 2^32)"""
        k &= 0xFFFFFFFF
        key = (source, D, radius, k, on)
        if key not in self._samples:
            o, d = self.rays(source, k)
            self._samples[key] = oe.shade(self.E, self.scene, o, d, D, radius, self.list if on else None, width=self.W, sample=k)
        return self._samples[key]

    def mean(self, source, D, radius, first, n, on=True):
        total = sum(self.sample(source, D, radius, first + k, on)[0].astype(np.uint64) for k in range(n))
        out = ((total + n // 2) // n).astype(np.uint8)
        out[:, 3] = 255
        return out.reshape(self.H, self.W, 4)

    def frame_id(self):
        return self.sample("corner", 1, 0.0, 0)[1].reshape(self.H, self.W, 2)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("oracle_emit")
    return oe.build(tmp), osun.build(tmp), oracle_rays.build(tmp), oracle_lens.build(tmp), oracle_hdr.build(tmp)


@pytest.fixture(scope="module")
def refs(libs, O, V):
    w = ew.lamp_room(V)
    r = Refs(libs, O, V, w)
    w.close()
    assert len(r.list) == 4 and r.list[:, 3].max() == 2
    return r


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _load(c, r, depth=1, radius=0.0, on=True, variant=0):
    c.upload_octree(r.tex, r.dim)
    c.set_camera(*r.cam)
    c.set_params(c.default_params())
    c.set_variant(variant)
    c.set_lens(0.0, 1.0)
    c.set_path_depth(depth)
    c.set_sun_disc(radius)
    c.set_emitter_sampling(on)


def _reset(c):
    c.set_variant(0)
    c.set_lens(0.0, 1.0)
    c.set_path_depth(1)
    c.set_sun_disc(0.0)
    c.set_emitter_sampling(0)


def _same(got, ref, what, W=W):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} against {ref.shape}"
    if not np.array_equal(got, ref):
        g, r = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
        bad = np.argwhere(np.any(g != r, axis=-1))[:, 0]
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(r)} differ; first at {i} (x {i % W}, y {i // W}): got {g[i]} want {r[i]}")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _begin(c, r, source, first=0, W=W, H=H, **kw):
    jitter, lens = ALL_SOURCES[source]
    c.set_lens(*(r.lens if lens else (0.0, 1.0)))
    c.accum_begin(W, H, first, mode=2, jitter=jitter, **kw)


def _forms(c, r, source, D, radius, on=True, W=W, H=H, what=None):
    """plain, adaptive and HDR accumulations of one (source, D, radius): samples 0 .. 7 added as 3 + 5, an adaptive run of six
    rounds, an HDR run of 1 + 2; W, H: the frame r was built for; what: the name the failure messages carry"""
    what = what or f"{source} D={D} radius {radius}"
    same, begin = partial(_same, W=W), partial(_begin, W=W, H=H)
    begin(c, r, source)
    assert c.accum_add(3) == 3
    same(c.accum_resolve()[0], r.mean(source, D, radius, 0, 3, on), f"{what} rgba8 after 3")
    assert c.accum_add(5) == 8
    got = c.accum_resolve()
    same(got[0], r.mean(source, D, radius, 0, 8, on), f"{what} rgba8 after 3 + 5")
    same(got[1], r.frame_id(), f"{what} id_dist")
    begin(c, r, source)
    assert c.accum_add(8) == 8
    same(c.accum_resolve()[0], got[0], f"{what}: 8 in one add against 3 + 5")
    begin(c, r, source, adaptive=RULE)
    assert c.accum_add(2) == 2 and c.accum_add(4) == 6
    got = c.accum_resolve()
    counts, active = c.accum_counts()
    st = oracle_adaptive.accumulate(lambda k: r.sample(source, D, radius, k, on)[0].reshape(H, W, 4), H, W, 0, 6, RULE, np.int64)
    assert np.array_equal(counts, st.counts()), f"{what}: adaptive counts"
    assert active == int(st.active(RULE).sum())
    same(got[0], st.resolve(), f"{what} adaptive rgba8")
    same(got[1], r.frame_id(), f"{what} adaptive id_dist")
    begin(c, r, source, hdr=True)
    assert c.accum_add(1) == 1 and c.accum_add(2) == 3
    acc = oracle_hdr.Accum(r.HH, H, W)
    for k in range(3):
        acc.add(r.sample(source, D, radius, k, on)[2].reshape(H, W, 3))
    want = acc.mean()
    for op, e in (("clamp", 1.0), ("reinhard", 1.7)):
        rgb, rgba, _ = c.accum_resolve_hdr(op, e)
        same(_bits(rgb), _bits(want), f"{what} float mean ({op})")
        same(rgba, oracle_hdr.tonemap(r.HH, want, op, e), f"{what} {op} bytes")
    same(c.accum_resolve()[0], r.mean(source, D, radius, 0, 3, on), f"{what} the bytes beside the floats")


# ---- the accumulation ----

@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_accumulations_are_the_checkers_mean(ctx, refs, source, D, radius):
    _load(ctx, refs, D, radius)
    try:
        _forms(ctx, refs, source, D, radius)
    finally:
        _reset(ctx)


def test_a_first_sample_of_2_to_the_32_minus_2(ctx, refs):
    _load(ctx, refs, 3, 0.05)
    first = (1 << 32) - 2
    try:
        for source in ("corner", "jitter"):
            _begin(ctx, refs, source, first=first)
            assert ctx.accum_add(4) == 4   # 2^32 - 2, 2^32 - 1, 0, 1
            _same(ctx.accum_resolve()[0], refs.mean(source, 3, 0.05, first, 4), f"{source} first sample 2^32 - 2")
    finally:
        _reset(ctx)


def test_the_record_array_kernels(ctx, refs):
    """vrt_set_variant(1): the kernels over EmitPaths<v1::Trav>"""
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
    """name -> (origins, dirs, cache): the frame's 3168 rays, and a list of 100 arbitrary ones -- origins in glass, in solids, on
    faces, outside the world, un-normalised and axis-parallel directions (test_gpu_shade_rays.py's mix)"""
    fo, fd = refs.rays("corner", 0)
    ao, ad = _ray_mix(np.random.default_rng(43), 100, (ew.LO, ew.LO, ew.LO), (ew.HI + 1, ew.HI + 1, ew.HI + 1),
                      ((ew.PANE_X, ew.PANE_Y[0], ew.PANE_Z[0]), (ew.PANE_X + 1, ew.PANE_Y[1], ew.PANE_Z[1])),
                      ((ew.TABLE[0], ew.TABLE_Y, ew.TABLE[0]), (ew.TABLE[1], ew.TABLE_Y + 1, ew.TABLE[1])))
    return {"frame": (fo, fd, {}), "list": (ao, ad, {})}


def _width(name):
    return W if name == "frame" else 1


def _batch_sample(refs, batches, name, D, radius, k, on=True):
    o, d, cache = batches[name]
    key = (D, radius, k, on)
    if key not in cache:
        cache[key] = oe.shade(refs.E, refs.scene, o, d, D, radius, refs.list if on else None, width=_width(name), sample=k)
    return cache[key]


def _batch_mean(refs, batches, name, D, radius, first, n, on=True):
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


# ---- the list: upload, patch, compaction ----

def test_the_list_after_upload_patch_and_compaction(ctx, libs, O, V):
    w = ew.lamp_room(V)
    try:
        r = Refs(libs, O, V, w)
        _load(ctx, r, 3, 0.0)
        assert np.array_equal(ctx.emitters(), r.list) and len(r.list) == 4, "after the upload"
        _begin(ctx, r, "corner")
        assert ctx.accum_add(2) == 2
        _same(ctx.accum_resolve()[0], r.mean("corner", 3, 0.0, 0, 2), "after the upload")
        # a patch that removes one single emitter and adds another
        (gx, gy, gz), _ = ew.SINGLES[0]
        (ax, ay, az), ac = ew.SPARE
        ctx.patch_begin()
        w.remove(gx, gy, gz)
        assert ctx.patch_voxel(w, gx, gy, gz) is not None
        w.insert(ax, ay, az, ac, 3.0, 1.0, 0.0)
        assert ctx.patch_voxel(w, ax, ay, az) is not None
        with pytest.raises(V.VrtError):
            ctx.emitters()   # VRT_E_STATE while the batch is open
        ctx.patch_end()
        r2 = Refs(libs, O, V, w)
        assert [ax, ay, az, 1] in r2.list.tolist() and [gx, gy, gz, 1] not in r2.list.tolist() and len(r2.list) == 4
        assert np.array_equal(ctx.emitters(), r2.list), "after the patch"
        assert ctx.accum_add(3) == 3, "the patch did not restart the sums"
        _same(ctx.accum_resolve()[0], r2.mean("corner", 3, 0.0, 0, 3), "after the patch")
        rgba, _ = ctx.shade_rays(*r2.rays("corner", 0), 2, width=W, first_sample=1)
        _same(rgba, r2.sample("corner", 3, 0.0, 1)[0], "a ray batch after the patch")
        ctx.compact()
        assert np.array_equal(ctx.emitters(), r2.list), "after the compaction"
        assert ctx.accum_add(2) == 2, "the compaction did not restart the sums"
        _same(ctx.accum_resolve()[0], r2.mean("corner", 3, 0.0, 0, 2), "after the compaction")
    finally:
        w.close()
        _reset(ctx)


def test_emitters_before_an_upload_is_a_state_error(V):
    c = V.Context(0)
    try:
        assert c._L.vrt_emitters(c._h, None, 0) == -5
        with pytest.raises(V.VrtError):
            c.emitters()
        assert c._L.vrt_emitters(None, None, 0) == -1
        for bad in (2, -1):
            assert c._L.vrt_set_emitter_sampling(c._h, bad) == -1
        assert c._L.vrt_set_emitter_sampling(None, 1) == -1
    finally:
        c.close()


# ---- off is today's output ----

def test_sampling_off_is_oracle_sun(ctx, refs, batches):
    _load(ctx, refs, 3, 0.05, on=True)
    try:
        _begin(ctx, refs, "corner")
        ctx.accum_add(1)
        ctx.set_emitter_sampling(0)
        assert ctx.emitter_sampling is False
        assert np.array_equal(ctx.emitters(), refs.list), "vrt_emitters works with sampling off"
        for D, radius in ((1, 0.0), (3, 0.05)):
            ctx.set_path_depth(D)
            ctx.set_sun_disc(radius)
            for source in sorted(SOURCES):
                total = None
                for k in range(2):
                    o, d = refs.rays(source, k)
                    s = osun.shade(refs.S, refs.scene, o, d, D, radius, width=W, sample=k)[0].astype(np.uint64)
                    total = s if total is None else total + s
                want = ((total + 1) // 2).astype(np.uint8)
                want[:, 3] = 255
                _begin(ctx, refs, source)
                assert ctx.accum_add(2) == 2
                _same(ctx.accum_resolve()[0], want.reshape(H, W, 4), f"{source} D={D} radius {radius} with sampling off")
            o, d, _ = batches["frame"]
            rgba, _ = ctx.shade_rays(o, d, 2, width=W, first_sample=3)
            _same(rgba, osun.shade(refs.S, refs.scene, o, d, D, radius, width=W, sample=3)[0], f"shade_rays D={D} radius {radius} with sampling off")
    finally:
        _reset(ctx)


@pytest.fixture(scope="module")
def dragon(libs, O, V, product_scenes):
    class Dragon:
        pass
    r = Dragon()
    r.tex, r.dim = product_scenes["dragon"]
    ip, iv, cp, _ = V.camera_block(ew.DRAGON_POSE[:3], ew.DRAGON_POSE[3], ew.DRAGON_POSE[4], W, H)
    r.cam = (ip, iv, cp)
    r.lens = (0.8, 80.0)
    r.scene = O.make_scene(r.tex, r.dim, ip, iv, cp)
    r.rays = oracle_rays.frame_rays(libs[2], r.scene, W, H)
    return r


def test_sampling_on_without_emitters_is_sampling_off_on_every_route(ctx, V, dragon):
    """the dragon has no emitter: every route -- the opaque ones (VRT_OPT_FULL_OPAQUE forms), the general one, ray batches, plain,
    adaptive and HDR -- gives the bytes of sampling off"""
    def outputs():
        out = []
        for D, radius in ((1, 0.0), (3, 0.05)):
            ctx.set_path_depth(D)
            ctx.set_sun_disc(radius)
            for form in (0, 1, 6):
                ctx.set_option(V.OPT_FULL_OPAQUE, form)
                for source in sorted(SOURCES):
                    _begin(ctx, dragon, source)
                    ctx.accum_add(2)
                    out += list(ctx.accum_resolve())
            ctx.set_option(V.OPT_FULL_OPAQUE, 6)
            _begin(ctx, dragon, "jitter", adaptive=RULE)
            ctx.accum_add(4)
            out += list(ctx.accum_resolve())
            _begin(ctx, dragon, "corner", hdr=True)
            ctx.accum_add(2)
            out += [_bits(ctx.accum_resolve_hdr("clamp", 1.0)[0])]
            out += list(ctx.shade_rays(*dragon.rays, 2, width=W, first_sample=1, n_samples=2))
            out += [_bits(ctx.shade_rays_hdr(*dragon.rays, 2, width=W, first_sample=1, n_samples=2)[0])]
        return out
    _load(ctx, dragon, on=False)
    try:
        assert len(ctx.emitters()) == 0
        before = outputs()
        ctx.set_emitter_sampling(1)
        for i, (x, y) in enumerate(zip(outputs(), before)):
            _same(x, y, f"dragon output {i} with sampling on against off")
    finally:
        ctx.set_option(V.OPT_FULL_OPAQUE, 6)
        _reset(ctx)


# ---- the flag itself ----

def test_toggling_restarts_a_full_accumulation_only(ctx, refs):
    _load(ctx, refs, 1, 0.0, on=True)
    try:
        _begin(ctx, refs, "corner")
        assert ctx.accum_add(2) == 2
        ctx.set_emitter_sampling(1)
        assert ctx.accum_add(1) == 3, "the same value set again restarted the sums"
        _same(ctx.accum_resolve()[0], refs.mean("corner", 1, 0.0, 0, 3), "sampling on, 2 + 1")
        ctx.set_emitter_sampling(0)
        assert ctx.accum_add(2) == 2, "switching sampling off did not restart the sums"
        _same(ctx.accum_resolve()[0], refs.mean("corner", 1, 0.0, 0, 2, on=False), "after the restart with sampling off")
        ctx.set_emitter_sampling(1)
        assert ctx.accum_add(1) == 1, "switching sampling on did not restart the sums"
        for mode in (0, 1):
            ctx.accum_begin(W, H, 0, mode=mode, jitter=True)
            assert ctx.accum_add(2) == 2
            ctx.set_emitter_sampling(0)
            assert ctx.accum_add(1) == 3, f"mode {mode}: the flag restarted the sums"
            ctx.set_emitter_sampling(1)
            assert ctx.accum_add(1) == 4, f"mode {mode}: the flag restarted the sums"
    finally:
        _reset(ctx)


def test_frames_and_the_primary_modes_ignore_the_flag(ctx, refs):
    _load(ctx, refs, 1, 0.0, on=False)
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
        ctx.set_emitter_sampling(1)
        for i, (x, y) in enumerate(zip(outputs(), before)):
            _same(x, y, f"output {i} with sampling on against off")
    finally:
        _reset(ctx)


def test_profiling_slots_with_sampling_on(ctx, refs, batches):
    """one slot per ray-batch call, none for vrt_accum_add"""
    o, d, _ = batches["frame"]
    _load(ctx, refs, 3, 0.0)
    try:
        for ns in (1, 3):
            ctx.set_profiling(8)
            ctx.shade_rays(o, d, 2, width=W, first_sample=0, n_samples=ns)
            ms = ctx.profile_read()
            assert len(ms) == 1 and ms[0] > 0.0, f"n_samples={ns}: {len(ms)} slots"
            ctx.set_profiling(0)
        ctx.set_profiling(8)
        _begin(ctx, refs, "corner")
        ctx.accum_add(2)
        ctx.synchronize()
        assert len(ctx.profile_read()) == 0, "vrt_accum_add took a slot"
    finally:
        ctx.set_profiling(0)
        _reset(ctx)
