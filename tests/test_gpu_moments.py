"""Luminance moments of an HDR accumulation on the MI355X (vrt_accum_keep_moments, vrt_accum_variance{,_device}) against the checker
(tests/oracle_moments.c: M1-M3 of include/vrt.h), bit for bit: floats are compared as their uint32 views. test_gpu_accum_hdr.py's
scenes, frame sizes, FIRST and N, and 43 x 21 -- the three modes, the four ray sources, plain and adaptive, both record-array
traversals, one case per family of path tracer kernels (depth 3, a sun disc, emitter sampling uniform, by power and with MIS), the
opaque routes -- then what must hold around them: any split of the samples, the restart rule, the setter's timing, a caller's
stream, everything else the accumulation returns with and without moments, the variance-guided resolve against the stateless
filter on the device and against the checker chain, one sample falling back to the spatial estimate, the error codes and buffer
growth. Every reference is computed once per (scene, size, mode, source, rule) and shared."""
import numpy as np
import pytest

import guide_worlds as GW
import oracle_filter_var as FV
import oracle_guides as G
import oracle_hdr
import oracle_moments as OM
import test_gpu_emit_mis as tem
import test_gpu_sun_disc as tsd
from test_gpu_accum_hdr import FIRST, LENS, N, RULE, SOURCES
from test_gpu_accum_jitter import SCENES, _same, _setup

pytestmark = pytest.mark.gpu

RAGGED = (43, 21)          # partial 8 x 8 tiles on the right and at the bottom
SWEPT = dict(sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=1.0, sigma_lum=2.0)     # tests/test_gpu_filter_var.py's
UNKNOWN = OM.VAR_UNKNOWN


@pytest.fixture(scope="module")
def ML(tmp_path_factory):
    return OM.build(tmp_path_factory.mktemp("oracle_moments"))


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(ctx):
    yield
    ctx.set_variant(0)
    ctx.set_lens(0.0, 1.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, ref, what):
    got, ref = _bits(got), _bits(ref)
    if got.ndim == 2:
        got, ref = got[..., None], ref[..., None]
    _same(got, ref, what)


def _lens_of(name, source):
    return LENS[name] if SOURCES[source][1] else (0.0, 1.0)


_refs = {}


def _reference(ML, scene, name, W, H, mode, first, n, source, rule, pose=None):
    """the checker's accumulation of samples first .. first + n - 1 (rounds, when adaptive), computed once"""
    key = (name, W, H, mode, first, n, source, rule, pose)
    if key not in _refs:
        acc = OM.Accum(ML, H, W, rule)
        for k in range(n):
            acc.add(oracle_hdr.render(ML, scene, W, H, mode, (first + k) & 0xFFFFFFFF, SOURCES[source][0], *_lens_of(name, source)))
        _refs[key] = acc
    return _refs[key]


def _accumulate(ctx, W, H, mode, first, chunks, name, source, rule, moments=True):
    ctx.set_lens(*_lens_of(name, source))
    ctx.accum_begin(W, H, first, mode=mode, jitter=SOURCES[source][0], adaptive=rule, hdr=True, moments=moments)
    total = 0
    for n in chunks:
        total += n
        assert ctx.accum_add(n) == total


def _scene(ctx, V, O, product_scenes, name, size=None, records=None):
    m, W, H, pose = SCENES[name]
    if size:
        W, H = size
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose, records=records)
    return scene, W, H


def _check(ctx, ML, scene, name, W, H, mode, source, rule, what):
    acc = _reference(ML, scene, name, W, H, mode, FIRST, N, source, rule)
    _accumulate(ctx, W, H, mode, FIRST, [N], name, source, rule)
    tag = f"{what} {W}x{H} mode {mode} {source} {'adaptive' if rule else 'plain'}"
    _same_bits(ctx.accum_variance(), acc.variance(), f"{tag}: variance")
    _same_bits(ctx.accum_resolve_hdr()[0], acc.mean(), f"{tag}: the float mean beside it")
    _same(ctx.accum_resolve()[0], acc.resolve_bytes(), f"{tag}: the byte resolve beside it")
    if rule:
        _same(ctx.accum_counts()[0][..., None], acc.counts()[..., None], f"{tag}: counts")
    return acc


# ---- every kernel route ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", [None, RULE], ids=["plain", "adaptive"])
@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("name,mode", [("dragon", 2), ("room_outside", 2), ("dragon", 0), ("dragon", 1), ("nature", 2)])
@pytest.mark.parametrize("size", [None, RAGGED], ids=["own", "43x21"])
def test_variance_is_the_checkers(ctx, V, O, ML, product_scenes, size, name, mode, source, rule):
    """the dragon is opaque: from the corner pass 1 + the sample-looped bounce (its sky pixels on the product shortcut), with jitter
    or a lens the one-kernel chain; the room takes the general path tracer; modes 0 and 1 the repeat kernels from the corner and the
    sample-looped primary kernels otherwise"""
    scene, W, H = _scene(ctx, V, O, product_scenes, name, size)
    acc = _check(ctx, ML, scene, name, W, H, mode, source, rule, name)
    var = acc.variance()
    if mode != 2 and source == "corner":
        assert not _bits(var).any()                      # every sample is the frame: exactly +0 everywhere
    else:
        assert (var > 0).any() and np.isfinite(var).all()


@pytest.mark.parametrize("variant", [4, 1])
def test_both_record_array_traversals(ctx, V, O, ML, product_scenes, variant):
    scene, W, H = _scene(ctx, V, O, product_scenes, "room_outside")
    ctx.set_variant(variant)
    for mode, source, rule in ((2, "corner", None), (2, "jitter_lens", RULE), (1, "jitter", None), (1, "lens", RULE), (0, "corner", None)):
        _check(ctx, ML, scene, "room_outside", W, H, mode, source, rule, f"variant {variant}")


def test_record_only_upload(ctx, V, O, ML, product_scenes):
    import os
    from conftest import MAPS
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    rec = w.records()
    w.close()
    scene, W, H = _scene(ctx, V, O, product_scenes, "dragon", records=rec)
    for mode, source, rule in ((2, "corner", None), (2, "jitter", RULE), (1, "jitter_lens", None)):
        _check(ctx, ML, scene, "dragon", W, H, mode, source, rule, "records")


@pytest.mark.parametrize("form", [0, 1, 6])
def test_every_opaque_route_on_the_dragon(ctx, V, O, ML, product_scenes, form):
    """VRT_OPT_FULL_OPAQUE 1 and 6: pass 1 + bounce from the corner, the one-kernel chain with jitter; 0: the general path tracer"""
    scene, W, H = _scene(ctx, V, O, product_scenes, "dragon", RAGGED)
    ctx.set_option(V.OPT_FULL_OPAQUE, form)
    try:
        for source, rule in (("corner", None), ("corner", RULE), ("jitter", None), ("lens", RULE)):
            _check(ctx, ML, scene, "dragon", W, H, 2, source, rule, f"VRT_OPT_FULL_OPAQUE {form}")
    finally:
        ctx.set_option(V.OPT_FULL_OPAQUE, 6)


# ---- one case per family of path tracer kernels ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sun_refs(tmp_path_factory, O, V, product_scenes):
    return tsd.Refs(tmp_path_factory.mktemp("oracle_sun_moments"), O, V, product_scenes)


@pytest.fixture(scope="module")
def mis_refs(tmp_path_factory, O, V):
    tmp = tmp_path_factory.mktemp("oracle_mis_moments")
    libs = (tem.oe.build(tmp), tem.osun.build(tmp), tem.oracle_rays.build(tmp), tem.oracle_lens.build(tmp), oracle_hdr.build(tmp), tem.om.build(tmp))
    w = tem.mw.room(V)
    r = tem.Refs(libs, O, V, w)
    w.close()
    return r


def _family(ctx, ML, sample, W, H, first, rule, what, noisy=True):
    """three samples (rounds) added as 1 + 2 against the checker's sums of sample(k) -> float32[H,W,3]; noisy: the samples differ"""
    acc = OM.Accum(ML, H, W, rule)
    for k in range(3):
        acc.add(sample(first + k))
    assert ctx.accum_add(1) == 1 and ctx.accum_add(2) == 3
    _same_bits(ctx.accum_variance(), acc.variance(), f"{what}: variance")
    _same_bits(ctx.accum_resolve_hdr()[0], acc.mean(), f"{what}: float mean")
    assert not noisy or (acc.variance() > 0).any()


@pytest.mark.parametrize("D,radius", [(3, 0.0), (1, tsd.R_SOFT), (3, tsd.R_SOFT)], ids=["deep", "sun", "deep_sun"])
@pytest.mark.parametrize("world,source", [("dragon", "corner"), ("dragon", "jitter"), ("room", "lens"), ("unit", "corner")])
def test_depth_and_sun_disc(ctx, ML, sun_refs, world, source, D, radius):
    """DeepPaths<...> and SunPaths<...>: the dragon's opaque routes (bounce from the corner, the chain with jitter), the room's
    general kernel, the unit-internal stream's record-array kernels (eight voxels under a point sun: its samples need not differ)"""
    tsd._load(ctx, sun_refs, world, D, radius)
    try:
        for rule in (None, (2, 4, 0)):
            tsd._begin(ctx, world, source, adaptive=rule, hdr=True, moments=True)
            _family(ctx, ML, lambda k: sun_refs.sample(world, source, D, radius, k)[2].reshape(tsd.H, tsd.W, 3), tsd.W, tsd.H, tsd.FIRST, rule,
                    f"{world} {source} D={D} radius {radius} {'adaptive' if rule else 'plain'}", noisy=world != "unit")
    finally:
        tsd._reset(ctx)


@pytest.mark.parametrize("on,mode,mis", [(tem.UNIFORM, 0, 0), (tem.POWER, 1, 0), (tem.MIS, 1, 1)], ids=["uniform", "power", "power_mis"])
@pytest.mark.parametrize("source", ["corner", "jitter", "lens"])
def test_emitter_sampling(ctx, ML, mis_refs, source, on, mode, mis):
    """EmitPaths<...>, EmitPowerPaths<...> and EmitMisPaths<...> in the lamp room, at depth 3 with a sun disc; variant 1 once"""
    for variant, rule in ((0, None), (0, tem.RULE), (1, None)):
        tem._load(ctx, mis_refs, 3, 0.05, True, variant, mode, mis)
        try:
            tem._begin(ctx, mis_refs, source, adaptive=rule, hdr=True, moments=True)
            _family(ctx, ML, lambda k: mis_refs.sample(source, 3, 0.05, k, on)[2].reshape(tem.H, tem.W, 3), tem.W, tem.H, 0, rule,
                    f"{source} {on} variant {variant} {'adaptive' if rule else 'plain'}")
        finally:
            tem._reset(ctx)


# ---- what holds around them ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", [None, RULE], ids=["plain", "adaptive"])
@pytest.mark.parametrize("name,mode,source", [("dragon", 2, "corner"), ("dragon", 2, "jitter"), ("room_outside", 2, "lens"),
                                              ("dragon", 1, "corner"), ("dragon", 0, "jitter_lens")])
def test_three_plus_five_adds_equal_eight(ctx, V, O, product_scenes, name, mode, source, rule):
    _, W, H = _scene(ctx, V, O, product_scenes, name)
    _accumulate(ctx, W, H, mode, 11, [8], name, source, rule)
    ref = ctx.accum_variance()
    for chunks in ([3, 5], [1] * 8):
        _accumulate(ctx, W, H, mode, 11, chunks[:1], name, source, rule)
        ctx.accum_variance()                                  # a resolve between the adds changes nothing
        for n, total in zip(chunks[1:], np.cumsum(chunks)[1:]):
            assert ctx.accum_add(n) == total
        _same_bits(ctx.accum_variance(), ref, f"{name} mode {mode} {source} {chunks}")


def test_one_sample_is_unknown_everywhere(ctx, V, O, product_scenes):
    _, W, H = _scene(ctx, V, O, product_scenes, "room_outside", RAGGED)
    for mode, source in ((2, "jitter"), (1, "corner")):
        _accumulate(ctx, W, H, mode, 0, [1], "room_outside", source, None)
        assert np.all(_bits(ctx.accum_variance()) == _bits(UNKNOWN))
    _accumulate(ctx, W, H, 2, 0, [1], "room_outside", "jitter", RULE)      # one round of an adaptive accumulation
    assert np.all(_bits(ctx.accum_variance()) == _bits(UNKNOWN))


def test_a_camera_change_restarts_the_sums(ctx, V, O, ML, product_scenes):
    m, W, H, pose = SCENES["room_outside"]
    _setup(ctx, V, O, product_scenes, m, W, H, pose)
    ctx.accum_begin(W, H, 3, mode=2, jitter=True, hdr=True, moments=True)
    assert ctx.accum_add(4) == 4
    moved = (pose[0] + 1.0, pose[1], pose[2], pose[3], pose[4])
    ip, iv, cp, _ = V.camera_block(moved[:3], moved[3], moved[4], W, H)
    ctx.set_camera(ip, iv, cp)
    assert ctx.accum_add(2) == 2
    tex, dim = product_scenes[m]
    acc = _reference(ML, O.make_scene(tex, dim, ip, iv, cp), "room_outside", W, H, 2, 3, 2, "jitter", None, pose=moved)
    _same_bits(ctx.accum_variance(), acc.variance(), "samples 3, 4 from the new camera alone")


def test_keep_moments_is_read_at_the_begin_only(ctx, V, O, product_scenes):
    _, W, H = _scene(ctx, V, O, product_scenes, "dragon")
    L, h = ctx._L, ctx._h
    ctx.accum_begin(W, H, 0, mode=2, hdr=True, moments=True)
    assert ctx.accum_add(2) == 2
    ref = ctx.accum_variance()
    assert L.vrt_accum_keep_moments(h, 0) == 0               # a running accumulation keeps its moments, and is not restarted
    assert ctx.accum_add(1) == 3
    var3 = ctx.accum_variance()
    ctx.accum_begin(W, H, 0, mode=2, hdr=True, moments=True)
    assert ctx.accum_add(3) == 3
    _same_bits(ctx.accum_variance(), var3, "2 + 1 samples across the setter")
    assert not np.array_equal(_bits(ref), _bits(var3))
    ctx.accum_begin(W, H, 0, mode=2, hdr=True, moments=False)
    assert ctx.accum_add(1) == 1
    assert L.vrt_accum_keep_moments(h, 1) == 0               # ... and one begun without stays without
    assert ctx.accum_add(1) == 2
    assert L.vrt_accum_variance(h, ref.ctypes.data) == -5
    assert L.vrt_accum_keep_hdr(h, 0) == 0                   # moments without HDR are ignored: a plain accumulation
    assert L.vrt_accum_begin_ex(h, W, H, 2, 0, 0) == 0
    assert ctx.accum_add(2) == 2
    assert L.vrt_accum_variance(h, ref.ctypes.data) == -5 and L.vrt_accum_resolve_hdr(h, None, None, None, None) == -5
    plain = ctx.accum_resolve()
    assert L.vrt_accum_keep_moments(h, 0) == 0
    assert L.vrt_accum_begin_ex(h, W, H, 2, 0, 0) == 0
    assert ctx.accum_add(2) == 2
    for a, b in zip(ctx.accum_resolve(), plain):
        assert np.array_equal(a, b)


def test_the_device_form_on_a_callers_stream_is_the_host_form(ctx, V, O, product_scenes):
    import torch
    _, W, H = _scene(ctx, V, O, product_scenes, "room_outside")
    d_var = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    for rule in (None, RULE):
        _accumulate(ctx, W, H, 2, 0, [4], "room_outside", "jitter", rule)
        for stream in (None, side.cuda_stream, None):
            d_var.zero_()
            torch.cuda.synchronize()
            ctx.accum_variance_device(d_var.data_ptr(), stream=stream)
            torch.cuda.synchronize()
            host = ctx.accum_variance()                         # (synchronises the context's stream)
            _same_bits(d_var.cpu().numpy(), host, f"stream {stream}")
        ctx.accum_variance_device(d_var.data_ptr(), stream=side.cuda_stream)     # ... and an add queued behind a read on the side stream
        assert ctx.accum_add(2) == 6
        torch.cuda.synchronize()
        _same_bits(d_var.cpu().numpy(), host, "the read before the add")
        assert not np.array_equal(_bits(ctx.accum_variance()), _bits(host))


@pytest.mark.parametrize("rule", [None, RULE], ids=["plain", "adaptive"])
@pytest.mark.parametrize("name,mode,source", [("dragon", 2, "corner"), ("dragon", 2, "jitter_lens"), ("room_outside", 2, "jitter"),
                                              ("dragon", 1, "corner"), ("dragon", 1, "lens")])
def test_everything_else_is_identical_with_and_without_moments(ctx, V, O, product_scenes, name, mode, source, rule):
    _, W, H = _scene(ctx, V, O, product_scenes, name, RAGGED if mode == 1 else None)

    def run(moments):
        _accumulate(ctx, W, H, mode, FIRST, [2, 3], name, source, rule, moments=moments)
        if moments:
            ctx.accum_variance()
        out = ctx.accum_resolve() + ctx.accum_resolve_hdr("reinhard", 1.5) + tuple(ctx.accum_guides()[k] for k in G.KEYS)
        out += ctx.accum_resolve_hdr_filtered({"levels": 2, "demodulate": True})
        if rule:
            out += (ctx.accum_counts()[0],)
        return out

    without, with_moments = run(False), run(True)
    assert len(without) == len(with_moments) == (13 if rule else 12)
    for i, (a, b) in enumerate(zip(without, with_moments)):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"output {i} differs with moments on"


# ---- the variance-guided resolve -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def LV(tmp_path_factory):
    return FV.build(tmp_path_factory.mktemp("oracle_filter_var_moments"))


@pytest.fixture(scope="module")
def LG(tmp_path_factory):
    return G.build(tmp_path_factory.mktemp("oracle_guides_moments"))


@pytest.fixture(scope="module")
def worlds(V, O):
    out = {}
    for name in ("room", "lamp"):
        w = GW.world(V, name)
        tex, dim = w.flatten()
        w.close()
        for size in ((GW.W, GW.H), GW.RAGGED):
            cam = GW.camera(V, name, size)
            out[name, size] = (tex, dim, cam, O.make_scene(tex, dim, *cam))
    return out


_chains = {}


def _chain(ML, LG, worlds, name, source, size, first, n, rule=None):
    """-> (the checker's Accum, its guide planes) of samples first .. first + n - 1 in GW's frames, computed once"""
    key = (name, source, size, first, n, rule)
    if key not in _chains:
        jitter, _ = GW.SOURCES[source]
        lens = GW.lens_of(name, source)
        scene = worlds[name, size][3]
        acc = OM.Accum(ML, size[1], size[0], rule)
        for k in range(first, first + n):
            acc.add(oracle_hdr.render(ML, scene, size[0], size[1], 2, k, jitter, *lens))
        _chains[key] = (acc, G.planes(LG, scene, size[0], size[1], first, n, jitter, *lens)[0])
    return _chains[key]


def _open(ctx, worlds, name, source, size, moments=True, rule=None):
    tex, dim, cam, _ = worlds[name, size]
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    ctx.set_camera(*cam)
    ctx.set_lens(*GW.lens_of(name, source))
    ctx.accum_begin(size[0], size[1], GW.FIRST, mode=2, jitter=GW.SOURCES[source][0], adaptive=rule, hdr=True, moments=moments)


def _same_all(got, want, what):
    for g, w, part in zip(got, want, ("floats", "bytes", "variance")):
        assert g.dtype == w.dtype and g.shape == w.shape
        bad = np.argwhere(g.view(np.uint8).reshape(g.shape[0], g.shape[1], -1) != w.view(np.uint8).reshape(w.shape[0], w.shape[1], -1))
        assert len(bad) == 0, f"{what}: {part}: {len(np.unique(bad[:, :2], axis=0))} pixels differ; first at (x={bad[0][1]}, y={bad[0][0]})"


@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("source", ["jitter", "lens"])
@pytest.mark.parametrize("name", ["room", "lamp"])
@pytest.mark.parametrize("size", [(GW.W, GW.H), GW.RAGGED], ids=["40x24", "43x21"])
def test_filtered_var_takes_the_measured_plane(ctx, V, ML, LV, LG, worlds, size, name, source, variant):
    import torch
    ctx.set_variant(variant)
    acc, planes = _chain(ML, LG, worlds, name, source, size, GW.FIRST, GW.N)
    f = {"levels": 3, "demodulate": True, **SWEPT}
    want = OM.resolve_filtered_var(LV, acc, planes, FV.make(3, True, **SWEPT), "reinhard", 0.8)
    spatial = FV.filter(LV, acc.mean(), planes, FV.make(3, True, **SWEPT), None, "reinhard", 0.8)
    assert not np.array_equal(_bits(want[0]), _bits(spatial[0]))              # the plane is not the spatial estimate
    what = f"{name} {size} {source} variant {variant}"
    _open(ctx, worlds, name, source, size)
    assert ctx.accum_add(GW.N) == GW.N
    _same_all(ctx.accum_resolve_hdr_filtered_var(f, "reinhard", 0.8), want, what + ": against the checker chain")
    # ... and on the device: vrt_filter_hdr_var fed vrt_accum_variance_device's plane, the accumulation's mean and its guides
    w, h = size
    d_mean = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    d_var = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
    d = {"normal": torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"), "albedo": torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0"),
         "depth": torch.zeros((h, w), dtype=torch.float32, device="cuda:0"), "coverage": torch.zeros((h, w), dtype=torch.float32, device="cuda:0")}
    outs = (torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"), torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0"),
            torch.zeros((h, w), dtype=torch.float32, device="cuda:0"))
    torch.cuda.synchronize()
    ctx.accum_resolve_hdr_device(d_mean.data_ptr(), None, None)
    ctx.accum_guides_device(*(d[k].data_ptr() for k in G.KEYS))
    ctx.accum_variance_device(d_var.data_ptr())
    ctx.filter_hdr_var_device(w, h, d_mean.data_ptr(), *(d[k].data_ptr() for k in G.KEYS), d_var.data_ptr(), *(o.data_ptr() for o in outs), f,
                              "reinhard", 0.8)
    ctx.synchronize()
    torch.cuda.synchronize()
    _same_all([o.cpu().numpy() for o in outs], want, what + ": the stateless form on the device planes")
    _same_bits(d_var.cpu().numpy(), acc.variance(), what + ": the plane itself")
    # the device form on a caller's stream, and the defaults
    side = torch.cuda.Stream(device="cuda:0")
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    ctx.accum_resolve_hdr_filtered_var_device(*(o.data_ptr() for o in outs), f, "reinhard", 0.8, stream=side.cuda_stream)
    torch.cuda.synchronize()
    _same_all([o.cpu().numpy() for o in outs], want, what + ": the device form on a side stream")
    _same_all(ctx.accum_resolve_hdr_filtered_var(), OM.resolve_filtered_var(LV, acc, planes, FV.make(**V.default_filter_var())), what + ": defaults")
    # the same accumulation without moments: the spatial estimate, as before
    _open(ctx, worlds, name, source, size, moments=False)
    assert ctx.accum_add(GW.N) == GW.N
    _same_all(ctx.accum_resolve_hdr_filtered_var(f, "reinhard", 0.8), spatial, what + ": without moments")


def test_filtered_var_of_an_adaptive_accumulation(ctx, ML, LV, LG, worlds):
    name, source, size, rule = "lamp", "jitter", GW.RAGGED, (2, 6, 24)
    acc, planes = _chain(ML, LG, worlds, name, source, size, GW.FIRST, 6, rule)
    f = {"levels": 2, "demodulate": True, **SWEPT}
    _open(ctx, worlds, name, source, size, rule=rule)
    assert ctx.accum_add(6) == 6
    _same(ctx.accum_counts()[0][..., None], acc.counts()[..., None], "counts")
    assert acc.counts().min() >= 2 and acc.counts().max() > acc.counts().min()
    _same_bits(ctx.accum_variance(), acc.variance(), "the plane by each pixel's own count")
    _same_all(ctx.accum_resolve_hdr_filtered_var(f), OM.resolve_filtered_var(LV, acc, planes, FV.make(2, True, **SWEPT)), "adaptive")


def test_with_one_sample_the_spatial_estimate_runs(ctx, ML, LV, LG, worlds):
    name, source, size = "room", "jitter", (GW.W, GW.H)
    f = {"levels": 2, "demodulate": True, **SWEPT}
    acc, planes = _chain(ML, LG, worlds, name, source, size, GW.FIRST, 1)
    want = FV.filter(LV, acc.mean(), planes, FV.make(2, True, **SWEPT), None)
    _open(ctx, worlds, name, source, size)
    assert ctx.accum_add(1) == 1
    _same_all(ctx.accum_resolve_hdr_filtered_var(f), want, "one sample, moments on")
    _same_all(OM.resolve_filtered_var(LV, acc, planes, FV.make(2, True, **SWEPT)), want, "the chain says the same")
    _open(ctx, worlds, name, source, size, moments=False)
    assert ctx.accum_add(1) == 1
    _same_all(ctx.accum_resolve_hdr_filtered_var(f), want, "one sample, moments off")
    _open(ctx, worlds, name, source, size)                     # ... and from the second sample on the plane
    assert ctx.accum_add(1) == 1 and ctx.accum_add(1) == 2
    acc2, planes2 = _chain(ML, LG, worlds, name, source, size, GW.FIRST, 2)
    _same_all(ctx.accum_resolve_hdr_filtered_var(f), OM.resolve_filtered_var(LV, acc2, planes2, FV.make(2, True, **SWEPT)), "two samples")


# ---- errors and growth -------------------------------------------------------------------------------------------------------------------

def test_error_codes(V, product_scenes):
    import torch
    c = V.Context(0)
    try:
        L, h = c._L, c._h
        m, W, H, pose = SCENES["dragon"]
        out = np.zeros((H, W), np.float32)
        d_out = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        assert L.vrt_accum_keep_moments(None, 1) == -1
        for bad in (2, -1, 255):
            assert L.vrt_accum_keep_moments(h, bad) == -1
        assert L.vrt_accum_variance(None, out.ctypes.data) == -1
        assert L.vrt_accum_variance(h, out.ctypes.data) == -5                        # no begin
        assert L.vrt_accum_variance_device(h, d_out.data_ptr(), None) == -5
        tex, dim = product_scenes[m]
        c.upload_octree(tex, dim)
        ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
        c.set_camera(ip, iv, cp)
        c.accum_begin(W, H, 0, hdr=True, moments=True)
        assert L.vrt_accum_variance(h, out.ctypes.data) == -5                        # no sample yet
        assert L.vrt_accum_variance_device(h, d_out.data_ptr(), None) == -5
        assert c.accum_add(2) == 2
        assert L.vrt_accum_variance(h, None) == -1                                   # a NULL output
        assert L.vrt_accum_variance_device(h, None, None) == -1
        assert L.vrt_accum_variance(h, out.ctypes.data) == 0 and L.vrt_accum_variance_device(h, d_out.data_ptr(), None) == 0
        c.synchronize()
        assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(out))
        c.accum_begin(W, H, 0, hdr=True)
        assert c.accum_add(2) == 2
        assert L.vrt_accum_variance(h, out.ctypes.data) == -5                        # begun without moments
        assert L.vrt_accum_variance_device(h, d_out.data_ptr(), None) == -5
        c.accum_begin(W, H, 0)
        assert c.accum_add(2) == 2
        assert L.vrt_accum_variance(h, out.ctypes.data) == -5                        # begun without HDR
        assert L.vrt_accum_variance_device(h, d_out.data_ptr(), None) == -5
        for flags in (2, 4, 0x80000001):                                             # moments are no flag of the begin
            assert L.vrt_accum_begin_ex(h, W, H, 2, 0, flags) == -1
        with pytest.raises(ValueError):
            c.accum_begin(W, H, 0, moments=True)
    finally:
        c.close()


def test_buffer_growth_against_fresh_contexts(V, O, product_scenes):
    """a small frame, a larger one, the small one again on one context -- the sums, the plane's scratch and the filter's stage grow and
    are reused -- each against a context of its own"""
    m, _, _, pose = SCENES["room_outside"]
    f = {"levels": 2, "demodulate": True, **SWEPT}

    def run(c, W, H, rule):
        _setup(c, V, O, product_scenes, m, W, H, pose)
        c.accum_begin(W, H, FIRST, mode=2, jitter=True, adaptive=rule, hdr=True, moments=True)
        assert c.accum_add(3) == 3
        return (c.accum_variance(),) + c.accum_resolve_hdr_filtered_var(f) + c.accum_resolve_hdr()[:1]

    one = V.Context(0)
    try:
        for W, H, rule in ((24, 13, None), (90, 47, RULE), (24, 13, RULE), (43, 21, None)):
            got = run(one, W, H, rule)
            fresh = V.Context(0)
            try:
                want = run(fresh, W, H, rule)
            finally:
                fresh.close()
            for i, (a, b) in enumerate(zip(got, want)):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{W}x{H} {'adaptive' if rule else 'plain'}: output {i}"
    finally:
        one.close()
