"""Guided upsampling on the MI355X (vrt_guide_frame, vrt_upsample_hdr, vrt_accum_resolve_hdr_upsampled and their host and device
forms) against the checkers (tests/oracle_upsample.c, tests/oracle_guides.c), bit for bit on every output: random planes with every
kind of bad input at ragged sizes and every factor, the smallest frames, each optional output NULL in turn on a caller's stream, the
error codes, buffer growth, the r = 1 identity against vrt_filter_hdr on the device, the guide planes of a frame against the begin /
add(1) / guides sequence and in the middle of an accumulation, the accumulation route on both traversal routes and ray sources, the
accumulation's own resolves untouched, the restart rule, the state errors, and no profiling slot taken."""
import ctypes as C

import numpy as np
import pytest

import guide_worlds as GW
import oracle_filter_hdr as F
import oracle_guides as G
import oracle_hdr
import oracle_upsample as U
from test_upsample import random_planes

pytestmark = pytest.mark.gpu

FIRST = GW.FIRST
N = 2                       # samples of the accumulation route
MODE_FULL = 2
SETS = {"default": {}, "wide": dict(sigma_normal=2.0, sigma_albedo=0.5, sigma_depth=8.0, min_weight=0.25),
        "jittered": dict(sigma_normal=0.5, sigma_albedo=0.1, sigma_depth=1.0, offset_lo=(0.5, 0.5), offset_hi=(0.25, 1.0))}
NAMES = ("out_rgb", "out_rgba8", "out_unresolved")


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return U.build(tmp_path_factory.mktemp("oracle_upsample"))


@pytest.fixture(scope="module")
def LG(tmp_path_factory):
    return G.build(tmp_path_factory.mktemp("oracle_guides"))


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
    ctx.set_guide_glass(0)


def _same_all(got, want, what, names=NAMES):
    assert len(got) == len(want) == len(names)
    for g, w, n in zip(got, want, names):
        F.same(g, w, f"{what}: {n}")


def _case(seed, h, w, r, bad=0.05):
    """random low and high planes that show related surfaces (so that taps count) with bad entries in every plane of both sizes"""
    rng = np.random.default_rng(seed)
    rgb, g = random_planes(rng, h, w)
    hi = {k: np.ascontiguousarray(np.repeat(np.repeat(v, r, axis=0), r, axis=1)) for k, v in g.items()}
    hi["albedo"] = np.clip(hi["albedo"] + (rng.random(hi["albedo"].shape).astype(np.float32) - 0.5) * 0.1, 0, 1).astype(np.float32)
    hi["depth"] = (hi["depth"] * (1 + 0.02 * rng.random(hi["depth"].shape))).astype(np.float32)
    y, x = int(rng.integers(0, h * r)), int(rng.integers(0, w * r))
    hi["coverage"][y:y + 5, x:x + 7] = 0.0                    # a dead block of the high planes' own
    vals = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0, 0.0, 1e30, 7e4], np.float32)
    for a in (rgb, *g.values(), *hi.values()):
        m = rng.random(a.shape) < bad
        a[m] = vals[rng.integers(0, len(vals), int(m.sum()))]
    return rgb, g, hi


def _run_host(ctx, L, rgb, g, hi, u, what, op="clamp", exposure=1.0):
    want = U.upsample(L, rgb, g, hi, u, op, exposure)
    _same_all(ctx.upsample_hdr(rgb, g, hi, U.keys(u), op, exposure), want, what)
    return want


# ---- the stateless form on random planes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("kw", list(SETS), ids=list(SETS))
@pytest.mark.parametrize("size", [(35, 19, 2), (35, 19, 3), (35, 19, 4), (70, 37, 1)], ids=lambda s: f"{s[0]}x{s[1]}r{s[2]}")
def test_random_planes_are_the_checkers(ctx, L, size, kw, demodulate):
    w, h, r = size
    rgb, g, hi = _case(w * 10 + r, h, w, r)
    u = U.make(r, demodulate, **SETS[kw])
    for op, exposure in (("clamp", 1.0), ("reinhard", 0.6)):
        want = _run_host(ctx, L, rgb, g, hi, u, f"{size} {kw} {op}", op, exposure)
    assert np.isfinite(want[0]).all() and (want[0] >= 0).all()
    assert 0.02 < want[2].mean() < 0.9 or r == 1, "pixels of both kinds"


@pytest.mark.parametrize("size", [(1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 1, 4), (9, 1, 3), (1, 9, 3), (4, 4, 2), (3, 3, 3), (33, 3, 2)],
                         ids=lambda s: f"{s[0]}x{s[1]}r{s[2]}")
def test_smallest_frames(ctx, L, size):
    """one low pixel at every factor; a row and a column; one tile; 9 x 9 high pixels off the tile grid; 66 high pixels across a
    workgroup's seam"""
    w, h, r = size
    rgb, g, hi = _case(w * 100 + h * 10 + r, h, w, r, bad=0.0)
    for kw in ("default", "jittered"):
        _run_host(ctx, L, rgb, g, hi, U.make(r, True, **SETS[kw]), f"{size} {kw}")


# ---- the device form ---------------------------------------------------------------------------------------------------------------
def _to_device(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]


def _outputs(torch, h, w):
    return (torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"), torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0"),
            torch.zeros((h, w), dtype=torch.uint8, device="cuda:0"))


def _check_outputs(outs, used, want, what, names=NAMES):
    for o, u, w_, name in zip(outs, used, want, names):
        if u:
            F.same(o.cpu().numpy(), w_, f"{what}: {name}")
        else:
            assert not o.any(), f"{what}: {name} written though NULL"


def _planes_in(rgb, g, hi):
    return [rgb] + [g[k] for k in G.KEYS] + [hi[k] for k in G.KEYS]


@pytest.fixture(scope="module")
def case35():
    return _case(352, 19, 35, 2)


def test_device_form_each_output_null_in_turn_on_a_callers_stream(ctx, L, case35):
    import torch
    rgb, g, hi = case35
    u = U.make(2, True, **SETS["wide"])
    want = U.upsample(L, rgb, g, hi, u, "reinhard", 0.8)
    ins = _to_device(torch, *_planes_in(rgb, g, hi))
    outs = _outputs(torch, 38, 70)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    for stream in (None, side.cuda_stream):
        for used in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0)):
            for o in outs:
                o.zero_()
            torch.cuda.synchronize()
            ctx.upsample_hdr_device(35, 19, *(i.data_ptr() for i in ins), *(o.data_ptr() if k else None for o, k in zip(outs, used)),
                                    U.keys(u), "reinhard", 0.8, stream=stream)
            torch.cuda.synchronize()
            _check_outputs(outs, used, want, f"stream {stream} outputs {used}")
    # u == NULL is vrt_upsample_default, tm == NULL the clamp at exposure 1
    ctx.upsample_hdr_device(35, 19, *(i.data_ptr() for i in ins), *(o.data_ptr() for o in outs), None, None)
    torch.cuda.synchronize()
    _check_outputs(outs, (1, 1, 1), U.upsample(L, rgb, g, hi, U.make(), None), "defaults")


def test_invalid_arguments(ctx, V, case35):
    import torch
    rgb, g, hi = case35
    w, h = 35, 19
    keep = _to_device(torch, *_planes_in(rgb, g, hi))
    ins = [t.data_ptr() for t in keep]
    out, out8, mask = _outputs(torch, 4 * h, 4 * w)           # room for every factor
    lib, hnd = V.hip_lib(), ctx._h

    def with_(**kw):
        u = V.Upsample()
        lib.vrt_upsample_default(C.byref(u))
        for k, v in kw.items():
            setattr(u, k, v)
        return u

    def call(ins=ins, u=with_(), tm=None, o=out.data_ptr(), o8=out8.data_ptr(), om=mask.data_ptr(), size=(w, h)):
        return lib.vrt_upsample_hdr(hnd, size[0], size[1], *ins, C.byref(u) if u else None, C.byref(tm) if tm else None, o, o8, om, None)

    assert call() == 0 and call(u=None) == 0
    for i in range(9):                                                       # a NULL input; an output aliasing that input
        assert call(ins=ins[:i] + [None] + ins[i + 1:]) == -1
        assert call(o=ins[i]) == -1 and call(o8=ins[i]) == -1 and call(om=ins[i]) == -1
    assert call(o=None) == 0 and call(o8=None) == 0 and call(om=None) == 0 and call(o=None, om=None) == 0
    assert call(o=None, o8=None) == -1                                       # both colour outputs
    assert call(o8=out.data_ptr()) == -1 and call(om=out8.data_ptr()) == -1 and call(om=out.data_ptr()) == -1   # two outputs in one place
    for bad in (dict(factor=0), dict(factor=5), dict(factor=-1), dict(flags=2), dict(flags=3), dict(sigma_normal=0.0), dict(sigma_albedo=-1.0),
                dict(sigma_depth=float("inf")), dict(sigma_depth=float("nan")), dict(sigma_normal=1e-30), dict(sigma_albedo=1e-25),
                dict(min_weight=-0.1), dict(min_weight=1.0), dict(min_weight=float("nan")), dict(offset_lo_x=-0.1), dict(offset_lo_y=1.1),
                dict(offset_hi_x=float("nan")), dict(offset_hi_y=2.0)):
        assert call(u=with_(**bad)) == -1, bad
    # the extremes that pass, at sizes the buffers hold: 17 x 9 at factor 4 reads 68 x 36 high pixels of the 70 x 38 there are
    assert call(u=with_(factor=4, flags=0, min_weight=0.999, offset_lo_x=1.0, offset_hi_y=1.0, sigma_depth=1e30), size=(17, 9)) == 0
    assert call(u=with_(factor=1)) == 0
    assert call(tm=V.Tonemap(2, 1.0)) == -1 and call(tm=V.Tonemap(1, 0.0)) == -1 and call(tm=V.Tonemap(1, 2.0)) == 0
    assert call(size=(0, h)) == -1 and call(size=(w, -1)) == -1 and call(size=(1 << 16, 1 << 15)) == -1
    assert lib.vrt_upsample_hdr(None, w, h, *ins, None, None, out.data_ptr(), None, None, None) == -1
    host = [a.ctypes.data for a in _planes_in(rgb, g, hi)]
    o, o8, om = np.zeros((2 * h, 2 * w, 3), np.float32), np.zeros((2 * h, 2 * w, 4), np.uint8), np.zeros((2 * h, 2 * w), np.uint8)
    assert lib.vrt_upsample_hdr_host(hnd, w, h, *host, None, None, o.ctypes.data, None, None) == 0
    assert lib.vrt_upsample_hdr_host(hnd, w, h, *host, None, None, None, None, om.ctypes.data) == -1
    assert lib.vrt_upsample_hdr_host(hnd, w, h, *host[:5], None, *host[6:], None, None, o.ctypes.data, o8.ctypes.data, om.ctypes.data) == -1
    assert lib.vrt_upsample_hdr_host(hnd, w, h, *host, C.byref(with_(factor=7)), None, o.ctypes.data, None, None) == -1
    torch.cuda.synchronize()
    del keep


def test_buffer_growth(V, L):
    """a small frame, a large one, the small one again on a context that has no staging yet; each against the checker"""
    c = V.Context(0)
    try:
        for i, (w, h, r) in enumerate(((10, 6, 2), (45, 21, 4), (10, 6, 2), (33, 9, 3))):
            rgb, g, hi = _case(50 + i, h, w, r)
            _run_host(c, L, rgb, g, hi, U.make(r, True, **SETS["wide"]), f"call {i}")
    finally:
        c.close()


@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
def test_factor_one_is_vrt_filter_hdr_at_levels_zero_on_the_device(ctx, demodulate):
    import torch
    rgb, g, _ = _case(701, 37, 70, 1)
    ins = _to_device(torch, rgb, *(g[k] for k in G.KEYS))
    a, b = _outputs(torch, 37, 70), _outputs(torch, 37, 70)
    torch.cuda.synchronize()
    ptr = [i.data_ptr() for i in ins]
    ctx.filter_hdr_device(70, 37, *ptr, a[0].data_ptr(), a[1].data_ptr(), {"levels": 0, "demodulate": demodulate}, "reinhard", 1.5)
    ctx.upsample_hdr_device(70, 37, *ptr, *ptr[1:], b[0].data_ptr(), b[1].data_ptr(), None,
                            {"factor": 1, "demodulate": demodulate, "offset_lo_x": 0.5, "offset_lo_y": 0.5, "offset_hi_x": 0.5, "offset_hi_y": 0.5},
                            "reinhard", 1.5)
    ctx.synchronize()
    torch.cuda.synchronize()
    _same_all([t.cpu().numpy() for t in b[:2]], [t.cpu().numpy() for t in a[:2]], "r = 1", NAMES[:2])


# ---- the guide planes of a frame ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worlds(V, O):
    """name -> (tex, dim); and (name, size) -> (cam, the checker's scene)"""
    out = {}
    for name in ("room", "lamp"):
        w = GW.world(V, name)
        out[name] = w.flatten()
        w.close()
        for size in ((40, 24), (43, 21), (80, 48), (86, 42), (129, 63)):
            cam = GW.camera(V, name, size)
            out[name, size] = (cam, O.make_scene(*out[name], *cam))
    return out


def _load(c, worlds, name, size):
    c.upload_octree(*worlds[name])
    c.set_params(c.default_params())
    c.set_camera(*worlds[name, size][0])
    c.set_lens(0.0, 1.0)


@pytest.fixture(scope="module")
def other(V):
    """a second context: the begin / add(1) / guides sequence the planes are defined by"""
    c = V.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("glass", [0, 1], ids=["plain", "glass"])
@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("name", ["room", "lamp"])
def test_guide_frame_is_the_begin_add_guides_sequence(ctx, other, V, LG, worlds, name, variant, glass):
    import torch
    for size in ((40, 24), (43, 21), (86, 42)):
        w, h = size
        for c in (ctx, other):
            _load(c, worlds, name, size)
            c.set_variant(variant)
            c.set_guide_glass(glass)
        other.accum_begin(w, h, 0, mode=V.MODE_PRIMARY)
        assert other.accum_add(1) == 1
        want = other.accum_guides()
        G.same(ctx.guide_frame(w, h), want, f"{name} {size} variant {variant} glass {glass}")
        if not glass:
            G.same(want, G.planes(LG, worlds[name, size][1], w, h, 0, 1)[0], "the sequence is the checker's one corner sample")
        d = {k: torch.zeros(want[k].shape, dtype=torch.float32, device="cuda:0") for k in G.KEYS}
        side = torch.cuda.Stream(device="cuda:0")
        torch.cuda.synchronize()
        for stream, used in ((side.cuda_stream, (1, 1, 1, 1)), (None, (0, 1, 0, 1)), (side.cuda_stream, (1, 0, 1, 0))):
            for t in d.values():
                t.zero_()
            torch.cuda.synchronize()
            ctx.guide_frame_device(w, h, *(d[k].data_ptr() if u else None for k, u in zip(G.KEYS, used)), stream=stream)
            torch.cuda.synchronize()
            for k, u in zip(G.KEYS, used):
                if u:
                    F.same(d[k].cpu().numpy(), want[k], f"device {k}")
                else:
                    assert not d[k].any()
    assert (want["coverage"] > 0).mean() > 0.5


def test_guide_frame_in_the_middle_of_an_accumulation_leaves_it_alone(ctx, V, worlds):
    """3 + 5 samples of a jittered HDR accumulation that keeps moments at 43 x 21 with frames of other sizes marched in between,
    against the uninterrupted 8"""
    def run(interrupt):
        _load(ctx, worlds, "lamp", (43, 21))
        ctx.accum_begin(43, 21, FIRST, mode=MODE_FULL, jitter=True, hdr=True, moments=True)
        ctx.accum_add(3)
        mid = ()
        if interrupt:
            ctx.guide_frame(86, 42)
            mid = tuple(ctx.accum_guides()[k] for k in G.KEYS)           # the guide state of 3 samples, made between two frames
            ctx.guide_frame(40, 24)
        ctx.accum_add(5)
        if interrupt:
            ctx.guide_frame(129, 63)
        out = ctx.accum_resolve() + ctx.accum_resolve_hdr() + tuple(ctx.accum_guides()[k] for k in G.KEYS) + (ctx.accum_variance(),)
        return mid, out

    (_, plain), (mid, cut) = run(False), run(True)
    assert len(plain) == len(cut) == 11 and len(mid) == 4
    for a, b in zip(plain, cut):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    ctx.accum_begin(43, 21, 0, adaptive=(2, 6, 3))
    ctx.accum_add(4)
    counts = ctx.accum_counts()
    ctx.guide_frame(86, 42)
    again = ctx.accum_counts()
    assert np.array_equal(counts[0], again[0]) and counts[1] == again[1]


def test_guide_frame_errors_and_no_profiling_slot(V, worlds):
    c = V.Context(0)
    try:
        with pytest.raises(V.VrtError, match="vrt error -5"):               # no upload
            c.guide_frame(40, 24)
        c.upload_octree(*worlds["room"])
        with pytest.raises(V.VrtError, match="vrt error -5"):               # no camera
            c.guide_frame(40, 24)
        c.set_camera(*worlds["room", (40, 24)][0])
        n = np.zeros((24, 40, 3), np.float32)
        lib = V.hip_lib()
        assert lib.vrt_guide_frame(c._h, 40, 24, None, None, None, None) == -1
        assert lib.vrt_guide_frame_device(c._h, 40, 24, None, None, None, None, None) == -1
        assert lib.vrt_guide_frame(c._h, 0, 24, n.ctypes.data, None, None, None) == -1
        assert lib.vrt_guide_frame(c._h, 1 << 16, 1 << 15, n.ctypes.data, None, None, None) == -1
        assert lib.vrt_guide_frame(None, 40, 24, n.ctypes.data, None, None, None) == -1
        assert lib.vrt_guide_frame(c._h, 40, 24, n.ctypes.data, None, None, None) == 0 and n.any()
        c.set_profiling(16)
        c.guide_frame(40, 24)
        assert len(c.profile_read()) == 0
        c.dispatch(40, 24)
        assert len(c.profile_read()) == 1                                   # ... while a frame takes one
    finally:
        c.close()


# ---- the accumulation route --------------------------------------------------------------------------------------------------------
_refs = {}


def _ref(L, LG, worlds, name, jitter, size, r):
    """the checker's mean and planes of the N low samples and its planes of the one high corner sample, computed once"""
    key = (name, jitter, size, r)
    if key not in _refs:
        w, h = size
        scene = worlds[name, size][1]
        acc = oracle_hdr.Accum(L, h, w)
        for k in range(FIRST, FIRST + N):
            acc.add(oracle_hdr.render(L, scene, w, h, MODE_FULL, k, jitter))
        _refs[key] = (acc.mean(), G.planes(LG, scene, w, h, FIRST, N, jitter)[0], G.planes(LG, worlds[name, (r * w, r * h)][1], r * w, r * h, 0, 1)[0])
    return _refs[key]


def _open(ctx, worlds, name, jitter, size):
    _load(ctx, worlds, name, size)
    ctx.accum_begin(size[0], size[1], FIRST, mode=MODE_FULL, jitter=jitter, hdr=True)
    assert ctx.accum_add(N) == N


@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("jitter", [False, True], ids=["corner", "jitter"])
@pytest.mark.parametrize("name", ["room", "lamp"])
@pytest.mark.parametrize("size", [(40, 24, 2), (43, 21, 2), (43, 21, 3)], ids=lambda s: f"{s[0]}x{s[1]}r{s[2]}")
def test_the_accumulation_route_is_the_checker_chain(ctx, V, L, LG, worlds, size, name, jitter, variant):
    import torch
    w, h, r = size
    ctx.set_variant(variant)
    _open(ctx, worlds, name, jitter, (w, h))
    mean, lo, hi = _ref(L, LG, worlds, name, jitter, (w, h), r)
    kw = dict(sigma_normal=1.0, sigma_albedo=0.25, sigma_depth=4.0, min_weight=0.1)
    off = (0.5, 0.5) if jitter else (0.0, 0.0)
    want = U.upsample(L, mean, lo, hi, U.make(r, True, offset_lo=off, **kw), "reinhard", 0.8)
    what = f"{name} {size} jitter {jitter} variant {variant}"
    before = ctx.accum_resolve() + ctx.accum_resolve_hdr()
    # the offsets are the call's own: what the caller passes is replaced
    given = dict(U.keys(U.make(r, True, **kw)), offset_lo_x=0.25, offset_hi_y=1.0)
    _same_all(ctx.accum_resolve_hdr_upsampled(given, "reinhard", 0.8), want, what)
    assert 0 < want[2].mean() < 0.5 or name == "lamp"
    # ... and vrt_upsample_hdr fed with the device's own resolves and vrt_guide_frame_device
    f32 = dict(dtype=torch.float32, device="cuda:0")
    d_mean = torch.zeros((h, w, 3), **f32)
    d = [torch.zeros(s, **f32) for s in ((h, w, 3), (h, w, 4), (h, w), (h, w))]
    dh = [torch.zeros(s, **f32) for s in ((r * h, r * w, 3), (r * h, r * w, 4), (r * h, r * w), (r * h, r * w))]
    outs, outs2 = _outputs(torch, r * h, r * w), _outputs(torch, r * h, r * w)
    side = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    ctx.accum_resolve_hdr_device(d_mean.data_ptr(), None, None)
    ctx.accum_guides_device(*(t.data_ptr() for t in d))
    ctx.guide_frame_device(r * w, r * h, *(t.data_ptr() for t in dh))
    ctx.upsample_hdr_device(w, h, d_mean.data_ptr(), *(t.data_ptr() for t in d), *(t.data_ptr() for t in dh), *(o.data_ptr() for o in outs),
                            U.keys(U.make(r, True, offset_lo=off, **kw)), "reinhard", 0.8)
    ctx.accum_resolve_hdr_upsampled_device(*(o.data_ptr() for o in outs2), given, "reinhard", 0.8, stream=side.cuda_stream)
    ctx.synchronize()
    torch.cuda.synchronize()
    _same_all([o.cpu().numpy() for o in outs], want, what + ": the stateless forms on the device planes")
    _same_all([o.cpu().numpy() for o in outs2], want, what + ": the device form on a caller's stream")
    for a, b in zip(before, ctx.accum_resolve() + ctx.accum_resolve_hdr()):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the accumulation's resolves are unchanged"


def test_the_accumulation_route_defaults_outputs_and_the_guide_glass_rule(ctx, V, L, LG, worlds):
    import torch
    w, h = 40, 24
    ctx.set_guide_glass(1)
    _open(ctx, worlds, "lamp", False, (w, h))                     # begun past glass ...
    ctx.set_guide_glass(0)                                        # ... and resolved with the rule off: both sides take it AS BEGUN
    lo, hi = ctx.accum_guides(), None
    ctx.set_guide_glass(1)
    hi = ctx.guide_frame(2 * w, 2 * h)
    ctx.set_guide_glass(0)
    mean = ctx.accum_resolve_hdr()[0]
    want = U.upsample(L, mean, lo, hi, U.make(), None)
    _same_all(ctx.accum_resolve_hdr_upsampled(None, None), want, "u == NULL, tm == NULL, glass as begun")
    outs = _outputs(torch, 2 * h, 2 * w)
    for used in ((1, 0, 0), (0, 1, 1), (1, 1, 0)):
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        ctx.accum_resolve_hdr_upsampled_device(*(o.data_ptr() if k else None for o, k in zip(outs, used)), None, None)
        ctx.synchronize()
        torch.cuda.synchronize()
        _check_outputs(outs, used, want, f"outputs {used}")
    with pytest.raises(V.VrtError, match="vrt error -1"):
        ctx.accum_resolve_hdr_upsampled_device(None, None, outs[2].data_ptr())
    lib = V.hip_lib()
    o = np.zeros((2 * h, 2 * w, 3), np.float32)
    for bad_u, bad_tm in ((V.Upsample(5, 1, 1, 1, 1, 0, 0, 0, 0, 0), None), (V.Upsample(2, 1, 1, 1, 0, 0, 0, 0, 0, 0), None), (None, V.Tonemap(2, 1.0))):
        assert lib.vrt_accum_resolve_hdr_upsampled(ctx._h, C.byref(bad_u) if bad_u else None, C.byref(bad_tm) if bad_tm else None,
                                                   o.ctypes.data, None, None) == -1


def test_state_errors_the_restart_rule_and_no_profiling_slot(V, L, LG, worlds):
    c = V.Context(0)
    try:
        w, h = 40, 24
        _load(c, worlds, "room", (w, h))
        with pytest.raises(V.VrtError, match="vrt error -5"):               # no begin
            c.accum_resolve_hdr_upsampled()
        c.accum_begin(w, h, FIRST, hdr=True)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # no sample
            c.accum_resolve_hdr_upsampled()
        c.accum_begin(w, h, FIRST)
        c.accum_add(1)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # without HDR
            c.accum_resolve_hdr_upsampled()
        c.accum_begin(w, h, FIRST, mode=MODE_FULL, hdr=True)
        c.accum_add(N)
        c.set_profiling(16)
        got = c.accum_resolve_hdr_upsampled()
        _same_all(got, U.upsample(L, *_ref(L, LG, worlds, "room", False, (w, h), 2), U.make(), None), "before the camera moves")
        assert len(c.profile_read()) == 0
        cam = worlds["room", (w, h)][0]
        moved = V.camera_block((cam[2][0] + 1.25, cam[2][1], cam[2][2] - 0.5), 40.0, -8.0, w, h)[:3]
        c.set_camera(*moved)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # the high planes would show another view
            c.accum_resolve_hdr_upsampled()
        c.set_camera(*cam)
        _same_all(c.accum_resolve_hdr_upsampled(), got, "the camera back where the samples were taken")
        c.set_camera(*moved)
        assert c.accum_add(1) == 1                                          # the restart rule: the sums start again ...
        again = c.accum_resolve_hdr_upsampled()                             # ... and both sides show the new view
        assert not np.array_equal(again[0], got[0])
        hi = c.guide_frame(2 * w, 2 * h)
        _same_all(again, U.upsample(L, c.accum_resolve_hdr()[0], c.accum_guides(), hi, U.make(), None), "after the restart")
    finally:
        c.close()
