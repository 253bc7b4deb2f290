"""The variance-guided filter on the MI355X (vrt_filter_hdr_var and its host and accumulation forms) against the checker
(tests/oracle_filter_var.c), bit for bit on all three outputs: tests/test_gpu_filter_hdr.py's shapes -- random planes with every kind
of bad input at a ragged frame size, every level count whose launches differ, the smallest frames, the accumulation route on both
traversal routes and ray sources, any split of the samples, the restart rule, the accumulation's own resolves untouched, a caller's
stream, the error codes, buffer growth -- with the variance plane NULL and supplied, and the two identities against vrt_filter_hdr."""
import ctypes as C

import numpy as np
import pytest

import guide_worlds as GW
import oracle_filter_hdr as F
import oracle_filter_var as FV
import oracle_guides as G
from test_filter_hdr import random_case
from test_filter_var import random_variance
from test_gpu_filter_hdr import LG, _open, _ref, _to_device, worlds  # noqa: F401  (two fixtures; the references are computed once for both files)

pytestmark = pytest.mark.gpu

W, H, FIRST, N = GW.W, GW.H, GW.FIRST, GW.N
TONEMAPS = (("clamp", 1.0), ("reinhard", 0.6))
SWEPT = dict(sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=1.0, sigma_lum=2.0)     # wide guide sigmas: the luminance term decides


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return FV.build(tmp_path_factory.mktemp("oracle_filter_var"))


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


def _f(levels, demod, **kw):
    return {"levels": levels, "demodulate": demod, **kw}


def _same_all(got, want, what):
    F.same(got[0], want[0], what + ": floats")
    F.same(got[1], want[1], what + ": bytes")
    F.same(got[2], want[2], what + ": variance")


# ---- the stateless form on random planes -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planes70():
    """test_gpu_filter_hdr's 70 x 37 planes, and a variance plane with NaN, Inf, negative, zero and huge entries"""
    rng = np.random.default_rng(70)
    rgb, g = random_case(rng, 37, 70, negative_depth=True)
    return rgb, g, random_variance(rng, 37, 70)


@pytest.mark.parametrize("tonemap,exposure", TONEMAPS)
@pytest.mark.parametrize("plane", [False, True], ids=["spatial", "plane"])
@pytest.mark.parametrize("demod", [False, True])
@pytest.mark.parametrize("levels", [0, 1, 3, 5, 8])
def test_random_planes_are_the_checkers(ctx, L, planes70, levels, demod, plane, tonemap, exposure):
    """levels 0 (the variance kernel writes the output plane), 1 (first and last level in one launch), 3 (every lattice step), 5 (the
    crossover: steps 8 and 16 gathered), 8 (taps outside the image on every side at once)"""
    rgb, g, var = planes70
    var = var if plane else None
    want = FV.filter(L, rgb, g, FV.make(levels, demod, **SWEPT), var, tonemap, exposure)
    _same_all(ctx.filter_hdr_var(rgb, g, var, _f(levels, demod, **SWEPT), tonemap, exposure), want, f"levels {levels} demod {demod} {tonemap}")
    if levels:
        assert (want[0] != F.filter(L, rgb, g, F.make(levels, demod, 0.5, 0.25, 1.0), tonemap, exposure)[0]).any()
    assert want[2].any() and np.isfinite(want[2]).all()


def test_defaults_null_filter_and_null_tonemap(ctx, V, L, planes70):
    rgb, g, var = planes70
    want = FV.filter(L, rgb, g, FV.make(**V.default_filter_var()), None, None)
    _same_all(ctx.filter_hdr_var(rgb, g, None, None, None), want, "f == NULL, tm == NULL")
    _same_all(ctx.filter_hdr_var(rgb, g, None, V.default_filter_var()), want, "the defaults spelled out")
    _same_all(ctx.filter_hdr_var(rgb, g, var), FV.filter(L, rgb, g, FV.make(**V.default_filter_var()), var), "f == NULL with a plane")


@pytest.mark.parametrize("size", [(8, 8), (9, 1), (1, 1), (1, 9), (65, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_smallest_frames(ctx, L, size):
    """borders narrower than the 7 x 7 and the 3 x 3 windows; 65 x 5: one pixel and one row past a workgroup"""
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    g = {"normal": rng.normal(size=(h, w, 3)).astype(np.float32), "albedo": rng.random((h, w, 4)).astype(np.float32),
         "depth": (10 + rng.random((h, w))).astype(np.float32), "coverage": (rng.random((h, w)) > 0.2).astype(np.float32)}
    rgb = rng.random((h, w, 3)).astype(np.float32) * 4
    var = rng.random((h, w)).astype(np.float32)
    for levels in (0, 1, 4):
        for v in (None, var):
            _same_all(ctx.filter_hdr_var(rgb, g, v, _f(levels, True, **SWEPT), "reinhard", 2.0),
                      FV.filter(L, rgb, g, FV.make(levels, True, **SWEPT), v, "reinhard", 2.0), f"{size} levels {levels} plane {v is not None}")


def _outputs(torch, h, w):
    return (torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"), torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0"),
            torch.zeros((h, w), dtype=torch.float32, device="cuda:0"))


def _check_outputs(outs, used, want, what):
    for o, u, w_, name in zip(outs, used, want, ("floats", "bytes", "variance")):
        if u:
            F.same(o.cpu().numpy(), w_, f"{what}: {name}")
        else:
            assert not o.any(), f"{what}: {name} written though NULL"


@pytest.mark.parametrize("levels", [0, 3])
def test_device_form_each_output_null_in_turn_on_a_callers_stream(ctx, L, planes70, levels):
    import torch
    rgb, g, var = planes70
    h, w = rgb.shape[:2]
    ins = _to_device(torch, rgb, g)
    d_var = torch.from_numpy(var).to("cuda:0")
    outs = _outputs(torch, h, w)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    ptrs = [t.data_ptr() for t in ins]
    for plane in (None, d_var):
        want = FV.filter(L, rgb, g, FV.make(levels, True, **SWEPT), var if plane is not None else None, "reinhard", 0.6)
        for stream in (None, side.cuda_stream):
            for used in ((1, 1, 1), (1, 0, 1), (0, 1, 1), (1, 1, 0), (0, 1, 0)):
                for o in outs:
                    o.zero_()
                torch.cuda.synchronize()
                ctx.filter_hdr_var_device(w, h, *ptrs, plane.data_ptr() if plane is not None else None,
                                          *(o.data_ptr() if u else None for o, u in zip(outs, used)), _f(levels, True, **SWEPT), "reinhard", 0.6,
                                          stream=stream)
                torch.cuda.synchronize()
                _check_outputs(outs, used, want, f"levels {levels} plane {plane is not None} stream {stream} outputs {used}")


def test_invalid_arguments(ctx, V, planes70):
    import torch
    rgb, g, var = planes70
    h, w = rgb.shape[:2]
    keep = _to_device(torch, rgb, g) + [torch.from_numpy(var).to("cuda:0")]
    ins = [t.data_ptr() for t in keep]
    out, out8, outv = _outputs(torch, h, w)
    lib, hnd = V.hip_lib(), ctx._h

    def call(ins=ins, f=None, tm=None, o=out.data_ptr(), o8=out8.data_ptr(), ov=outv.data_ptr(), size=(w, h)):
        return lib.vrt_filter_hdr_var(hnd, size[0], size[1], *ins, C.byref(f) if f else None, C.byref(tm) if tm else None, o, o8, ov, None)

    assert call() == 0
    for i in range(5):                                                       # a NULL input; an output aliasing that input
        assert call(ins=ins[:i] + [None] + ins[i + 1:]) == -1
        assert call(o=ins[i]) == -1 and call(ov=ins[i]) == -1
    assert call(ins=ins[:5] + [None]) == 0                                   # the variance plane may be NULL ...
    assert call(o=ins[5]) == -1 and call(ov=ins[5]) == -1                    # ... and is an input where it is not
    assert call(o=None, o8=None) == -1                                       # the variance alone is not an output
    assert call(o=None) == 0 and call(o8=None) == 0 and call(ov=None) == 0
    FVar = V.FilterVar
    for bad in (FVar(-1, 1, 1, 1, 1, 1), FVar(9, 1, 1, 1, 1, 1), FVar(1, 2, 1, 1, 1, 1), FVar(1, 3, 1, 1, 1, 1), FVar(1, 1, 0.0, 1, 1, 1),
                FVar(1, 1, 1, -1.0, 1, 1), FVar(1, 1, 1, 1, float("nan"), 1), FVar(1, 1, float("inf"), 1, 1, 1), FVar(1, 1, 1e-30, 1, 1, 1),
                FVar(1, 1, 1, 1, 0.0, 1), FVar(1, 1, 1, 1, 1, 0.0), FVar(1, 1, 1, 1, 1, -2.0), FVar(1, 1, 1, 1, 1, float("nan")),
                FVar(1, 1, 1, 1, 1, float("inf"))):
        assert call(f=bad) == -1, (bad.levels, bad.flags, bad.sigma_normal, bad.sigma_albedo, bad.sigma_depth, bad.sigma_lum)
    assert call(f=FVar(0, 0, 1e-15, 1e15, 1e-30, 1e-30)) == 0 and call(f=FVar(2, 1, 1, 1, 1, 1e30)) == 0
    assert call(tm=V.Tonemap(2, 1.0)) == -1 and call(tm=V.Tonemap(0, 0.0)) == -1 and call(tm=V.Tonemap(1, float("inf"))) == -1
    assert call(size=(0, h)) == -1 and call(size=(w, -1)) == -1 and call(size=(1 << 16, 1 << 15)) == -1
    host = [a.ctypes.data for a in (rgb, g["normal"], g["albedo"], g["depth"], g["coverage"], var)]
    o, o8, ov = np.zeros_like(rgb), np.zeros((h, w, 4), np.uint8), np.zeros((h, w), np.float32)
    assert lib.vrt_filter_hdr_var_host(hnd, w, h, *host, None, None, None, None, ov.ctypes.data) == -1
    assert lib.vrt_filter_hdr_var_host(hnd, w, h, *host[:4], None, host[5], None, None, o.ctypes.data, o8.ctypes.data, ov.ctypes.data) == -1
    assert lib.vrt_filter_hdr_var_host(hnd, w, h, *host[:5], None, None, None, o.ctypes.data, None, None) == 0
    # flags 2 and 3 stay invalid on vrt_filter too
    assert lib.vrt_filter_hdr(hnd, w, h, *ins[:5], C.byref(V.Filter(1, 2, 1, 1, 1)), None, out.data_ptr(), out8.data_ptr(), None) == -1
    torch.cuda.synchronize()
    del keep


def test_buffer_growth(V, L):
    """a small frame, a larger one with more levels, the small one again, levels 0 first on a context that has no scratch yet, and the
    guide-only filter between them on the same scratch; each against the checker (what a fresh context gives, by the tests above)"""
    c = V.Context(0)
    try:
        for i, (w, h, levels) in enumerate(((20, 12, 0), (20, 12, 2), (90, 41, 4), (20, 12, 3), (33, 9, 1))):
            rng = np.random.default_rng(5 + i)
            rgb, g = random_case(rng, max(h, 12), max(w, 12))
            rgb, g = rgb[:h, :w].copy(), {k: v[:h, :w].copy() for k, v in g.items()}
            var = random_variance(rng, h, w) if i % 2 else None
            _same_all(c.filter_hdr_var(rgb, g, var, _f(levels, True, **SWEPT)), FV.filter(L, rgb, g, FV.make(levels, True, **SWEPT), var), f"call {i}")
            got = c.filter_hdr(rgb, g, {"levels": 3, "demodulate": True})
            F.same(got[0], F.filter(L, rgb, g, F.make(3))[0], f"the guide-only filter after call {i}")
    finally:
        c.close()


# ---- the two identities against vrt_filter_hdr on the device -------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [0, 1, 3, 5])
def test_one_colour_is_vrt_filter_hdr(ctx, planes70, levels):
    rgb, g, var = planes70
    rgb = rgb.copy()
    rgb[F.g_of(g["coverage"]) > 0] = (0.5, 2.0, 0.125)                          # powers of two: every level returns them exactly
    guide = dict(sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=1.0)
    want = ctx.filter_hdr(rgb, g, _f(levels, False, **guide), "reinhard", 0.6)
    for v in (None, var):
        got = ctx.filter_hdr_var(rgb, g, v, _f(levels, False, **guide, sigma_lum=1.0), "reinhard", 0.6)
        F.same(got[0], want[0], f"floats, levels {levels}")
        F.same(got[1], want[1], f"bytes, levels {levels}")


@pytest.mark.parametrize("demod", [False, True])
def test_levels_0_is_vrt_filter_hdr_at_levels_0(ctx, planes70, demod):
    rgb, g, var = planes70
    want = ctx.filter_hdr(rgb, g, _f(0, demod))
    for v in (None, var):
        got = ctx.filter_hdr_var(rgb, g, v, _f(0, demod))
        F.same(got[0], want[0], "floats")
        F.same(got[1], want[1], "bytes")


# ---- the accumulation route --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("source", ["jitter", "lens"])
@pytest.mark.parametrize("name", ["room", "lamp"])
@pytest.mark.parametrize("size", [(W, H), GW.RAGGED], ids=["40x24", "43x21"])
def test_filtered_resolve_is_the_checker_on_its_own_mean_and_planes(ctx, V, L, LG, worlds, size, name, source, variant):
    import torch
    ctx.set_variant(variant)
    mean, planes = _ref(L, LG, worlds, name, source, size)
    f = _f(3, True, **SWEPT)
    want = FV.filter(L, mean, planes, FV.make(3, True, **SWEPT), None, "reinhard", 0.8)
    what = f"{name} {size} {source} variant {variant}"
    _open(ctx, worlds, name, source, size)
    assert ctx.accum_add(N) == N
    _same_all(ctx.accum_resolve_hdr_filtered_var(f, "reinhard", 0.8), want, what)
    # ... and vrt_filter_hdr_var fed with vrt_accum_resolve_hdr_device's mean and vrt_accum_guides_device's planes
    w, h = size
    d_mean = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    d = {"normal": torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"), "albedo": torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0"),
         "depth": torch.zeros((h, w), dtype=torch.float32, device="cuda:0"), "coverage": torch.zeros((h, w), dtype=torch.float32, device="cuda:0")}
    outs = _outputs(torch, h, w)
    torch.cuda.synchronize()
    ctx.accum_resolve_hdr_device(d_mean.data_ptr(), None, None)
    ctx.accum_guides_device(*(d[k].data_ptr() for k in G.KEYS))
    ctx.filter_hdr_var_device(w, h, d_mean.data_ptr(), *(d[k].data_ptr() for k in G.KEYS), None, *(o.data_ptr() for o in outs), f, "reinhard", 0.8)
    ctx.synchronize()
    torch.cuda.synchronize()
    _same_all([o.cpu().numpy() for o in outs], want, what + ": the stateless form on the device planes")
    # the defaults, f == NULL
    _same_all(ctx.accum_resolve_hdr_filtered_var(), FV.filter(L, mean, planes, FV.make(**V.default_filter_var())), what + ": defaults")


def test_3_plus_5_with_a_filtered_resolve_between_equal_8(ctx, L, LG, worlds):
    name, source = "lamp", "jitter"
    f, fo = _f(2, True, **SWEPT), FV.make(2, True, **SWEPT)
    _open(ctx, worlds, name, source)
    assert ctx.accum_add(3) == 3
    m3, p3 = _ref(L, LG, worlds, name, source, (W, H), FIRST, 3)
    _same_all(ctx.accum_resolve_hdr_filtered_var(f), FV.filter(L, m3, p3, fo), "after 3")
    assert ctx.accum_add(N - 3) == N
    m8, p8 = _ref(L, LG, worlds, name, source, (W, H))
    _same_all(ctx.accum_resolve_hdr_filtered_var(f), FV.filter(L, m8, p8, fo), "after 3 + 5")
    _open(ctx, worlds, name, source)
    assert ctx.accum_add(N) == N
    _same_all(ctx.accum_resolve_hdr_filtered_var(f), FV.filter(L, m8, p8, fo), "8 in one go")


def test_a_camera_change_is_a_state_error_where_guides_is(ctx, V, L, LG, worlds):
    import torch
    name, source = "room", "jitter"
    out8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    tex, dim, cam, _ = worlds[name, (W, H)]
    _open(ctx, worlds, name, source)
    assert ctx.accum_add(3) == 3
    m3, p3 = _ref(L, LG, worlds, name, source, (W, H), FIRST, 3)
    fo = FV.make(**V.default_filter_var())
    want = FV.filter(L, m3, p3, fo)
    _same_all(ctx.accum_resolve_hdr_filtered_var(), want, "before the move")
    pose = GW.FRAMES[name][0]
    moved = V.camera_block((pose[0] + 1.25, pose[1], pose[2] - 0.5), pose[3] + 4.0, pose[4], W, H)[:3]
    ctx.set_camera(*moved)
    _same_all(ctx.accum_resolve_hdr_filtered_var(), want, "moved, nothing added: the state is up to date")
    ctx.set_camera(*cam)
    assert ctx.accum_add(1) == 4                                            # same inputs again: no restart, one guide sample missing
    ctx.set_camera(*moved)
    with pytest.raises(V.VrtError, match="vrt error -5"):
        ctx.accum_guides()
    with pytest.raises(V.VrtError, match="vrt error -5"):
        ctx.accum_resolve_hdr_filtered_var()
    with pytest.raises(V.VrtError, match="vrt error -5"):
        ctx.accum_resolve_hdr_filtered_var_device(None, out8.data_ptr(), None)
    ctx.synchronize()
    assert not out8.any()
    ctx.set_camera(*cam)
    m4, p4 = _ref(L, LG, worlds, name, source, (W, H), FIRST, 4)
    _same_all(ctx.accum_resolve_hdr_filtered_var(), FV.filter(L, m4, p4, fo), "back again")


def test_the_accumulations_own_resolves_do_not_change(ctx, worlds):
    name, source = "lamp", "jitter"

    def run(filtered):
        _open(ctx, worlds, name, source)
        ctx.accum_add(3)
        if filtered:
            ctx.accum_resolve_hdr_filtered_var(_f(3, True))
        mid = ctx.accum_resolve() + ctx.accum_resolve_hdr() + tuple(ctx.accum_guides()[k] for k in G.KEYS) + ctx.accum_resolve_hdr_filtered(_f(2, True))
        if filtered:
            ctx.accum_resolve_hdr_filtered_var(_f(5, False))
        ctx.accum_add(N - 3)
        if filtered:
            ctx.accum_resolve_hdr_filtered_var()
        return mid + ctx.accum_resolve() + ctx.accum_resolve_hdr() + tuple(ctx.accum_guides()[k] for k in G.KEYS)

    plain, with_filter = run(False), run(True)
    assert len(plain) == len(with_filter) == 22
    for a, b in zip(plain, with_filter):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_the_device_form_runs_on_a_callers_stream(ctx, V, L, LG, worlds):
    import torch
    name, source = "room", "lens"
    _open(ctx, worlds, name, source)
    assert ctx.accum_add(N) == N
    mean, planes = _ref(L, LG, worlds, name, source, (W, H))
    f = _f(4, True, **SWEPT)
    want = FV.filter(L, mean, planes, FV.make(4, True, **SWEPT))
    outs = _outputs(torch, H, W)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    for stream in (None, side.cuda_stream, None):
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        ctx.accum_resolve_hdr_filtered_var_device(*(o.data_ptr() for o in outs), f, stream=stream)
        torch.cuda.synchronize()
        _same_all([o.cpu().numpy() for o in outs], want, f"stream {stream}")
        _same_all(ctx.accum_resolve_hdr_filtered_var(f), want, "host form")
    for used in ((1, 0, 1), (0, 1, 0), (1, 1, 0)):
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        ctx.accum_resolve_hdr_filtered_var_device(*(o.data_ptr() if u else None for o, u in zip(outs, used)), f, stream=side.cuda_stream)
        torch.cuda.synchronize()
        _check_outputs(outs, used, want, f"outputs {used}")
    with pytest.raises(V.VrtError, match="vrt error -1"):
        ctx.accum_resolve_hdr_filtered_var_device(None, None, outs[2].data_ptr(), f)


def test_state_errors(V, worlds):
    import torch
    out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    c = V.Context(0)
    try:
        tex, dim, cam, _ = worlds["room", (W, H)]
        c.upload_octree(tex, dim)
        c.set_camera(*cam)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # no begin
            c.accum_resolve_hdr_filtered_var()
        c.accum_begin(W, H, FIRST, hdr=True)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # no sample
            c.accum_resolve_hdr_filtered_var()
        c.accum_begin(W, H, FIRST)
        c.accum_add(1)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # without HDR
            c.accum_resolve_hdr_filtered_var()
        with pytest.raises(V.VrtError, match="vrt error -5"):
            c.accum_resolve_hdr_filtered_var_device(out.data_ptr(), None, None)
    finally:
        c.close()
