"""The guided filter on the MI355X (vrt_filter_hdr and its host and accumulation forms) against the checker
(tests/oracle_filter_hdr.c), bit for bit on both outputs: random planes with every kind of bad input at a ragged frame size, every
level count whose launches differ, the smallest frames, the accumulation route on both traversal routes and ray sources, any split
of the samples, the restart rule, the accumulation's own resolves untouched, a caller's stream, the error codes, buffer growth, and
an image-shaped ray batch filtered with vrt_guide_rays' planes."""
import ctypes as C

import numpy as np
import pytest

import guide_worlds as GW
import oracle_filter_hdr as F
import oracle_guides as G
import oracle_hdr
from test_filter_hdr import random_case

pytestmark = pytest.mark.gpu

W, H, FIRST, N = GW.W, GW.H, GW.FIRST, GW.N
MODE_FULL = 2
TONEMAPS = (("clamp", 1.0), ("reinhard", 0.6))
SWEPT = dict(sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=1.0)     # wider than the defaults: more taps carry weight


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return F.build(tmp_path_factory.mktemp("oracle_filter_hdr"))


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


def _f(levels, demod, **kw):
    return {"levels": levels, "demodulate": demod, **kw}


def _same_both(got, want, what):
    F.same(got[0], want[0], what + ": floats")
    F.same(got[1], want[1], what + ": bytes")


# ---- the stateless form on random planes -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planes70():
    """70 x 37: the lattice levels' 32 x 8 tile gives three tiles across (the last 6 wide) and five down at step 1, 2 x 3 per residue
    class at step 2 and 1 x 2 at step 4, every class with class 0's count; the gather levels' 64 x 4 workgroups two across with a
    ragged right edge, ten down with a ragged last one. Frames that cross the lattice tiles' seams at steps 2 and 4:
    tests/test_gpu_filter_seams.py. NaN, Inf, negative values (depth included), dead pixels singly, a dead block and a live pixel alone
    inside it"""
    return random_case(np.random.default_rng(70), 37, 70, negative_depth=True)


@pytest.mark.parametrize("tonemap,exposure", TONEMAPS)
@pytest.mark.parametrize("demod", [False, True])
@pytest.mark.parametrize("levels", [0, 1, 3, 5])
def test_random_planes_are_the_checkers(ctx, L, planes70, levels, demod, tonemap, exposure):
    """levels 0 (no prepass), 1 (first and last level in one launch), 3 (first, middle, last: both level images), 5 (step 16: taps
    outside the image on every side at once)"""
    rgb, g = planes70
    want = F.filter(L, rgb, g, F.make(levels, demod, **SWEPT), tonemap, exposure)
    _same_both(ctx.filter_hdr(rgb, g, _f(levels, demod, **SWEPT), tonemap, exposure), want, f"levels {levels} demod {demod} {tonemap}")
    assert levels == 0 or (want[0] != F.h_of(rgb)).any()


def test_defaults_null_filter_and_null_tonemap(ctx, V, L, planes70):
    rgb, g = planes70
    want = F.filter(L, rgb, g, F.make(**V.default_filter()), None)
    _same_both(ctx.filter_hdr(rgb, g, None, None), want, "f == NULL, tm == NULL")
    _same_both(ctx.filter_hdr(rgb, g, V.default_filter()), want, "the defaults spelled out")
    _same_both(ctx.filter_hdr(rgb, g, _f(V.FILTER_MAX_LEVELS, True)), F.filter(L, rgb, g, F.make(V.FILTER_MAX_LEVELS)), "8 levels")


@pytest.mark.parametrize("size", [(8, 8), (9, 1), (1, 1), (1, 9), (65, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_smallest_frames(ctx, L, size):
    """vrt_denoise takes any frame of at least one pixel; 65 x 5: one pixel and one row past a workgroup"""
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    g = {"normal": rng.normal(size=(h, w, 3)).astype(np.float32), "albedo": rng.random((h, w, 4)).astype(np.float32),
         "depth": (10 + rng.random((h, w))).astype(np.float32), "coverage": (rng.random((h, w)) > 0.2).astype(np.float32)}
    rgb = rng.random((h, w, 3)).astype(np.float32) * 4
    for levels in (0, 1, 4):
        _same_both(ctx.filter_hdr(rgb, g, _f(levels, True, **SWEPT), "reinhard", 2.0),
                   F.filter(L, rgb, g, F.make(levels, True, **SWEPT), "reinhard", 2.0), f"{size} levels {levels}")


def _to_device(torch, rgb, g):
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (rgb, g["normal"], g["albedo"], g["depth"], g["coverage"])]


def test_device_form_each_output_null_in_turn_on_a_callers_stream(ctx, L, planes70):
    import torch
    rgb, g = planes70
    h, w = rgb.shape[:2]
    ins = _to_device(torch, rgb, g)
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    out8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    want = F.filter(L, rgb, g, F.make(3, True, **SWEPT), "reinhard", 0.6)
    ptrs = [t.data_ptr() for t in ins]
    for stream in (None, side.cuda_stream):
        for o_rgb, o_rgba in ((out, out8), (out, None), (None, out8)):
            out.zero_()
            out8.zero_()
            torch.cuda.synchronize()
            ctx.filter_hdr_device(w, h, *ptrs, o_rgb.data_ptr() if o_rgb is not None else None,
                                  o_rgba.data_ptr() if o_rgba is not None else None, _f(3, True, **SWEPT), "reinhard", 0.6, stream=stream)
            torch.cuda.synchronize()
            if o_rgb is not None:
                F.same(out.cpu().numpy(), want[0], f"floats, stream {stream}")
            else:
                assert not out.any()
            if o_rgba is not None:
                F.same(out8.cpu().numpy(), want[1], f"bytes, stream {stream}")
            else:
                assert not out8.any()


def test_invalid_arguments(ctx, V, planes70):
    import torch
    rgb, g = planes70
    h, w = rgb.shape[:2]
    keep = _to_device(torch, rgb, g)
    ins = [t.data_ptr() for t in keep]
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    out8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    lib, hnd = V.hip_lib(), ctx._h

    def call(ins=ins, f=None, tm=None, o=out.data_ptr(), o8=out8.data_ptr(), size=(w, h)):
        return lib.vrt_filter_hdr(hnd, size[0], size[1], *ins, C.byref(f) if f else None, C.byref(tm) if tm else None, o, o8, None)

    assert call() == 0
    for i in range(5):                                                       # a NULL input; d_out_rgb aliasing that input
        assert call(ins=ins[:i] + [None] + ins[i + 1:]) == -1
        assert call(o=ins[i]) == -1
    assert call(o=None, o8=None) == -1
    assert call(o=None) == 0 and call(o8=None) == 0
    for bad in (V.Filter(-1, 1, 1, 1, 1), V.Filter(9, 1, 1, 1, 1), V.Filter(1, 2, 1, 1, 1), V.Filter(1, 3, 1, 1, 1),
                V.Filter(1, 1, 0.0, 1, 1), V.Filter(1, 1, 1, -1.0, 1), V.Filter(1, 1, 1, 1, float("nan")), V.Filter(1, 1, float("inf"), 1, 1),
                V.Filter(1, 1, 1e-30, 1, 1), V.Filter(1, 1, 1, 1, 0.0)):
        assert call(f=bad) == -1, (bad.levels, bad.flags, bad.sigma_normal, bad.sigma_albedo, bad.sigma_depth)
    assert call(f=V.Filter(0, 0, 1e-15, 1e15, 1e-30)) == 0                   # small, large, and a tiny sigma_depth are all taken
    assert call(tm=V.Tonemap(2, 1.0)) == -1 and call(tm=V.Tonemap(0, 0.0)) == -1 and call(tm=V.Tonemap(1, float("inf"))) == -1
    assert call(size=(0, h)) == -1 and call(size=(w, -1)) == -1 and call(size=(1 << 16, 1 << 15)) == -1
    host = [a.ctypes.data for a in (rgb, g["normal"], g["albedo"], g["depth"], g["coverage"])]
    o, o8 = np.zeros_like(rgb), np.zeros((h, w, 4), np.uint8)
    assert lib.vrt_filter_hdr_host(hnd, w, h, *host, None, None, None, None) == -1
    assert lib.vrt_filter_hdr_host(hnd, w, h, *host[:4], None, None, None, o.ctypes.data, o8.ctypes.data) == -1
    assert lib.vrt_filter_hdr_host(hnd, w, h, *host, None, None, o.ctypes.data, None) == 0
    torch.cuda.synchronize()
    del keep


def test_buffer_growth(V, L):
    """a small frame, a larger one with more levels, the small one again on one context; each against the checker (what a fresh
    context gives, by the tests above)"""
    c = V.Context(0)
    try:
        for i, (w, h, levels) in enumerate(((20, 12, 2), (90, 41, 4), (20, 12, 3), (33, 9, 1))):
            rgb, g = random_case(np.random.default_rng(5 + i), max(h, 12), max(w, 12))
            rgb, g = rgb[:h, :w].copy(), {k: v[:h, :w].copy() for k, v in g.items()}
            _same_both(c.filter_hdr(rgb, g, _f(levels, True, **SWEPT)), F.filter(L, rgb, g, F.make(levels, True, **SWEPT)), f"call {i}")
    finally:
        c.close()


# ---- the accumulation route --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worlds(V, O):
    out = {}
    for name in ("room", "lamp"):
        w = GW.world(V, name)
        tex, dim = w.flatten()
        w.close()
        for size in ((W, H), GW.RAGGED):
            cam = GW.camera(V, name, size)
            out[name, size] = (tex, dim, cam, O.make_scene(tex, dim, *cam))
    return out


_refs = {}


def _ref(L, LG, worlds, name, source, size, first=FIRST, n=N):
    """the checker's mean and planes of samples first .. first + n - 1, computed once"""
    key = (name, source, size, first, n)
    if key not in _refs:
        jitter, _ = GW.SOURCES[source]
        lens = GW.lens_of(name, source)
        scene = worlds[name, size][3]
        acc = oracle_hdr.Accum(L, size[1], size[0])
        for k in range(first, first + n):
            acc.add(oracle_hdr.render(L, scene, size[0], size[1], MODE_FULL, k, jitter, *lens))
        _refs[key] = (acc.mean(), G.planes(LG, scene, size[0], size[1], first, n, jitter, *lens)[0])
    return _refs[key]


def _open(ctx, worlds, name, source, size=(W, H), hdr=True, first=FIRST):
    tex, dim, cam, _ = worlds[name, size]
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    ctx.set_camera(*cam)
    ctx.set_lens(*GW.lens_of(name, source))
    ctx.accum_begin(size[0], size[1], first, mode=MODE_FULL, jitter=GW.SOURCES[source][0], hdr=hdr)


@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("source", ["jitter", "lens"])
@pytest.mark.parametrize("name", ["room", "lamp"])
@pytest.mark.parametrize("size", [(W, H), GW.RAGGED], ids=["40x24", "43x21"])
def test_filtered_resolve_is_the_checker_on_its_own_mean_and_planes(ctx, L, LG, worlds, size, name, source, variant):
    import torch
    ctx.set_variant(variant)
    mean, planes = _ref(L, LG, worlds, name, source, size)
    f = _f(3, True, **SWEPT)
    want = F.filter(L, mean, planes, F.make(3, True, **SWEPT), "reinhard", 0.8)
    what = f"{name} {size} {source} variant {variant}"
    _open(ctx, worlds, name, source, size)
    assert ctx.accum_add(N) == N
    _same_both(ctx.accum_resolve_hdr_filtered(f, "reinhard", 0.8), want, what)
    # ... and vrt_filter_hdr fed with vrt_accum_resolve_hdr_device's mean and vrt_accum_guides_device's planes
    w, h = size
    d_mean = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    d = {"normal": torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"), "albedo": torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0"),
         "depth": torch.zeros((h, w), dtype=torch.float32, device="cuda:0"), "coverage": torch.zeros((h, w), dtype=torch.float32, device="cuda:0")}
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    out8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.accum_resolve_hdr_device(d_mean.data_ptr(), None, None)
    ctx.accum_guides_device(*(d[k].data_ptr() for k in G.KEYS))
    ctx.filter_hdr_device(w, h, d_mean.data_ptr(), *(d[k].data_ptr() for k in G.KEYS), out.data_ptr(), out8.data_ptr(), f, "reinhard", 0.8)
    ctx.synchronize()
    torch.cuda.synchronize()
    F.same(d_mean.cpu().numpy(), mean, what + ": the mean")
    _same_both((out.cpu().numpy(), out8.cpu().numpy()), want, what + ": the stateless form on the device planes")
    # the defaults, f == NULL
    _same_both(ctx.accum_resolve_hdr_filtered(), F.filter(L, mean, planes, F.make(1)), what + ": defaults")


def test_3_plus_5_with_a_filtered_resolve_between_equal_8(ctx, L, LG, worlds):
    name, source = "lamp", "jitter"
    f = _f(2, True, **SWEPT)
    _open(ctx, worlds, name, source)
    assert ctx.accum_add(3) == 3
    m3, p3 = _ref(L, LG, worlds, name, source, (W, H), FIRST, 3)
    _same_both(ctx.accum_resolve_hdr_filtered(f), F.filter(L, m3, p3, F.make(2, True, **SWEPT)), "after 3")
    assert ctx.accum_add(N - 3) == N
    m8, p8 = _ref(L, LG, worlds, name, source, (W, H))
    _same_both(ctx.accum_resolve_hdr_filtered(f), F.filter(L, m8, p8, F.make(2, True, **SWEPT)), "after 3 + 5")
    _open(ctx, worlds, name, source)
    assert ctx.accum_add(N) == N
    _same_both(ctx.accum_resolve_hdr_filtered(f), F.filter(L, m8, p8, F.make(2, True, **SWEPT)), "8 in one go")


def test_a_camera_change_is_a_state_error_where_guides_is(ctx, V, L, LG, worlds):
    import torch
    name, source = "room", "jitter"
    out8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    tex, dim, cam, _ = worlds[name, (W, H)]
    _open(ctx, worlds, name, source)
    assert ctx.accum_add(3) == 3
    m3, p3 = _ref(L, LG, worlds, name, source, (W, H), FIRST, 3)
    want = F.filter(L, m3, p3, F.make(1))
    _same_both(ctx.accum_resolve_hdr_filtered(), want, "before the move")
    pose = GW.FRAMES[name][0]
    moved = V.camera_block((pose[0] + 1.25, pose[1], pose[2] - 0.5), pose[3] + 4.0, pose[4], W, H)[:3]
    ctx.set_camera(*moved)
    _same_both(ctx.accum_resolve_hdr_filtered(), want, "moved, nothing added: the state is up to date")
    ctx.set_camera(*cam)
    assert ctx.accum_add(1) == 4                                            # same inputs again: no restart, one guide sample missing
    ctx.set_camera(*moved)
    with pytest.raises(V.VrtError, match="vrt error -5"):
        ctx.accum_guides()
    with pytest.raises(V.VrtError, match="vrt error -5"):
        ctx.accum_resolve_hdr_filtered()
    with pytest.raises(V.VrtError, match="vrt error -5"):
        ctx.accum_resolve_hdr_filtered_device(None, out8.data_ptr())
    ctx.synchronize()
    assert not out8.any()
    ctx.set_camera(*cam)
    m4, p4 = _ref(L, LG, worlds, name, source, (W, H), FIRST, 4)
    _same_both(ctx.accum_resolve_hdr_filtered(), F.filter(L, m4, p4, F.make(1)), "back again")


def test_the_accumulations_own_resolves_do_not_change(ctx, worlds):
    name, source = "lamp", "jitter"

    def run(filtered):
        _open(ctx, worlds, name, source)
        ctx.accum_add(3)
        if filtered:
            ctx.accum_resolve_hdr_filtered(_f(3, True))
        mid = ctx.accum_resolve() + ctx.accum_resolve_hdr() + tuple(ctx.accum_guides()[k] for k in G.KEYS)
        if filtered:
            ctx.accum_resolve_hdr_filtered(_f(5, False))
        ctx.accum_add(N - 3)
        if filtered:
            ctx.accum_resolve_hdr_filtered()
        return mid + ctx.accum_resolve() + ctx.accum_resolve_hdr() + tuple(ctx.accum_guides()[k] for k in G.KEYS)

    plain, with_filter = run(False), run(True)
    assert len(plain) == len(with_filter) == 20
    for a, b in zip(plain, with_filter):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_the_device_form_runs_on_a_callers_stream(ctx, V, L, LG, worlds):
    import torch
    name, source = "room", "lens"
    _open(ctx, worlds, name, source)
    assert ctx.accum_add(N) == N
    mean, planes = _ref(L, LG, worlds, name, source, (W, H))
    f = _f(4, True, **SWEPT)
    want = F.filter(L, mean, planes, F.make(4, True, **SWEPT))
    out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    out8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    for stream in (None, side.cuda_stream, None):
        out.zero_()
        out8.zero_()
        torch.cuda.synchronize()
        ctx.accum_resolve_hdr_filtered_device(out.data_ptr(), out8.data_ptr(), f, stream=stream)
        torch.cuda.synchronize()
        _same_both((out.cpu().numpy(), out8.cpu().numpy()), want, f"stream {stream}")
        _same_both(ctx.accum_resolve_hdr_filtered(f), want, "host form")
    out.zero_()
    torch.cuda.synchronize()
    ctx.accum_resolve_hdr_filtered_device(out.data_ptr(), None, f, stream=side.cuda_stream)
    torch.cuda.synchronize()
    F.same(out.cpu().numpy(), want[0], "floats alone")
    with pytest.raises(V.VrtError, match="vrt error -1"):
        ctx.accum_resolve_hdr_filtered_device(None, None, f)


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
            c.accum_resolve_hdr_filtered()
        c.accum_begin(W, H, FIRST, hdr=True)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # no sample
            c.accum_resolve_hdr_filtered()
        c.accum_begin(W, H, FIRST)
        c.accum_add(1)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # without HDR
            c.accum_resolve_hdr_filtered()
        with pytest.raises(V.VrtError, match="vrt error -5"):
            c.accum_resolve_hdr_filtered_device(out.data_ptr(), None)
    finally:
        c.close()


# ---- an image-shaped ray batch -----------------------------------------------------------------------------------------------------
def test_a_ray_batch_filtered_with_guide_rays_planes(ctx, L, worlds):
    """vrt_shade_rays_hdr's colours and vrt_guide_rays' planes of a 24 x 13 batch, its hit bytes as the coverage plane"""
    tex, dim, cam, _ = worlds["lamp", (W, H)]
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    o, d = GW.picking_rays(n=24 * 13)
    rgb = ctx.shade_rays_hdr(o, d, width=24, n_samples=2)[0].reshape(13, 24, 3)
    r = ctx.guide_rays(o, d, width=24)
    g = {"normal": r["normal"].reshape(13, 24, 3), "albedo": r["albedo"].reshape(13, 24, 4), "depth": r["depth"].reshape(13, 24),
         "coverage": r["hit"].astype(np.float32).reshape(13, 24)}
    assert g["coverage"].sum() > 200
    _same_both(ctx.filter_hdr(rgb, g, _f(2, True, **SWEPT)), F.filter(L, rgb, g, F.make(2, True, **SWEPT)), "ray batch")
