"""The temporal pass with measured variances and a 3 x 3 search on the MI355X (vrt_temporal_hdr_mom, its host form and the
accumulation forms) against the checker (tests/oracle_temporal_mom.c), bit for bit on every output: test_gpu_temporal.py's shapes --
random planes on a real camera block with every kind of bad input in the planes, the history and the variance plane at a ragged
frame size, over search x measured_below x the parameter sets; an input built so that the search matters; the smallest frames, a first
frame, reprojections that leave the previous image, each optional pointer NULL in turn on a caller's stream, the error codes, buffer
growth, the identity with vrt_temporal_hdr on the device, and the accumulation route over three poses with the history ping-ponged,
begun with and without moments, with the accumulation's own resolves untouched and no profiling slot taken."""
import ctypes as C

import numpy as np
import pytest

import guide_worlds as GW
import oracle_filter_hdr as F
import oracle_filter_var as FV
import oracle_guides as G
import oracle_hdr
import oracle_moments as OM
import oracle_temporal as T
import oracle_temporal_mom as M
import temporal_worlds as TW
from test_temporal import random_history, random_planes, sphere
from test_temporal_mom import bad_variance, case70 as make_case70, mom_of, search_case

pytestmark = pytest.mark.gpu

W, H, FIRST = GW.W, GW.H, GW.FIRST
N = 2                       # samples per pose: M3 is not "unknown"
MODE_FULL = 2
SWEPT = dict(sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=1.0, sigma_lum=2.0)
LOOSE = dict(depth_tol=0.5, normal_min=-1.0)
NAMES = ("history", "integrated", "filtered floats", "bytes", "variance")


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return M.build(tmp_path_factory.mktemp("oracle_temporal_mom"))


@pytest.fixture(scope="module")
def LG(tmp_path_factory):
    return G.build(tmp_path_factory.mktemp("oracle_guides"))


@pytest.fixture(scope="module")
def LOM(tmp_path_factory):
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


def _keys(m):
    """a TemporalMom's parameters as the dict Context.temporal_hdr_mom takes"""
    return {k: getattr(m, k) for k in ("offset_x", "offset_y", "max_history", "alpha_min", "alpha_moments_min", "normal_min", "depth_tol",
                                       "measured_below", "search")}


def _same_all(got, want, what, names=("history", "integrated", "variance")):
    assert len(got) == len(want) == len(names)
    for g, w, n in zip(got, want, names):
        F.same(g, w, f"{what}: {n}")


def _run_host(ctx, L, cam, rgb, g, var, hist, cam_prev, what, below=4, search=1, **kw):
    """the host form against the checker -> the new history"""
    m = mom_of(cam_prev if hist is not None else None, below, search, **kw)
    want = M.temporal(L, cam, rgb, g, var, hist, m)
    got = ctx.temporal_hdr_mom(cam, rgb, g, var, hist, TW.prev_camera(cam_prev) if hist is not None else None, _keys(m))
    _same_all(got, want, what)
    return want[0]


# ---- the stateless form on random planes -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case70(V):
    return make_case70(V)


@pytest.mark.parametrize("kw", [LOOSE, {}, dict(LOOSE, offset=(0.5, 0.5), max_history=7, alpha_min=0.3, alpha_moments_min=0.05)],
                         ids=["loose", "defaults", "jittered"])
@pytest.mark.parametrize("below", [1, 2, 4, M.ALWAYS])
@pytest.mark.parametrize("search", [0, 1])
def test_random_planes_are_the_checkers(ctx, L, case70, search, below, kw):
    cam, cam_prev, rgb, g, hist, var = case70
    m = mom_of(cam_prev, below, search, **kw)
    want = M.temporal(L, cam, rgb, g, var, hist, m, details=True)
    _same_all(ctx.temporal_hdr_mom(cam, rgb, g, var, hist, TW.prev_camera(cam_prev), _keys(m)), want[:3], f"{search} {below} {kw}")
    if kw:
        assert want[3][..., 3:7].any(axis=2).mean() > 0.3 and (want[0][0, ..., 3] > 1).mean() > 0.3
    if search:
        assert (want[3][..., 9] > 0).sum() > 20, "the search finds histories on these planes"
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and np.isfinite(want[2]).all()
    _run_host(ctx, L, cam_prev, rgb[::-1].copy(), g, var[::-1].copy(), want[0], cam, "the next frame, on the pass's own history", below, search, **kw)


def test_an_input_built_so_that_the_search_matters(ctx, V, L):
    cam, prev, rgb, g, var, hist = search_case(V, size=(70, 37))
    kw = dict(max_history=64, alpha_min=0.0, alpha_moments_min=0.0, normal_min=0.9, depth_tol=0.05)
    m = mom_of(prev, 4, 1, **kw)
    want = M.temporal(L, cam, rgb, g, var, hist, m, details=True)
    det = want[3]
    ran = det[..., 8] != 0
    xc, yc = np.floor(det[..., 0] + np.float32(0.5)).astype(int), np.floor(det[..., 1] + np.float32(0.5)).astype(int)
    assert (ran & (det[..., 9] > 0)).sum() >= 20, "pixels that ran the search and found a history"
    assert (ran & (det[..., 9] == 0)).sum() >= 1, "... and found none"
    assert (ran & ((xc == 0) | (xc == 69) | (yc == 0) | (yc == 36))).sum() >= 1, "... with the centre on an image border"
    _same_all(ctx.temporal_hdr_mom(cam, rgb, g, var, hist, TW.prev_camera(prev), _keys(m)), want[:3], "search")
    off = mom_of(prev, 4, 0, **kw)
    _same_all(ctx.temporal_hdr_mom(cam, rgb, g, var, hist, TW.prev_camera(prev), _keys(off)), M.temporal(L, cam, rgb, g, var, hist, off), "no search")


def test_a_first_frame_reads_no_previous_camera(ctx, V, L, case70):
    cam, _, rgb, g, _, var = case70
    m = mom_of(None, 4, 1)
    want = M.temporal(L, cam, rgb, g, var, None, m)
    _same_all(ctx.temporal_hdr_mom(cam, rgb, g, var, temporal=_keys(m)), want, "history_in == NULL")
    nan = (np.full(16, np.nan, np.float32), np.full(4, np.nan, np.float32))
    t = V.Context._temporal_mom(_keys(m), nan)
    out_h, out, outv = np.zeros_like(want[0]), np.zeros_like(want[1]), np.zeros_like(want[2])
    ptr = [a.ctypes.data for a in (*cam, rgb, g["normal"], g["depth"], g["coverage"], var)]
    assert V.hip_lib().vrt_temporal_hdr_mom_host(ctx._h, 70, 37, *ptr, None, C.byref(t), out_h.ctypes.data, out.ctypes.data, outv.ctypes.data) == 0
    _same_all((out_h, out, outv), want, "a previous camera of NaN, never read")
    live = F.g_of(g["coverage"]) > 0
    F.same(want[0][2, ..., 3], np.where(live, FV.hv_of(var), np.float32(0)), "V' = hv(v)")
    F.same(want[2], want[0][2, ..., 3], "N' = 1 < 4: the measured variance goes out")


@pytest.mark.parametrize("size", [(8, 8), (9, 1), (1, 1), (1, 9), (65, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_smallest_frames_with_the_search_on(ctx, V, L, size):
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    poses = TW.poses("lamp")
    cams = [TW.camera(V, p, size) for p in poses]
    hist = None
    for k in range(3):
        rgb, g = random_planes(rng, h, w, dead=w * h > 9)
        g["depth"][:] = 20
        hist = _run_host(ctx, L, cams[k], rgb, g, bad_variance(rng, h, w), hist, cams[k - 1], f"{size} frame {k}", **LOOSE)
        if k == 1 and w * h > 1:
            hist[1, ..., 3].flat[::2] = 0                     # every other pixel of the history dead: the next frame has to search
    assert (hist[0, ..., 3] >= 2).any() or w * h == 1


@pytest.mark.parametrize("dyaw,dpitch", [(12.0, 0.0), (-12.0, 0.0), (0.0, 9.0), (0.0, -9.0), (180.0, 0.0)],
                         ids=["left", "right", "top", "bottom", "behind"])
def test_a_reprojection_that_leaves_the_image(ctx, V, L, dyaw, dpitch):
    pose = TW.poses("room")[0]
    size = (43, 21)
    cam = TW.camera(V, pose, size)
    prev = TW.camera(V, (pose[0], pose[1], pose[2], pose[3] + dyaw, pose[4] + dpitch), size)
    centre = np.asarray(pose[:3], np.float32)
    rng = np.random.default_rng(5)
    rgb = (rng.random((21, 43, 3)) * 4).astype(np.float32)
    var = (rng.random((21, 43)) * 2).astype(np.float32)
    h1 = _run_host(ctx, L, prev, rgb, sphere(prev, centre, 20.0, *size), var, None, None, "previous")
    h1[1, ::3, ::2, 3] = 0                                    # dead pixels in the history: the search runs up to the window's edge
    h2 = _run_host(ctx, L, cam, rgb[:, ::-1].copy(), sphere(cam, centre, 20.0, *size), var, h1, prev, "current")
    n = h2[0, ..., 3]
    assert (n == 1).sum() > 43 and ((n == 2).sum() > 43 or dyaw == 180.0)


# ---- the device form ---------------------------------------------------------------------------------------------------------------
def _to_device(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]


def _outputs(torch, h, w):
    return (torch.zeros((3, h, w, 4), dtype=torch.float32, device="cuda:0"), torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"),
            torch.zeros((h, w), dtype=torch.float32, device="cuda:0"))


def _check_outputs(outs, used, want, what, names=("history", "integrated", "variance")):
    for o, u, w_, name in zip(outs, used, want, names):
        if u:
            F.same(o.cpu().numpy(), w_, f"{what}: {name}")
        else:
            assert not o.any(), f"{what}: {name} written though NULL"


def test_device_form_each_optional_pointer_null_in_turn_on_a_callers_stream(ctx, L, case70):
    import torch
    cam, cam_prev, rgb, g, hist, var = case70
    ins = _to_device(torch, rgb, g["normal"], g["depth"], g["coverage"])
    d_var, d_hist = _to_device(torch, var, hist)
    outs = _outputs(torch, 37, 70)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    for history in (None, d_hist):
        m = mom_of(cam_prev if history is not None else None, 4, 1, **LOOSE)
        for variance in (d_var, None):
            want = M.temporal(L, cam, rgb, g, var if variance is not None else None, hist if history is not None else None, m)
            for stream in (None, side.cuda_stream):
                for used in ((1, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0)):
                    for o in outs:
                        o.zero_()
                    torch.cuda.synchronize()
                    ctx.temporal_hdr_mom_device(70, 37, cam, *(i.data_ptr() for i in ins), variance.data_ptr() if variance is not None else None,
                                                history.data_ptr() if history is not None else None,
                                                *(o.data_ptr() if u else None for o, u in zip(outs, used)), TW.prev_camera(cam_prev), _keys(m),
                                                stream=stream)
                    torch.cuda.synchronize()
                    _check_outputs(outs, used, want, f"history {history is not None} variance {variance is not None} stream {stream} outputs {used}")


def test_identity_with_vrt_temporal_hdr_on_the_device(ctx, L, case70):
    cam, cam_prev, rgb, g, hist, var = case70
    for kw in (LOOSE, {}):
        m = mom_of(cam_prev, 1, 0, **kw)
        old = ctx.temporal_hdr(cam, rgb, g, hist, TW.prev_camera(cam_prev), {k: v for k, v in _keys(m).items() if k not in ("measured_below", "search")})
        for v in (var, None):
            new = ctx.temporal_hdr_mom(cam, rgb, g, v, hist, TW.prev_camera(cam_prev), _keys(m))
            F.same(new[1], old[1], "integrated")
            F.same(new[2], old[2], "variance")
            F.same(new[0][:2], old[0][:2], "history planes 0 and 1")
            F.same(new[0][2, ..., :3], old[0][2, ..., :3], "the history's normal")
        assert not old[0][2, ..., 3].any() and new[0][2, ..., 3].any()


def test_invalid_arguments(ctx, V, case70):
    import torch
    cam, cam_prev, rgb, g, hist, var = case70
    w, h = 70, 37
    keep = _to_device(torch, rgb, g["normal"], g["depth"], g["coverage"], var, hist)
    ins = [t.data_ptr() for t in keep]
    out_h, out, outv = _outputs(torch, h, w)
    lib, hnd = V.hip_lib(), ctx._h
    cam_ptr = [a.ctypes.data for a in cam]
    good = V.Context._temporal_mom(None, TW.prev_camera(cam_prev))

    def call(cam=cam_ptr, ins=ins, t=good, oh=out_h.data_ptr(), o=out.data_ptr(), ov=outv.data_ptr(), size=(w, h)):
        return lib.vrt_temporal_hdr_mom(hnd, size[0], size[1], *cam, *ins, C.byref(t) if t else None, oh, o, ov, None)

    def with_(**kw):
        t = V.Context._temporal_mom(None, TW.prev_camera(cam_prev))
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    assert call() == 0
    for i in range(4):                                                       # a NULL input; an output aliasing that input
        assert call(ins=ins[:i] + [None] + ins[i + 1:]) == -1
        assert call(oh=ins[i]) == -1 and call(o=ins[i]) == -1 and call(ov=ins[i]) == -1
    assert call(ins=ins[:4] + [None, ins[5]]) == 0 and call(ins=ins[:5] + [None]) == 0      # the variance and the history may be NULL ...
    for i in (4, 5):                                                         # ... and are inputs where they are not
        assert call(oh=ins[i]) == -1 and call(o=ins[i]) == -1 and call(ov=ins[i]) == -1
    assert call(oh=None) == -1 and call(t=None) == -1
    assert call(o=None) == 0 and call(ov=None) == 0 and call(o=None, ov=None) == 0
    assert call(o=out_h.data_ptr()) == -1 and call(ov=out.data_ptr()) == -1
    assert call(oh=out_h.data_ptr() + 4) == -1 and call(ins=ins[:5] + [ins[5] + 8]) == -1
    for i in range(3):
        assert call(cam=cam_ptr[:i] + [None] + cam_ptr[i + 1:]) == -1
    for bad in (dict(measured_below=0), dict(measured_below=-1), dict(measured_below=32770), dict(search=2), dict(search=-1),
                dict(max_history=0), dict(max_history=32769), dict(alpha_min=1.5), dict(alpha_moments_min=float("nan")), dict(normal_min=-1.5),
                dict(depth_tol=0.0), dict(offset_x=-0.1), dict(offset_y=float("nan"))):
        assert call(t=with_(**bad)) == -1, bad
    for fine in (dict(measured_below=1), dict(measured_below=32769, max_history=32768), dict(search=1), dict(search=0)):
        assert call(t=with_(**fine)) == 0, fine
    nan_prev = with_()
    nan_prev.prev_view_proj[5] = float("inf")
    assert call(t=nan_prev) == -1 and call(ins=ins[:5] + [None], t=nan_prev) == 0
    assert call(size=(0, h)) == -1 and call(size=(w, -1)) == -1 and call(size=(1 << 16, 1 << 15)) == -1
    host = [a.ctypes.data for a in (rgb, g["normal"], g["depth"], g["coverage"], var, hist)]
    oh, o, ov = np.zeros((3, h, w, 4), np.float32), np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
    assert lib.vrt_temporal_hdr_mom_host(hnd, w, h, *cam_ptr, *host, C.byref(good), oh.ctypes.data, None, None) == 0
    assert lib.vrt_temporal_hdr_mom_host(hnd, w, h, *cam_ptr, *host[:4], None, host[5], C.byref(good), oh.ctypes.data, None, None) == 0
    assert lib.vrt_temporal_hdr_mom_host(hnd, w, h, *cam_ptr, *host, C.byref(good), None, o.ctypes.data, ov.ctypes.data) == -1
    assert lib.vrt_temporal_hdr_mom_host(hnd, w, h, *cam_ptr, *host, C.byref(good), host[5], o.ctypes.data, ov.ctypes.data) == -1
    assert lib.vrt_temporal_hdr_mom_host(hnd, w, h, *cam_ptr, *host, C.byref(with_(search=3)), oh.ctypes.data, None, None) == -1
    assert lib.vrt_temporal_hdr_mom_host(hnd, w, h, *cam_ptr, *host, None, oh.ctypes.data, None, None) == -1
    with pytest.raises(V.VrtError, match="vrt error -1"):
        ctx.temporal_hdr_mom(cam, rgb, g, var, temporal={"measured_below": 40000})
    torch.cuda.synchronize()
    del keep


def test_buffer_growth(V, L):
    """a small frame, a large one, the small one again on a context that has no staging yet; each against the checker"""
    c = V.Context(0)
    try:
        poses = TW.poses("room")
        for i, (w, h) in enumerate(((20, 12), (90, 41), (20, 12), (33, 9))):
            rng = np.random.default_rng(5 + i)
            rgb, g = random_planes(rng, h, w)
            cam, cam_prev = TW.camera(V, poses[1], (w, h)), TW.camera(V, poses[0], (w, h))
            hist = random_history(rng, h, w) if i else None
            _run_host(c, L, cam, rgb, g, bad_variance(rng, h, w) if i != 2 else None, hist, cam_prev, f"call {i}", **LOOSE)
    finally:
        c.close()


# ---- the accumulation route --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worlds(V, O):
    """(name, size, pose index) -> (tex, dim, cam, the checker's scene)"""
    out = {}
    for name in ("room", "lamp"):
        w = GW.world(V, name)
        tex, dim = w.flatten()
        w.close()
        for size in ((W, H), GW.RAGGED):
            for i, pose in enumerate(TW.poses(name)):
                cam = TW.camera(V, pose, size)
                out[name, size, i] = (tex, dim, cam, O.make_scene(tex, dim, *cam))
    return out


_refs = {}


def _ref(LOM, LG, worlds, name, jitter, size, i):
    """the checker's mean, planes and M3 plane of the N samples of pose i, computed once"""
    key = (name, jitter, size, i)
    if key not in _refs:
        scene = worlds[name, size, i][3]
        acc = OM.Accum(LOM, size[1], size[0])
        for k in range(FIRST, FIRST + N):
            acc.add(oracle_hdr.render(LOM, scene, size[0], size[1], MODE_FULL, k, jitter))
        _refs[key] = (acc.mean(), G.planes(LG, scene, size[0], size[1], FIRST, N, jitter)[0], acc.variance())
    return _refs[key]


def _open(ctx, worlds, name, jitter, size, i, moments, upload=True):
    tex, dim, cam, _ = worlds[name, size, i]
    if upload:
        ctx.upload_octree(tex, dim)
        ctx.set_params(ctx.default_params())
    ctx.set_camera(*cam)
    ctx.set_lens(0.0, 1.0)
    ctx.accum_begin(size[0], size[1], FIRST, mode=MODE_FULL, jitter=jitter, hdr=True, moments=moments)
    assert ctx.accum_add(N) == N
    return cam


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "plain"])
@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("jitter", [False, True], ids=["corner", "jitter"])
@pytest.mark.parametrize("name", ["room", "lamp"])
@pytest.mark.parametrize("size", [(W, H), GW.RAGGED], ids=["40x24", "43x21"])
def test_three_poses_with_the_history_ping_ponged_are_the_checker_chain(ctx, V, L, LOM, LG, worlds, size, name, jitter, variant, moments):
    import torch
    ctx.set_variant(variant)
    w, h = size
    f, fo = {"levels": 3, "demodulate": True, **SWEPT}, FV.make(3, True, **SWEPT)
    kw = dict(alpha_min=0.2, alpha_moments_min=0.1, max_history=8, normal_min=0.9, depth_tol=0.05)
    extra = dict(measured_below=4, search=1)
    zeros = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda:0")   # noqa: E731
    d_mean, d_mvar = zeros(h, w, 3), zeros(h, w)
    d = {"normal": zeros(h, w, 3), "albedo": zeros(h, w, 4), "depth": zeros(h, w), "coverage": zeros(h, w)}
    d_hist = [zeros(3, h, w, 4) for _ in range(2)]
    d_int, d_var = zeros(h, w, 3), zeros(h, w)
    d_out = (zeros(h, w, 3), zeros(h, w, 4, dtype=torch.uint8), zeros(h, w))
    torch.cuda.synchronize()
    hist, cam_prev, grown = None, None, 0
    for i in (0, 1, 2):
        what = f"{name} {size} jitter {jitter} variant {variant} moments {moments} pose {i}"
        cam = _open(ctx, worlds, name, jitter, size, i, moments, upload=cam_prev is None)
        mean, planes, mvar = _ref(LOM, LG, worlds, name, jitter, size, i)
        m = mom_of(cam_prev, offset=(0.5, 0.5) if jitter else (0.0, 0.0), **extra, **kw)
        want = M.chain(L, cam, mean, planes, mvar if moments else None, hist, m, fo, "reinhard", 0.8)
        prev = TW.prev_camera(cam_prev) if hist is not None else None
        before = (ctx.accum_resolve_hdr(), ctx.accum_resolve(), ctx.accum_variance() if moments else ())
        # the offsets are the call's own: what the caller passes is replaced
        got = ctx.accum_resolve_hdr_temporal_mom(hist, prev, dict(kw, offset_x=0.25, offset_y=1.0, **extra), f, "reinhard", 0.8)
        _same_all(got, want, what, NAMES)
        # ... and vrt_temporal_hdr_mom plus vrt_filter_hdr_var fed with the device resolves and vrt_accum_variance_device
        ctx.accum_resolve_hdr_device(d_mean.data_ptr(), None, None)
        ctx.accum_guides_device(*(d[k].data_ptr() for k in G.KEYS))
        if moments:
            ctx.accum_variance_device(d_mvar.data_ptr())
        src, dst = d_hist[grown % 2], d_hist[(grown + 1) % 2]
        ctx.temporal_hdr_mom_device(w, h, cam, d_mean.data_ptr(), d["normal"].data_ptr(), d["depth"].data_ptr(), d["coverage"].data_ptr(),
                                    d_mvar.data_ptr() if moments else None, src.data_ptr() if hist is not None else None, dst.data_ptr(),
                                    d_int.data_ptr(), d_var.data_ptr(), prev, _keys(m))
        ctx.filter_hdr_var_device(w, h, d_int.data_ptr(), *(d[k].data_ptr() for k in G.KEYS), d_var.data_ptr(), *(o.data_ptr() for o in d_out),
                                  f, "reinhard", 0.8)
        ctx.synchronize()
        torch.cuda.synchronize()
        _same_all([dst.cpu().numpy(), d_int.cpu().numpy()] + [o.cpu().numpy() for o in d_out], want, what + ": the stateless forms on the device planes", NAMES)
        # ... and the device form of the chain, into the other history
        outs = (src, d_int, *d_out)
        for o in outs:
            o.zero_()
        d_in = _to_device(torch, hist)[0] if hist is not None else None
        ctx.accum_resolve_hdr_temporal_mom_device(d_in.data_ptr() if d_in is not None else None, *(o.data_ptr() for o in outs), prev,
                                                  dict(kw, **extra), f, "reinhard", 0.8)
        ctx.synchronize()
        torch.cuda.synchronize()
        _same_all([o.cpu().numpy() for o in outs], want, what + ": the device form", NAMES)
        after = (ctx.accum_resolve_hdr(), ctx.accum_resolve(), ctx.accum_variance() if moments else ())
        for a, b in zip(before, after):
            for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
                assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), what + ": the accumulation's own resolves"
        hist, cam_prev, grown = want[0], cam, grown + 1
    live = F.g_of(planes["coverage"]) > 0
    assert (hist[0, ..., 3][live] >= 3).mean() > 0.25, "pixels carry their history across the poses"
    if moments:
        assert (mvar[live] < T.VAR_MAX).all() and (hist[2, ..., 3][live] < T.VAR_MAX).all(), "two samples a pose: nothing is unknown"
    # the defaults: t's parameters, f == NULL, tm == NULL
    md = M.make(TW.temporal_of(cam, offset=(0.5, 0.5) if jitter else (0.0, 0.0)), V.default_temporal_mom()["measured_below"], V.default_temporal_mom()["search"])
    want = M.chain(L, cam, mean, planes, mvar if moments else None, hist, md, FV.make(**V.default_filter_var()), None)
    _same_all(ctx.accum_resolve_hdr_temporal_mom(hist, TW.prev_camera(cam), None, None, None), want, "defaults", NAMES)


def test_an_adaptive_accumulations_resolves_counts_and_variance_do_not_change(ctx, worlds):
    name, jitter, size = "lamp", True, (W, H)

    def run(temporal):
        tex, dim, cam, _ = worlds[name, size, 0]
        ctx.upload_octree(tex, dim)
        ctx.set_params(ctx.default_params())
        ctx.set_camera(*cam)
        ctx.accum_begin(size[0], size[1], FIRST, mode=MODE_FULL, jitter=jitter, adaptive=(2, 6, 40), hdr=True, moments=True)
        ctx.accum_add(2)
        hist = ctx.accum_resolve_hdr_temporal_mom(None, None, {"measured_below": 4, "search": 1})[0] if temporal else None
        mid = ctx.accum_resolve() + ctx.accum_resolve_hdr() + (ctx.accum_counts()[0], ctx.accum_variance()) + tuple(ctx.accum_guides()[k] for k in G.KEYS)
        mid += ctx.accum_resolve_hdr_filtered_var()
        if temporal:
            ctx.accum_resolve_hdr_temporal_mom(hist, TW.prev_camera(cam), {"measured_below": 32769, "search": 1, "max_history": 3})
        ctx.accum_add(3)
        if temporal:
            ctx.accum_resolve_hdr_temporal_mom(hist, TW.prev_camera(cam))
        return mid + ctx.accum_resolve() + ctx.accum_resolve_hdr() + (ctx.accum_counts()[0], ctx.accum_variance()) + tuple(ctx.accum_guides()[k] for k in G.KEYS)

    plain, with_temporal = run(False), run(True)
    assert len(plain) == len(with_temporal) and len(plain) > 20
    for a, b in zip(plain, with_temporal):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_state_errors_and_no_profiling_slot(V, worlds, case70):
    c = V.Context(0)
    try:
        tex, dim, cam, _ = worlds["room", (W, H), 0]
        c.upload_octree(tex, dim)
        c.set_camera(*cam)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # no begin
            c.accum_resolve_hdr_temporal_mom()
        c.accum_begin(W, H, FIRST, hdr=True, moments=True)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # no sample
            c.accum_resolve_hdr_temporal_mom()
        c.accum_begin(W, H, FIRST)
        c.accum_add(1)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # without HDR
            c.accum_resolve_hdr_temporal_mom()
        c.accum_begin(W, H, FIRST, hdr=True, moments=True)
        c.accum_add(1)                                                      # one sample: M3 is "unknown", the call goes through
        c.set_profiling(16)
        hist = c.accum_resolve_hdr_temporal_mom()[0]
        live = hist[1, ..., 3] > 0
        assert (hist[2, ..., 3][live] == T.VAR_MAX).all()
        c.accum_resolve_hdr_temporal_mom(hist, TW.prev_camera(cam), {"measured_below": 4, "search": 1})
        with pytest.raises(V.VrtError, match="vrt error -1"):
            c.accum_resolve_hdr_temporal_mom(hist, TW.prev_camera(cam), {"search": 2})
        with pytest.raises(V.VrtError, match="vrt error -1"):
            c.accum_resolve_hdr_temporal_mom(hist, TW.prev_camera(cam), {"measured_below": 0})
        cam70, prev70, rgb, g, h70, var = case70
        c.temporal_hdr_mom(cam70, rgb, g, var, h70, TW.prev_camera(prev70), {"search": 1})
        assert len(c.profile_read()) == 0
        c.dispatch(W, H)
        assert len(c.profile_read()) == 1                                   # ... while a frame takes one
    finally:
        c.close()
