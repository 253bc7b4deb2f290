"""The temporal pass on the MI355X (vrt_temporal_hdr, its host form and the accumulation forms) against the checker
(tests/oracle_temporal.c), bit for bit on every output: random planes on a real camera block with every kind of bad input in the
planes and in the history at a ragged frame size, the smallest frames, a first frame, reprojections that leave the previous image
on each side, each optional output NULL in turn on a caller's stream, the error codes, buffer growth, the accumulation route over
three poses with the history ping-ponged on both traversal routes and ray sources, the accumulation's own resolves untouched, and no
profiling slot taken."""
import ctypes as C

import numpy as np
import pytest

import guide_worlds as GW
import oracle_filter_hdr as F
import oracle_filter_var as FV
import oracle_guides as G
import oracle_hdr
import oracle_temporal as T
import temporal_worlds as TW
from test_temporal import random_history, random_planes, sphere

pytestmark = pytest.mark.gpu

W, H, FIRST = GW.W, GW.H, GW.FIRST
N = 2                       # samples per pose
MODE_FULL = 2
SWEPT = dict(sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=1.0, sigma_lum=2.0)
LOOSE = dict(depth_tol=0.5, normal_min=-1.0)     # random planes agree with no history: let the tests pass, the sanitising decide


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return T.build(tmp_path_factory.mktemp("oracle_temporal"))


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


def _keys(t):
    """an oracle Temporal's parameters as the dict Context.temporal_hdr takes"""
    return {k: getattr(t, k) for k in ("offset_x", "offset_y", "max_history", "alpha_min", "alpha_moments_min", "normal_min", "depth_tol")}


def _same_all(got, want, what, names=("history", "integrated", "variance")):
    assert len(got) == len(want) == len(names)
    for g, w, n in zip(got, want, names):
        F.same(g, w, f"{what}: {n}")


def _run_host(ctx, L, cam, rgb, g, hist, cam_prev, what, **kw):
    """the host form against the checker -> the new history"""
    t = TW.temporal_of(cam_prev if hist is not None else None, **kw)
    want = T.temporal(L, cam, rgb, g, hist, t)
    got = ctx.temporal_hdr(cam, rgb, g, hist, TW.prev_camera(cam_prev) if hist is not None else None, _keys(t))
    _same_all(got, want, what)
    return want[0]


# ---- the stateless form on random planes -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case70(V):
    """70 x 37 planes on the room's camera: depths of 5-40, axis normals, dead blocks, bad entries; a history with NaN, Inf, negative
    and zero entries; the previous camera yawed and moved"""
    rng = np.random.default_rng(70)
    rgb, g = random_planes(rng, 37, 70)
    bad = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0, 1e30], np.float32)
    for a in (rgb, g["normal"], g["depth"], g["coverage"]):
        m = rng.random(a.shape) < 0.05
        a[m] = bad[rng.integers(0, len(bad), int(m.sum()))]
    poses = TW.poses("room")
    return TW.camera(V, poses[2], (70, 37)), TW.camera(V, poses[0], (70, 37)), rgb, g, random_history(rng, 37, 70)


@pytest.mark.parametrize("kw", [LOOSE, dict(LOOSE, offset=(0.5, 0.5), max_history=7, alpha_min=0.3, alpha_moments_min=0.05), {},
                                dict(LOOSE, offset=(1.0, 0.0), max_history=32768, alpha_min=0.0, alpha_moments_min=1.0)],
                         ids=["loose", "jittered", "defaults", "extremes"])
def test_random_planes_are_the_checkers(ctx, L, case70, kw):
    cam, cam_prev, rgb, g, hist = case70
    t = TW.temporal_of(cam_prev, **kw)
    want = T.temporal(L, cam, rgb, g, hist, t, details=True)
    _same_all(ctx.temporal_hdr(cam, rgb, g, hist, TW.prev_camera(cam_prev), _keys(t)), want[:3], str(kw))
    if kw:
        assert want[3][..., 3:7].any(axis=2).mean() > 0.3 and (want[0][0, ..., 3] > 1).mean() > 0.3    # taps count ...
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and np.isfinite(want[2]).all()
    _run_host(ctx, L, cam_prev, rgb[::-1].copy(), g, want[0], cam, "the next frame, on the pass's own history", **kw)   # ... and carry on


def test_a_first_frame_reads_no_previous_camera(ctx, V, L, case70):
    cam, _, rgb, g, _ = case70
    want = T.temporal(L, cam, rgb, g, None, TW.temporal_of())
    _same_all(ctx.temporal_hdr(cam, rgb, g), want, "history_in == NULL")
    nan = (np.full(16, np.nan, np.float32), np.full(4, np.nan, np.float32))
    t = V.Context._temporal(None, nan)
    out_h, out, outv = np.zeros_like(want[0]), np.zeros_like(want[1]), np.zeros_like(want[2])
    ptr = [a.ctypes.data for a in (*cam, rgb, g["normal"], g["depth"], g["coverage"])]
    assert V.hip_lib().vrt_temporal_hdr_host(ctx._h, 70, 37, *ptr, None, C.byref(t), out_h.ctypes.data, out.ctypes.data, outv.ctypes.data) == 0
    _same_all((out_h, out, outv), want, "a previous camera of NaN, never read")
    F.same(want[0][0, ..., 3], (F.g_of(g["coverage"]) > 0).astype(np.float32), "N' = 1 on every live pixel")


@pytest.mark.parametrize("size", [(8, 8), (9, 1), (1, 1), (1, 9), (65, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_smallest_frames(ctx, V, L, size):
    """one tile, a row and a column narrower than a tile, one pixel; 65 x 5: one pixel past the workgroup's four tiles"""
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    poses = TW.poses("lamp")
    cams = [TW.camera(V, p, size) for p in poses]
    hist = None
    for k in range(3):
        rgb, g = random_planes(rng, h, w, dead=w * h > 9)
        g["depth"][:] = 20
        hist = _run_host(ctx, L, cams[k], rgb, g, hist, cams[k - 1], f"{size} frame {k}", **LOOSE)
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
    h1 = _run_host(ctx, L, prev, rgb, sphere(prev, centre, 20.0, *size), None, None, "previous")
    h2 = _run_host(ctx, L, cam, rgb[:, ::-1].copy(), sphere(cam, centre, 20.0, *size), h1, prev, "current")
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


def test_device_form_each_output_null_in_turn_on_a_callers_stream(ctx, L, case70):
    import torch
    cam, cam_prev, rgb, g, hist = case70
    ins = _to_device(torch, rgb, g["normal"], g["depth"], g["coverage"])
    d_hist = _to_device(torch, hist)[0]
    outs = _outputs(torch, 37, 70)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    for history in (None, d_hist):
        t = TW.temporal_of(cam_prev if history is not None else None, **LOOSE)
        want = T.temporal(L, cam, rgb, g, hist if history is not None else None, t)
        for stream in (None, side.cuda_stream):
            for used in ((1, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0)):
                for o in outs:
                    o.zero_()
                torch.cuda.synchronize()
                ctx.temporal_hdr_device(70, 37, cam, *(i.data_ptr() for i in ins), history.data_ptr() if history is not None else None,
                                        *(o.data_ptr() if u else None for o, u in zip(outs, used)), TW.prev_camera(cam_prev), _keys(t),
                                        stream=stream)
                torch.cuda.synchronize()
                _check_outputs(outs, used, want, f"history {history is not None} stream {stream} outputs {used}")


def test_invalid_arguments(ctx, V, case70):
    import torch
    cam, cam_prev, rgb, g, hist = case70
    w, h = 70, 37
    keep = _to_device(torch, rgb, g["normal"], g["depth"], g["coverage"], hist)
    ins = [t.data_ptr() for t in keep]
    out_h, out, outv = _outputs(torch, h, w)
    lib, hnd = V.hip_lib(), ctx._h
    cam_ptr = [a.ctypes.data for a in cam]
    good = V.Context._temporal(None, TW.prev_camera(cam_prev))

    def call(cam=cam_ptr, ins=ins, t=good, oh=out_h.data_ptr(), o=out.data_ptr(), ov=outv.data_ptr(), size=(w, h)):
        return lib.vrt_temporal_hdr(hnd, size[0], size[1], *cam, *ins, C.byref(t) if t else None, oh, o, ov, None)

    def with_(**kw):
        t = V.Context._temporal(None, TW.prev_camera(cam_prev))
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    assert call() == 0
    for i in range(4):                                                       # a NULL input; an output aliasing that input
        assert call(ins=ins[:i] + [None] + ins[i + 1:]) == -1
        assert call(oh=ins[i]) == -1 and call(o=ins[i]) == -1 and call(ov=ins[i]) == -1
    assert call(ins=ins[:4] + [None]) == 0                                   # the history may be NULL ...
    assert call(oh=ins[4]) == -1 and call(o=ins[4]) == -1                    # ... and is an input where it is not
    assert call(oh=None) == -1 and call(t=None) == -1
    assert call(o=None) == 0 and call(ov=None) == 0 and call(o=None, ov=None) == 0
    assert call(o=out_h.data_ptr()) == -1 and call(ov=out.data_ptr()) == -1  # two outputs in one place
    assert call(oh=out_h.data_ptr() + 4) == -1 and call(ins=ins[:4] + [ins[4] + 8]) == -1     # a history holds whole 16-byte words
    for i in range(3):
        assert call(cam=cam_ptr[:i] + [None] + cam_ptr[i + 1:]) == -1
        broken = [np.array(a, np.float32) for a in cam]
        broken[i][1] = np.inf if i else np.nan
        assert call(cam=[a.ctypes.data for a in broken]) == -1
    for bad in (dict(max_history=0), dict(max_history=32769), dict(max_history=-3), dict(alpha_min=-0.1), dict(alpha_min=1.5),
                dict(alpha_min=float("nan")), dict(alpha_moments_min=-1e-9), dict(alpha_moments_min=2.0), dict(normal_min=-1.5),
                dict(normal_min=1.01), dict(normal_min=float("nan")), dict(depth_tol=0.0), dict(depth_tol=-1.0), dict(depth_tol=float("inf")),
                dict(depth_tol=float("nan")), dict(offset_x=-0.1), dict(offset_y=1.1), dict(offset_x=float("nan"))):
        assert call(t=with_(**bad)) == -1, bad
    assert call(t=with_(max_history=1, alpha_min=0.0, alpha_moments_min=1.0, normal_min=-1.0, depth_tol=1e30, offset_x=1.0)) == 0
    nan_prev = with_()
    nan_prev.prev_view_proj[5] = float("inf")
    assert call(t=nan_prev) == -1 and call(ins=ins[:4] + [None], t=nan_prev) == 0       # read only where a history comes in
    nan_prev = with_()
    nan_prev.prev_camera_pos[2] = float("nan")
    assert call(t=nan_prev) == -1
    assert call(size=(0, h)) == -1 and call(size=(w, -1)) == -1 and call(size=(1 << 16, 1 << 15)) == -1
    host = [a.ctypes.data for a in (rgb, g["normal"], g["depth"], g["coverage"], hist)]
    oh, o, ov = np.zeros((3, h, w, 4), np.float32), np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
    assert lib.vrt_temporal_hdr_host(hnd, w, h, *cam_ptr, *host, C.byref(good), oh.ctypes.data, None, None) == 0
    assert lib.vrt_temporal_hdr_host(hnd, w, h, *cam_ptr, *host, C.byref(good), None, o.ctypes.data, ov.ctypes.data) == -1
    assert lib.vrt_temporal_hdr_host(hnd, w, h, *cam_ptr, *host, C.byref(good), host[4], o.ctypes.data, ov.ctypes.data) == -1
    assert lib.vrt_temporal_hdr_host(hnd, w, h, *cam_ptr, *host[:2], None, host[3], host[4], C.byref(good), oh.ctypes.data, None, None) == -1
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
            _run_host(c, L, cam, rgb, g, hist, cam_prev, f"call {i}", **LOOSE)
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


def _ref(L, LG, worlds, name, jitter, size, i):
    """the checker's mean and planes of the N samples of pose i, computed once"""
    key = (name, jitter, size, i)
    if key not in _refs:
        scene = worlds[name, size, i][3]
        acc = oracle_hdr.Accum(L, size[1], size[0])
        for k in range(FIRST, FIRST + N):
            acc.add(oracle_hdr.render(L, scene, size[0], size[1], MODE_FULL, k, jitter))
        _refs[key] = (acc.mean(), G.planes(LG, scene, size[0], size[1], FIRST, N, jitter)[0])
    return _refs[key]


def _open(ctx, worlds, name, jitter, size, i, upload=True):
    tex, dim, cam, _ = worlds[name, size, i]
    if upload:
        ctx.upload_octree(tex, dim)
        ctx.set_params(ctx.default_params())
    ctx.set_camera(*cam)
    ctx.set_lens(0.0, 1.0)
    ctx.accum_begin(size[0], size[1], FIRST, mode=MODE_FULL, jitter=jitter, hdr=True)
    assert ctx.accum_add(N) == N
    return cam


@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("jitter", [False, True], ids=["corner", "jitter"])
@pytest.mark.parametrize("name", ["room", "lamp"])
@pytest.mark.parametrize("size", [(W, H), GW.RAGGED], ids=["40x24", "43x21"])
def test_three_poses_with_the_history_ping_ponged_are_the_checker_chain(ctx, V, L, LG, worlds, size, name, jitter, variant):
    import torch
    ctx.set_variant(variant)
    w, h = size
    f, fo = {"levels": 3, "demodulate": True, **SWEPT}, FV.make(3, True, **SWEPT)
    kw = dict(alpha_min=0.2, alpha_moments_min=0.1, max_history=8)
    d_mean = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    d = {"normal": torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"), "albedo": torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0"),
         "depth": torch.zeros((h, w), dtype=torch.float32, device="cuda:0"), "coverage": torch.zeros((h, w), dtype=torch.float32, device="cuda:0")}
    d_hist = [torch.zeros((3, h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    d_int, d_var = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"), torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
    d_out = (torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"), torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0"),
             torch.zeros((h, w), dtype=torch.float32, device="cuda:0"))
    torch.cuda.synchronize()
    hist, cam_prev, grown = None, None, 0
    names = ("history", "integrated", "filtered floats", "bytes", "variance")
    for i in (0, 1, 2, 1):
        what = f"{name} {size} jitter {jitter} variant {variant} pose {i}"
        cam = _open(ctx, worlds, name, jitter, size, i, upload=cam_prev is None)
        mean, planes = _ref(L, LG, worlds, name, jitter, size, i)
        t = TW.temporal_of(cam_prev, offset=(0.5, 0.5) if jitter else (0.0, 0.0), **kw)
        want = T.chain(L, cam, mean, planes, hist, t, fo, "reinhard", 0.8)
        prev = TW.prev_camera(cam_prev) if hist is not None else None
        # the offsets are the call's own: what the caller passes is replaced
        got = ctx.accum_resolve_hdr_temporal(hist, prev, dict(kw, offset_x=0.25, offset_y=1.0), f, "reinhard", 0.8)
        _same_all(got, want, what, names)
        # ... and vrt_temporal_hdr plus vrt_filter_hdr_var fed with the device resolves
        ctx.accum_resolve_hdr_device(d_mean.data_ptr(), None, None)
        ctx.accum_guides_device(*(d[k].data_ptr() for k in G.KEYS))
        src, dst = d_hist[grown % 2], d_hist[(grown + 1) % 2]
        ctx.temporal_hdr_device(w, h, cam, d_mean.data_ptr(), d["normal"].data_ptr(), d["depth"].data_ptr(), d["coverage"].data_ptr(),
                                src.data_ptr() if hist is not None else None, dst.data_ptr(), d_int.data_ptr(), d_var.data_ptr(), prev, _keys(t))
        ctx.filter_hdr_var_device(w, h, d_int.data_ptr(), *(d[k].data_ptr() for k in G.KEYS), d_var.data_ptr(), *(o.data_ptr() for o in d_out),
                                  f, "reinhard", 0.8)
        ctx.synchronize()
        torch.cuda.synchronize()
        _same_all([dst.cpu().numpy(), d_int.cpu().numpy()] + [o.cpu().numpy() for o in d_out], want, what + ": the stateless forms on the device planes", names)
        hist, cam_prev, grown = want[0], cam, grown + 1
    live = F.g_of(planes["coverage"]) > 0
    assert (hist[0, ..., 3][live] >= 3).mean() > 0.25, "pixels carry their history across the poses"
    # the defaults: t's parameters, f == NULL, tm == NULL
    want = T.chain(L, cam, mean, planes, hist, TW.temporal_of(cam, offset=(0.5, 0.5) if jitter else (0.0, 0.0)), FV.make(**V.default_filter_var()), None)
    _same_all(ctx.accum_resolve_hdr_temporal(hist, TW.prev_camera(cam), None, None, None), want, "defaults", names)


def test_the_device_form_on_a_callers_stream_each_output_null_in_turn(ctx, V, L, LG, worlds):
    import torch
    name, jitter, size = "lamp", True, GW.RAGGED
    w, h = size
    f, fo = {"levels": 4, "demodulate": True, **SWEPT}, FV.make(4, True, **SWEPT)
    cam0 = _open(ctx, worlds, name, jitter, size, 0)
    first = T.chain(L, cam0, *_ref(L, LG, worlds, name, jitter, size, 0), None, TW.temporal_of(offset=(0.5, 0.5)), fo)
    cam = _open(ctx, worlds, name, jitter, size, 1, upload=False)
    want = T.chain(L, cam, *_ref(L, LG, worlds, name, jitter, size, 1), first[0], TW.temporal_of(cam0, offset=(0.5, 0.5)), fo)
    d_in = _to_device(torch, first[0])[0]
    outs = _outputs(torch, h, w)[:2] + (torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"),
                                        torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0"), torch.zeros((h, w), dtype=torch.float32, device="cuda:0"))
    names = ("history", "integrated", "filtered floats", "bytes", "variance")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    for stream, used in ((None, (1, 1, 1, 1, 1)), (side.cuda_stream, (1, 1, 1, 1, 1)), (side.cuda_stream, (1, 0, 1, 0, 1)),
                         (None, (1, 1, 0, 1, 0)), (side.cuda_stream, (1, 0, 1, 1, 0))):
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        ctx.accum_resolve_hdr_temporal_device(d_in.data_ptr(), *(o.data_ptr() if u else None for o, u in zip(outs, used)), TW.prev_camera(cam0),
                                              None, f, stream=stream)
        torch.cuda.synchronize()
        _check_outputs(outs, used, want, f"stream {stream} outputs {used}", names)
        _same_all(ctx.accum_resolve_hdr_temporal(first[0], TW.prev_camera(cam0), None, f), want, "host form", names)
    for bad in ((1, 1, 0, 0, 1), (0, 1, 1, 1, 1)):                            # no colour output of the filter; no history_out
        with pytest.raises(Exception, match="vrt error -1"):
            ctx.accum_resolve_hdr_temporal_device(d_in.data_ptr(), *(o.data_ptr() if u else None for o, u in zip(outs, bad)), TW.prev_camera(cam0), None, f)
    with pytest.raises(Exception, match="vrt error -1"):                       # history_out == history_in
        ctx.accum_resolve_hdr_temporal_device(d_in.data_ptr(), d_in.data_ptr(), *(o.data_ptr() for o in outs[1:]), TW.prev_camera(cam0), None, f)
    with pytest.raises(Exception, match="vrt error -1"):
        ctx.accum_resolve_hdr_temporal(first[0], TW.prev_camera(cam0), {"max_history": 0}, f)
    lib, t0 = V.hip_lib(), V.Context._temporal(None, None)
    oh, o = np.zeros((3, h, w, 4), np.float32), np.zeros((h, w, 3), np.float32)
    for bad_f, bad_tm, code in ((V.FilterVar(1, 1, 1, 1, 1, 0.0), None, -1), (V.FilterVar(9, 1, 1, 1, 1, 1), None, -1), (None, V.Tonemap(2, 1.0), -1),
                                (None, None, 0)):                              # the filter's and the tone map's own validation
        assert lib.vrt_accum_resolve_hdr_temporal(ctx._h, C.byref(t0), C.byref(bad_f) if bad_f else None, C.byref(bad_tm) if bad_tm else None, None,
                                                  oh.ctypes.data, None, o.ctypes.data, None, None) == code


def test_the_accumulations_own_resolves_do_not_change(ctx, worlds):
    name, jitter, size = "lamp", True, (W, H)

    def run(temporal):
        cam = _open(ctx, worlds, name, jitter, size, 0)
        hist = None
        if temporal:
            hist = ctx.accum_resolve_hdr_temporal()[0]
        mid = ctx.accum_resolve() + ctx.accum_resolve_hdr() + tuple(ctx.accum_guides()[k] for k in G.KEYS) + ctx.accum_resolve_hdr_filtered_var()
        if temporal:
            ctx.accum_resolve_hdr_temporal(hist, TW.prev_camera(cam), {"max_history": 3})
        ctx.accum_add(3)
        if temporal:
            ctx.accum_resolve_hdr_temporal(hist, TW.prev_camera(cam))
        return mid + ctx.accum_resolve() + ctx.accum_resolve_hdr() + tuple(ctx.accum_guides()[k] for k in G.KEYS)

    plain, with_temporal = run(False), run(True)
    assert len(plain) == len(with_temporal) == 23
    for a, b in zip(plain, with_temporal):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_state_errors_and_no_profiling_slot(V, worlds, case70):
    c = V.Context(0)
    try:
        tex, dim, cam, _ = worlds["room", (W, H), 0]
        c.upload_octree(tex, dim)
        c.set_camera(*cam)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # no begin
            c.accum_resolve_hdr_temporal()
        c.accum_begin(W, H, FIRST, hdr=True)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # no sample
            c.accum_resolve_hdr_temporal()
        c.accum_begin(W, H, FIRST)
        c.accum_add(1)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # without HDR
            c.accum_resolve_hdr_temporal()
        c.accum_begin(W, H, FIRST, hdr=True)
        c.accum_add(1)
        c.set_profiling(16)
        hist = c.accum_resolve_hdr_temporal()[0]
        c.accum_resolve_hdr_temporal(hist, TW.prev_camera(cam))
        cam70, prev70, rgb, g, h70 = case70
        c.temporal_hdr(cam70, rgb, g, h70, TW.prev_camera(prev70))
        assert len(c.profile_read()) == 0
        c.dispatch(W, H)
        assert len(c.profile_read()) == 1                                   # ... while a frame takes one
        moved = V.camera_block((cam[2][0] + 1.25, cam[2][1], cam[2][2] - 0.5), 40.0, -8.0, W, H)[:3]
        c.set_camera(*cam)
        assert c.accum_add(1) == 2                                          # one guide sample missing ...
        c.set_camera(*moved)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # ... and nothing to march it with: vrt_accum_guides' rule
            c.accum_resolve_hdr_temporal(hist, TW.prev_camera(cam))
    finally:
        c.close()
