"""The checker of the temporal pass with measured variances and a 3 x 3 search (tests/oracle_temporal_mom.c: T3s, T7, T6m of
include/vrt.h vrt_temporal_hdr_mom) on the CPU: its identity with tests/oracle_temporal.c, the closed forms of T7, T7 as the variance
it claims to be against the empirical variance of noise frames, the closed forms of T3s against a float32 restatement of the search
in numpy, the checker against its float64 restatement with derived bounds on real frames with their measured variance, four planted
misreadings those catch, and the validation that needs no device."""
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
from test_temporal import STRICT, grey, lum32, random_history, random_planes, sphere

EPS = F.EPS
VAR_MAX = T.VAR_MAX
W, H = 43, 21
MODE_FULL = 2
f32 = np.float32


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
def cams(V):
    return [TW.camera(V, p, (W, H)) for p in TW.poses("room")]


def mom_of(cam_prev=None, measured_below=1, search=0, **kw):
    return M.make(TW.temporal_of(cam_prev, **kw), measured_below, search)


def bad_variance(rng, h, w):
    """a variance plane with every kind of entry"""
    v = (rng.random((h, w)) * 2).astype(f32)
    bad = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0, 0.0, 1e30, 5e9], f32)
    m = rng.random(v.shape) < 0.1
    v[m] = bad[rng.integers(0, len(bad), int(m.sum()))]
    return v


def case70(V):
    """test_gpu_temporal.py's random 70 x 37 case, and a variance plane for it"""
    rng = np.random.default_rng(70)
    rgb, g = random_planes(rng, 37, 70)
    bad = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0, 1e30], f32)
    for a in (rgb, g["normal"], g["depth"], g["coverage"]):
        m = rng.random(a.shape) < 0.05
        a[m] = bad[rng.integers(0, len(bad), int(m.sum()))]
    poses = TW.poses("room")
    hist = random_history(rng, 37, 70)
    return TW.camera(V, poses[2], (70, 37)), TW.camera(V, poses[0], (70, 37)), rgb, g, hist, bad_variance(rng, 37, 70)


# ---- real frames with their measured variance ---------------------------------------------------------------------------------------
_frames = {}


def real_frame(LOM, LG, V, O, name, i, size=(GW.W, GW.H), n=2, jitter=False):
    """pose i of `name` -> (cam, the checker's mean of n samples, its guide planes, its M3 plane), computed once"""
    key = (name, i, size, n, jitter)
    if key not in _frames:
        w = GW.world(V, name)
        tex, dim = w.flatten()
        w.close()
        cam = TW.camera(V, TW.poses(name)[i], size)
        scene = O.make_scene(tex, dim, *cam)
        acc = OM.Accum(LOM, size[1], size[0])
        for k in range(GW.FIRST, GW.FIRST + n):
            acc.add(oracle_hdr.render(LOM, scene, size[0], size[1], MODE_FULL, k, jitter))
        _frames[key] = (cam, acc.mean(), G.planes(LG, scene, size[0], size[1], GW.FIRST, n, jitter)[0], acc.variance())
    return _frames[key]


# ---- identity -----------------------------------------------------------------------------------------------------------------------
def same_but_v(got, want, what):
    """every output of the old rule bit for bit; the history but plane 2's fourth float"""
    F.same(got[1], want[1], f"{what}: integrated")
    F.same(got[2], want[2], f"{what}: variance")
    F.same(got[0][:2], want[0][:2], f"{what}: history planes 0 and 1")
    F.same(got[0][2, ..., :3], want[0][2, ..., :3], f"{what}: the history's normal")


def test_measured_below_1_without_search_is_the_old_rule(L, LOM, LG, V, O):
    cam, cam_prev, rgb, g, hist, var = case70(V)
    for kw in (dict(depth_tol=0.5, normal_min=-1.0), {}, dict(offset=(0.5, 0.5), max_history=7, alpha_min=0.3, alpha_moments_min=0.05)):
        t = TW.temporal_of(cam_prev, **kw)
        for v in (var, None):
            same_but_v(M.temporal(L, cam, rgb, g, v, hist, M.make(t)), T.temporal(L, cam, rgb, g, hist, t), f"70 x 37 {kw}")
    old = new = None
    cam_prev = None
    for i in (0, 1, 2):
        cam, mean, planes, mvar = real_frame(LOM, LG, V, O, "room", i)
        t = TW.temporal_of(cam_prev)
        want = T.temporal(L, cam, mean, planes, old, t)
        got = M.temporal(L, cam, mean, planes, mvar, new, M.make(t))
        same_but_v(got, want, f"room pose {i}")
        old, new, cam_prev = want[0], got[0], cam         # each rule on its own history: they differ in that one float only
    assert (new[2, ..., 3] > 0).any() and not old[2, ..., 3].any()


# ---- closed forms of T7 -------------------------------------------------------------------------------------------------------------
def test_a_first_frame_stores_the_frames_own_variance(L, cams):
    rng = np.random.default_rng(3)
    rgb, g = random_planes(rng, H, W)
    var = bad_variance(rng, H, W)
    live = g["coverage"] > 0
    for below in (1, 2, 4, M.ALWAYS):
        hist, _, out = M.temporal(L, cams[0], rgb, g, var, None, mom_of(None, below))
        F.same(hist[2, ..., 3], np.where(live, FV.hv_of(var), f32(0)), "V' = hv(v), +0 where not live")
        F.same(out, np.where(live, FV.hv_of(var) if below >= 2 else VAR_MAX, f32(0)), f"out_variance at measured_below {below}")
    assert not np.signbit(hist[2, ..., 3]).any()


def check_static_constant_v(L, cam, plant=None, frames=6):
    """a = 1 / N' under an identical camera with the same v every frame: V' after K frames is v / K. The bound, from the operations:
    the reprojected weights are (1, ~1e-5, ...), so a previous quantity is its value within T3's 14 roundings and N' within 15 K EPS
    after K frames (tests/test_temporal.py allows 40 K EPS and so does this); a = 1 / N' then carries 40 K + 1, a * a twice that, and
    om = 1 - a no more than a (K >= 2). Both terms of T7 are positive, so the sum's relative error is the larger term's plus one:
    e(K) <= e(K - 1) + 2 * 40 K + 14 + 3, which sums to 40 K^2 + 57 K."""
    g = sphere(cam, np.asarray(cam[2])[:3], 20.0, W, H)
    v = np.full((H, W), 0.75, f32)
    m = mom_of(cam, M.ALWAYS, alpha_min=0.0, alpha_moments_min=0.0, max_history=1000)
    hist = None
    for k in range(frames):
        hist, _, out = M.temporal(L, cam, grey(1.0), g, v, hist, m, plant=plant if k else None)
        K = k + 1
        tol = (40 * K * K + 57 * K) * EPS
        assert np.abs(hist[2, ..., 3] / (0.75 / K) - 1).max() <= tol, f"V' after {K} frames"
        F.same(out, hist[2, ..., 3], "out_variance is V' at measured_below 32769")


def test_a_constant_variance_under_an_identical_camera_is_v_over_k(L, cams):
    check_static_constant_v(L, cams[0])


def test_once_alpha_min_binds_the_variance_tends_to_its_fixed_point(L, cams):
    """V = (1 - a)^2 V + a^2 v has the fixed point v a / (2 - a); the distance to it shrinks by (1 - a)^2 = 0.36 a frame"""
    cam = cams[0]
    g = sphere(cam, np.asarray(cam[2])[:3], 20.0, W, H)
    v = np.full((H, W), 0.75, f32)
    a = float(f32(0.4))
    m = mom_of(cam, M.ALWAYS, alpha_min=0.4, max_history=64)
    hist = None
    for k in range(40):
        hist = M.temporal(L, cam, grey(1.0), g, v, hist, m)[0]
    assert np.abs(hist[2, ..., 3] / (0.75 * a / (2 - a)) - 1).max() <= 0.36 ** 39 + 100 * EPS


def test_bad_variances_come_out_as_hv_says(L, cams):
    cam = cams[0]
    g = sphere(cam, np.asarray(cam[2])[:3], 20.0, W, H)
    m = mom_of(cam, M.ALWAYS, alpha_min=0.0, max_history=64)
    h1 = M.temporal(L, cam, grey(1.0), g, np.zeros((H, W), f32), None, m)[0]
    for bad, hv in ((np.nan, 0.0), (-2.0, 0.0), (-np.inf, 0.0), (np.inf, float(VAR_MAX)), (1e30, float(VAR_MAX)), (8.0, 8.0)):
        first = M.temporal(L, cam, grey(1.0), g, np.full((H, W), bad, f32), None, m)[0]
        F.same(first[2, ..., 3], np.full((H, W), hv, f32), f"variance_in {bad}")
        h = h1.copy()
        h[2, ..., 3] = bad                                    # a = 1 / 2: V' = hv(w) / 4 + v / 4, v = 0
        second = M.temporal(L, cam, grey(1.0), g, np.zeros((H, W), f32), h, m)[0]
        assert np.isfinite(second).all()
        assert np.abs(second[2, ..., 3] - hv / 4).max() <= 40 * EPS * hv / 4, f"the history's V {bad}"


def test_no_plane_is_a_plane_of_unknown(L, V):
    cam, cam_prev, rgb, g, hist, _ = case70(V)
    m = mom_of(cam_prev, 4, 1, depth_tol=0.5, normal_min=-1.0)
    for a, b in zip(M.temporal(L, cam, rgb, g, None, hist, m), M.temporal(L, cam, rgb, g, np.full((37, 70), VAR_MAX, f32), hist, m)):
        F.same(a, b, "NULL against 65504^2")


# ---- T7 is the variance it claims to be ---------------------------------------------------------------------------------------------
NW, NH = 96, 48                  # 4608 independent pixels
SIGMA = 0.1


def noise_run(L, V, frames, plant=None, **kw):
    """frames of independent grey noise of variance SIGMA^2 about 1 under a static camera -> (the empirical variance of the integrated
    luminance over the pixels, its standard error, the mean V', the mean of T6's estimate)"""
    cam = TW.camera(V, TW.poses("room")[0], (NW, NH))
    g = sphere(cam, np.asarray(cam[2])[:3], 20.0, NW, NH)
    rng = np.random.default_rng(11)
    v = np.full((NH, NW), SIGMA * SIGMA, f32)
    hist = {1: None, M.ALWAYS: None}
    for k in range(frames):
        c = (1.0 + SIGMA * rng.standard_normal((NH, NW))).astype(f32)
        rgb = np.repeat(c[..., None], 3, axis=2)
        for below in hist:
            hist[below], integ, out = M.temporal(L, cam, rgb, g, v, hist[below], mom_of(cam, below, **kw), plant=plant if k else None)
            if below == 1:
                t6 = out
            else:
                t7 = out
    y = lum32(integ).astype(np.float64)
    s2 = float(((y - y.mean()) ** 2).sum() / (y.size - 1))
    # the sample variance of n Gaussian values has the standard error s^2 sqrt(2 / (n - 1))
    return s2, s2 * np.sqrt(2.0 / (y.size - 1)), float(t7.astype(np.float64).mean()), float(t6.astype(np.float64).mean())


def check_noise(L, V, plant=None):
    """-> the two ratios (V' / empirical, T6 / empirical) with a = 1 / N' and with alpha_min binding"""
    out = []
    for what, frames, kw in (("a = 1 / N'", 8, dict(alpha_min=0.0, alpha_moments_min=0.0, max_history=64)),
                             ("alpha_min binds", 12, dict(alpha_min=0.4, alpha_moments_min=0.6, max_history=8))):
        s2, se, t7, t6 = noise_run(L, V, frames, plant, **kw)
        print(f"{what}: empirical {s2:.6g} +- {se:.3g}; V' / empirical {t7 / s2:.4f}; T6 / empirical {t6 / s2:.4f}; bound {4.5 * se / s2:.4f}")
        assert abs(t7 - s2) <= 4.5 * se, f"{what}: T7 {t7} against {s2} +- {se}"
        out.append((t7 / s2, t6 / s2, 4.5 * se / s2))
    return out


def test_the_integrated_variance_is_the_empirical_one(L, V):
    exact, binding = check_noise(L, V)
    assert abs(exact[1] - 1) <= exact[2], "T6 is exact while a = 1 / N'"
    assert abs(binding[1] - 1) > binding[2], "T6 is an approximation once alpha_min binds: it misses the bound T7 keeps"


# ---- closed forms of T3s ------------------------------------------------------------------------------------------------------------
def order_values(rng, h, w):
    """colours on which the order of a float32 sum shows: 16384 and 8192 beside values below their last bit"""
    big = np.array([16384.0, 8192.0, 0.001, 0.0007, 3.0], f32)
    return big[rng.integers(0, len(big), (h, w))]


def search_case(V, size=(W, H), dyaw=0.4, dpitch=0.4, seed=2, edge=None):
    """A history that makes the search matter: the planes of a sphere about the eye (every depth 20, so only the normals and what
    the test kills decide), the previous camera turned by a fraction of a pixel, and in the history: 2 x 2 dead blocks (all four
    bilinear taps of some pixel fail, a neighbour counts), one 7 x 7 dead block (every neighbour fails inside it), the image's
    outermost ring dead (centres on the border with taps outside), history lengths of 1-5, and colours and V on which the order
    of summation shows. edge: a depth step or a normal flip across the history -> (cam, cam_prev, rgb, guides, variance, history)"""
    w, h = size
    pose = TW.poses("room")[0]
    cam = TW.camera(V, pose, size)
    prev = TW.camera(V, (pose[0], pose[1], pose[2], pose[3] + dyaw, pose[4] + dpitch), size)
    centre = np.asarray(pose[:3], f32)
    rng = np.random.default_rng(seed)
    g, gp = sphere(cam, centre, 20.0, w, h), sphere(prev, centre, 20.0, w, h)
    hist = np.zeros((3, h, w, 4), f32)
    for k in range(3):
        hist[0, ..., k] = order_values(rng, h, w)
    hist[0, ..., 3] = rng.integers(1, 6, (h, w))
    hist[1, ..., 0], hist[1, ..., 1] = order_values(rng, h, w), order_values(rng, h, w)
    hist[1, ..., 2], hist[1, ..., 3] = gp["depth"], 1.0
    hist[2, ..., :3], hist[2, ..., 3] = gp["normal"], order_values(rng, h, w)
    alive = np.ones((h, w), bool)
    alive[0, :] = alive[-1, :] = alive[:, 0] = alive[:, -1] = False
    if h > 12 and w > 24:
        for y in range(3, h - 3, 5):
            for x in range(3 + (y % 2), w - 12, 6):
                alive[y:y + 2, x:x + 2] = False
        alive[h // 2 - 3:h // 2 + 4, w - 9:w - 2] = False
    if edge is not None:
        side = np.zeros((h, w), bool)
        side[:, w // 2:] = True
        side[h // 2:, :] ^= True
        if edge == "depth":
            hist[1, ..., 2] = np.where(side, hist[1, ..., 2] * f32(1.5), hist[1, ..., 2])
        else:
            hist[2, ..., :3] = np.where(side[..., None], -hist[2, ..., :3], hist[2, ..., :3])
    hist[1, ..., 3] = alive
    rgb = (rng.random((h, w, 3)) * 4).astype(f32)
    return cam, prev, rgb, g, (rng.random((h, w)) * 2).astype(f32), hist


def search32(hist, g, det, t, reverse=False, centre=None):
    """T3s of every pixel whose details say the search ran, restated in numpy float32 one operation at a time -> {(y, x): (counted,
    the seven previous quantities)}; the tests are T3's, on the history's own words (all finite and in range here: h, g, hv change
    nothing)"""
    h, w = det.shape[:2]
    out = {}
    for y, x in zip(*np.nonzero(det[..., 8])):
        fx, fy, zexp = (f32(v) for v in det[y, x, :3])
        xc, yc = centre(fx, fy) if centre else (int(np.floor(fx + f32(0.5))), int(np.floor(fy + f32(0.5))))
        np_ = g["normal"][y, x].astype(f32)
        taps = [(xc + dx, yc + dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        s, sw, n = [f32(0)] * 7, f32(0), 0
        for qx, qy in (taps[::-1] if reverse else taps):
            if qx < 0 or qx >= w or qy < 0 or qy >= h:
                continue
            q0, q1, q2 = hist[0, qy, qx], hist[1, qy, qx], hist[2, qy, qx]
            nd = f32(f32(f32(q2[0] * np_[0]) + f32(q2[1] * np_[1])) + f32(q2[2] * np_[2]))
            if not (q1[3] > 0 and q0[3] >= 1 and nd >= f32(t.normal_min)):
                continue
            if not (np.abs(f32(q1[2] - zexp)) <= f32(f32(f32(t.depth_tol) * zexp) + f32(2.0 ** -20))):
                continue
            xs = (q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q2[3])
            s = [f32(a + b) for a, b in zip(s, xs)]
            sw, n = f32(sw + f32(1)), n + 1
        out[int(y), int(x)] = (n, [f32(a / sw) for a in s] if n else [f32(0)] * 7)
    return out


def check_search(L, V, plant=None, edge=None, **case):
    """the checker's search against search32 on a search_case -> (its details, how many searched pixels found a history, how many
    found none)"""
    cam, prev, rgb, g, var, hist = search_case(V, edge=edge, **case)
    kw = dict(max_history=64, alpha_min=0.0, alpha_moments_min=0.0, normal_min=0.9, depth_tol=0.05)
    m = mom_of(prev, M.ALWAYS, 1, **kw)
    h2, out, outv, det = M.temporal(L, cam, rgb, g, var, hist, m, plant=plant, details=True)
    ran = det[..., 8] != 0
    # the search runs exactly where T2 gave a position and T3 counted nothing
    fx, fy = det[..., 0], det[..., 1]
    inside = (fx > -1) & (fx < W) & (fy > -1) & (fy < H) & (det[..., 2] != 0)
    assert np.array_equal(ran, inside & (det[..., 7] == 0))
    want = search32(hist, g, det, M.base(m))
    found = none = 0
    a_of = lambda n: f32(1) / n                                   # noqa: E731  (alpha_min 0)
    for (y, x), (n, p) in want.items():
        assert det[y, x, 9] == n, f"({x}, {y}): counted taps"
        nn = f32(min(f32(p[3] + f32(1)), f32(64)))
        assert h2[0, y, x, 3] == nn, f"({x}, {y}): N'"
        a = a_of(nn)
        c = F.h_of(rgb[y, x])
        for j in range(3):
            assert h2[0, y, x, j] == f32(p[j] + f32(a * f32(c[j] - p[j]))), f"({x}, {y}): colour {j}"
        om = f32(f32(1) - a)
        v = f32(f32(f32(om * om) * p[6]) + f32(f32(a * a) * var[y, x]))
        assert h2[2, y, x, 3] == v, f"({x}, {y}): V'"
        found, none = found + (n > 0), none + (n == 0)
    # without the search the same pixels start again, and every other pixel is the same bits
    h0 = M.temporal(L, cam, rgb, g, var, hist, mom_of(prev, M.ALWAYS, 0, **kw))[0]
    assert (h0[0, ..., 3][ran] == 1).all()
    F.same(h0[:, ~ran], h2[:, ~ran], "pixels that do not search")
    for (y, x), (n, p) in want.items():
        if n == 0:
            F.same(h2[:, y, x], h0[:, y, x], "a search that finds nothing is no search")
    return det, found, none, (cam, prev, rgb, g, var, hist, m)


def test_the_search_finds_the_neighbours_in_order(L, V):
    det, found, none, (cam, prev, rgb, g, var, hist, m) = check_search(L, V)
    assert found >= 20 and none >= 1
    fwd, rev = search32(hist, g, det, M.base(m)), search32(hist, g, det, M.base(m), reverse=True)
    assert any(n > 1 and any(a != b for a, b in zip(p, rev[k][1])) for k, (n, p) in fwd.items()), "the order of summation shows on these values"


def test_the_search_with_centres_on_each_border_and_corner(L, V):
    seen = set()
    for dyaw, dpitch in ((0.4, 0.4), (0.4, -0.4), (-0.4, 0.4), (-0.4, -0.4)):
        det, found, none, _ = check_search(L, V, dyaw=dyaw, dpitch=dpitch)
        ran = det[..., 8] != 0
        xc, yc = np.floor(det[..., 0] + f32(0.5)).astype(int), np.floor(det[..., 1] + f32(0.5)).astype(int)
        for name, where in (("left", xc == 0), ("right", xc == W - 1), ("top", yc == 0), ("bottom", yc == H - 1)):
            if (ran & where & (det[..., 9] > 0)).any():
                seen.add(name)
        for name, where in (("top left", (xc == 0) & (yc == 0)), ("top right", (xc == W - 1) & (yc == 0)),
                            ("bottom left", (xc == 0) & (yc == H - 1)), ("bottom right", (xc == W - 1) & (yc == H - 1))):
            if (ran & where).any():
                seen.add(name)
    assert seen == {"left", "right", "top", "bottom", "top left", "top right", "bottom left", "bottom right"}, seen


@pytest.mark.parametrize("edge", ["depth", "normal"])
def test_the_search_rejects_the_neighbours_t3_would(L, V, edge):
    det, found, none, (cam, prev, rgb, g, var, hist, m) = check_search(L, V, edge=edge)
    plain = check_search(L, V)[0]
    assert found >= 10 and (det[..., 9] < plain[..., 9]).sum() >= 10, "the edge takes neighbours away"


def test_a_position_outside_t2s_window_never_searches(L, V, cams):
    pose = TW.poses("room")[0]
    cam = cams[0]
    centre = np.asarray(cam[2])[:3]
    g = sphere(cam, centre, 20.0, W, H)
    for dyaw, dpitch in ((12.0, 0.0), (-12.0, 0.0), (0.0, 9.0), (0.0, -9.0), (180.0, 0.0)):
        prev = TW.camera(V, (pose[0], pose[1], pose[2], pose[3] + dyaw, pose[4] + dpitch), (W, H))
        h1 = M.temporal(L, prev, grey(1.0), sphere(prev, centre, 20.0, W, H), None, None, mom_of())[0]
        h1[1, ..., 3] = 0                                      # nothing to find: every pixel inside the window searches, in vain
        h2, _, _, det = M.temporal(L, cam, grey(1.0), g, None, h1, mom_of(prev, 4, 1), details=True)
        fx, fy = det[..., 0], det[..., 1]
        inside = (fx > -1) & (fx < W) & (fy > -1) & (fy < H) & (det[..., 2] != 0)
        assert np.array_equal(det[..., 8] != 0, inside) and (h2[0, ..., 3] == 1).all() and not det[..., 9].any()
        assert (~inside).sum() > W and (inside.sum() > W or dyaw == 180.0)
        for a, b in zip(M.temporal(L, cam, grey(1.0), g, None, h1, mom_of(prev, 4, 0)), (h2, None, None)):
            if b is not None:
                F.same(a, b, "search 1 against search 0")


# ---- the float64 restatement on real frames -----------------------------------------------------------------------------------------
def check_against_float64(L, prev_frame, frame, below, search, plant=None, seed=0, **kw):
    """tests/test_temporal.py's check with the measured variance of the frame and the new rule -> (the share of live pixels left out,
    how many pixels searched)"""
    cam_prev, _, g_prev, var_prev = prev_frame
    cam, _, g, var = frame
    h, w = g["depth"].shape
    rng = np.random.default_rng(seed)
    rgb = (rng.random((h, w, 3)) * 4).astype(f32)
    m = mom_of(cam_prev, below, search, **kw)
    hist = M.temporal(L, cam_prev, (rng.random((h, w, 3)) * 4).astype(f32), g_prev, var_prev, None, m)[0]
    # histories of many lengths, some of none; none of 1 (tests/test_temporal.py says why), and so none whose N' is measured_below
    # exactly unless the bound says so
    hist[0, ..., 3] = rng.integers(2, 12, (h, w)) * (hist[0, ..., 3] > 0) * (rng.random((h, w)) > 0.05)
    h2, out, outv, det = M.temporal(L, cam, rgb, g, var, hist, m, plant=plant, details=True)
    fx, fy, zexp, reached = T.position64(cam, g, M.base(m))
    live = F.g_of(g["coverage"]) > 0
    sure = live & reached
    for got, want, name in ((det[..., 0], fx, "fx"), (det[..., 1], fy, "fy"), (det[..., 2], zexp, "Zexp")):
        worst = (np.abs(got - want.v) / (1.1 * want.e + 1e-30))[sure].max()
        assert worst <= 1.0, f"{name}: {worst:.2f} of its bound"
    w64, v64, bw, bv, unsure, searched = M.integrate64(rgb, g, var, hist, m, det)
    keep = ~unsure
    assert np.array_equal(searched[keep], (det[..., 8] != 0)[keep]), "where the search ran"
    assert (np.abs(h2 - w64) <= bw)[:, keep].all(), "history"
    assert (np.abs(out - w64[0, ..., :3]) <= bw[0, ..., :3])[keep].all(), "out_rgb"
    assert (np.abs(outv - v64) <= bv)[keep].all(), "variance"
    return float(unsure[live].mean()), int((det[..., 8] != 0).sum())


@pytest.mark.parametrize("name", ["room", "lamp", "outside"])
def test_the_checker_is_its_float64_restatement_on_real_frames(L, LOM, LG, V, O, name):
    """four steps between the poses, the search on, SVGF's tap tests (where histories drop and the search has work) and the defaults
    in turn, measured_below over its values"""
    shares, searched = [], 0
    for k, (i, j) in enumerate(((0, 1), (1, 2), (2, 0), (1, 1))):
        share, n = check_against_float64(L, real_frame(LOM, LG, V, O, name, i), real_frame(LOM, LG, V, O, name, j), (4, M.ALWAYS, 2, 1)[k], 1,
                                         seed=10 * i + j, **(STRICT if (i + j) % 2 else {}))
        shares.append(share)
        searched += n
    print(f"{name}: share of live pixels left out per step {['%.4f' % s for s in shares]}; pixels that searched {searched}")
    assert max(shares) <= 0.02, shares
    assert searched > 0


# ---- planted misreadings ------------------------------------------------------------------------------------------------------------
def test_planted_misreadings_are_caught(L, LOM, LG, V, O, cams):
    with pytest.raises(AssertionError, match="V' after 2"):
        check_static_constant_v(L, cams[0], plant="no_decay")
    with pytest.raises(AssertionError, match="T7"):
        check_noise(L, V, plant="no_decay")
    with pytest.raises(AssertionError):
        check_search(L, V, plant="bilinear_in_search")
    with pytest.raises(AssertionError):
        check_search(L, V, plant="centre_by_floor")
    # N' = 2 on every pixel of a second frame: measured at measured_below 3, but Nprev = 1 is below 2 as well
    cam = cams[0]
    g = sphere(cam, np.asarray(cam[2])[:3], 20.0, W, H)
    v = np.full((H, W), 0.5, f32)
    m = mom_of(cam, 2)
    h1 = M.temporal(L, cam, grey(1.0), g, v, None, m)[0]
    good = M.temporal(L, cam, grey(2.0), g, v, h1, m)
    planted = M.temporal(L, cam, grey(2.0), g, v, h1, m, plant="switch_on_nprev")
    assert (good[0][0, ..., 3] == 2).all()
    F.same(good[2], T.temporal(L, cam, grey(2.0), g, h1, M.base(m))[2], "N' = 2 is not below 2: T6's value")
    with pytest.raises(AssertionError):
        F.same(planted[2], good[2], "the switch on Nprev")
    frames = [real_frame(LOM, LG, V, O, "room", i) for i in (1, 2)]
    for plant in ("no_decay", "bilinear_in_search", "centre_by_floor", "switch_on_nprev"):     # ... and the float64 restatement sees all four
        with pytest.raises(AssertionError):
            check_against_float64(L, frames[0], frames[1], 4, 1, plant=plant, **STRICT)


# ---- what needs no device -----------------------------------------------------------------------------------------------------------
def test_the_defaults_and_the_struct(V):
    d = V.default_temporal_mom()
    assert set(d) == set(V.TEMPORAL_MOM_KEYS) and 1 <= d["measured_below"] <= 32769 and d["search"] in (0, 1)
    assert {k: d[k] for k in V.TEMPORAL_KEYS} == V.default_temporal(), "vrt_temporal_default's fields as they are"
    assert C.sizeof(V.TemporalMom) == C.sizeof(M.TemporalMom) == 116
    assert V.TemporalMom.measured_below.offset == C.sizeof(V.Temporal) == 108
    t = V.TemporalMom()
    t.prev_view_proj[0] = 5.0
    V.hip_lib().vrt_temporal_mom_default(C.byref(t))
    assert not any(t.prev_view_proj) and not any(t.prev_camera_pos)
    with pytest.raises(ValueError, match="unknown temporal key"):
        V.Context._temporal_mom({"searches": 1}, None)
