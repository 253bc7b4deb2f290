"""The temporal pass's checker (tests/oracle_temporal.c) on the CPU: a first frame, an identical camera, constant and alternating
images with their closed forms, taps across a depth step and a normal flip, reprojections that leave the previous image or face away
from it, the parameters that bind, bad inputs, the checker against its two-stage float64 restatement with derived bounds on the
guide planes of real frames, four planted misreadings those catch, and the validation that needs no device."""
import ctypes as C

import numpy as np
import pytest

import guide_worlds as GW
import oracle_filter_hdr as F
import oracle_guides as G
import oracle_temporal as T
import temporal_worlds as TW

EPS = F.EPS
VAR_MAX = T.VAR_MAX
W, H = 43, 21


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return T.build(tmp_path_factory.mktemp("oracle_temporal"))


@pytest.fixture(scope="module")
def LG(tmp_path_factory):
    return G.build(tmp_path_factory.mktemp("oracle_guides"))


def random_planes(rng, h, w, dead=True):
    """depths of 5-40, axis normals, blocks of pixels that are not live, and a colour plane"""
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    g = {"normal": axes[rng.integers(0, 6, (h, w))], "depth": (5 + 35 * rng.random((h, w))).astype(np.float32),
         "coverage": np.ones((h, w), np.float32), "albedo": rng.random((h, w, 4)).astype(np.float32)}
    if dead:
        for _ in range(3):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            g["coverage"][y:y + 3, x:x + 4] = 0.0
    return (rng.random((h, w, 3)) * 4).astype(np.float32), g


def random_history(rng, h, w):
    """a history with every kind of entry: NaN, Inf, negative, zero, huge, and ordinary ones"""
    hist = (rng.random((3, h, w, 4)) * 3).astype(np.float32)
    hist[0, ..., 3] = rng.integers(0, 40, (h, w))
    hist[1, ..., 2] = 5 + 35 * rng.random((h, w))
    hist[1, ..., 3] = rng.random((h, w)) > 0.1
    bad = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0, 0.0, 1e30, 5e9], np.float32)
    m = rng.random(hist.shape) < 0.08
    hist[m] = bad[rng.integers(0, len(bad), int(m.sum()))]
    return hist


def sphere(cam, centre, radius, w, h, offset=(0.0, 0.0)):
    """the planes of a sphere seen from inside: depth along each pixel's ray, the inward normal, every pixel live"""
    d = T.rays64(cam, w, h, offset)
    oc = np.asarray(cam[2], np.float64)[:3] - np.asarray(centre, np.float64)
    b = d @ oc
    t = -b + np.sqrt(b * b - (oc @ oc - radius * radius))
    n = (np.asarray(centre, np.float64) - (np.asarray(cam[2], np.float64)[:3] + t[..., None] * d)) / radius
    return {"normal": n.astype(np.float32), "depth": t.astype(np.float32), "coverage": np.ones((h, w), np.float32),
            "albedo": np.full((h, w, 4), 0.5, np.float32)}


def grey(v, h=H, w=W):
    return np.full((h, w, 3), v, np.float32)


def lum32(rgb):
    c = F.h_of(rgb)
    return (np.float32(0.2126) * c[..., 0] + np.float32(0.7152) * c[..., 1]) + np.float32(0.0722) * c[..., 2]


@pytest.fixture(scope="module")
def cams(V):
    """the room's three poses at W x H"""
    return [TW.camera(V, p, (W, H)) for p in TW.poses("room")]


# ---- a first frame ------------------------------------------------------------------------------------------------------------------
def test_without_a_history_a_pixel_returns_its_own_colour_and_moments(L, cams):
    rng = np.random.default_rng(1)
    rgb, g = random_planes(rng, H, W)
    rgb[2, 3] = (np.nan, -1.0, 1e9)
    hist, out, var = T.temporal(L, cams[0], rgb, g, None, TW.temporal_of())
    live = g["coverage"] > 0
    F.same(out, F.h_of(rgb), "c' = h(c)")
    F.same(hist[0, ..., :3], F.h_of(rgb), "the history's colour")
    y = lum32(rgb)
    F.same(hist[0, ..., 3], live.astype(np.float32), "N' = 1, 0 where not live")
    F.same(hist[1, ..., 0], np.where(live, y, np.float32(0)), "m1 = Y")
    F.same(hist[1, ..., 1], np.where(live, y * y, np.float32(0)), "m2 = Y * Y")
    F.same(hist[1, ..., 2], np.where(live, g["depth"], np.float32(0)), "Z")
    F.same(hist[2, ..., :3], np.where(live[..., None], g["normal"], np.float32(0)), "n")
    F.same(var, np.where(live, VAR_MAX, np.float32(0)), "variance 65504^2, +0 where not live")
    assert not hist[2, ..., 3].any() and not np.signbit(hist[2, ..., 3]).any()


# ---- an identical camera ------------------------------------------------------------------------------------------------------------
def check_identical_camera(L, cam, offset, plant=None):
    g = sphere(cam, np.asarray(cam[2])[:3] + np.float32(1.5), 20.0, W, H, offset)
    t = TW.temporal_of(cam, offset=offset)
    h1 = T.temporal(L, cam, grey(1.0), g, None, t)[0]
    h2, _, _, det = T.temporal(L, cam, grey(1.0), g, h1, t, plant=plant, details=True)
    fx, fy, _, reached = T.position64(cam, g, t)
    assert reached.all()
    ys, xs = np.mgrid[0:H, 0:W]
    assert (np.abs(det[..., 0] - xs) <= 1.1 * fx.e + np.abs(fx.v - xs)).all() and (np.abs(fx.v - xs) <= 1e-3).all(), "fx is the pixel's own x"
    assert (np.abs(det[..., 1] - ys) <= 1.1 * fy.e + np.abs(fy.v - ys)).all() and (np.abs(fy.v - ys) <= 1e-3).all(), "fy is the pixel's own y"
    assert (np.abs(det[..., 0] - fx.v) <= 1.1 * fx.e).all() and (np.abs(det[..., 1] - fy.v) <= 1.1 * fy.e).all()
    F.same(h2[0, ..., 3], np.full((H, W), 2, np.float32), "N' = N + 1")


@pytest.mark.parametrize("offset", [(0.0, 0.0), (0.5, 0.5), (0.25, 1.0)])
def test_an_identical_camera_finds_every_pixel_where_it_was(L, cams, offset):
    check_identical_camera(L, cams[0], offset)


# ---- constant and alternating images ------------------------------------------------------------------------------------------------
def check_constant_image(L, V, plant=None):
    """Every channel a power of two and Y(1, 1, 1) = 1.0f exactly: each w * X is exact, a sum is X times sw's own rounded sums and
    the quotient X, so colour, m1 = Y and m2 = Y * Y come back exactly whatever the weights are, and m2 - m1 * m1 = +0. The camera
    yaws a pixel's fraction per frame around the sphere's centre, so the weights are not trivial and border taps are missing."""
    pose = TW.poses("room")[0]
    centre = np.asarray(pose[:3], np.float32)
    hist, cam_prev = None, None
    for k in range(5):
        cam = TW.camera(V, (pose[0], pose[1], pose[2], pose[3] + 0.13 * k, pose[4]), (W, H))
        g = sphere(cam, centre, 20.0, W, H)
        hist, out, var, det = T.temporal(L, cam, grey(4.0), g, hist, TW.temporal_of(cam_prev, alpha_min=0.0, alpha_moments_min=0.0),
                                         plant=plant if k else None, details=True)
        F.same(out, grey(4.0), f"frame {k}: the image")
        F.same(hist[1, ..., 0], np.full((H, W), 4, np.float32), f"frame {k}: m1")
        F.same(hist[1, ..., 1], np.full((H, W), 16, np.float32), f"frame {k}: m2")
        grown = hist[0, ..., 3] >= 2
        assert (var[grown] == 0).all() and not np.signbit(var[grown]).any() and (var[~grown] == VAR_MAX).all()
        if k:
            assert grown.mean() > 0.9 and (det[..., 7] > 0).mean() > 0.9 and ((det[..., 7] > 0) & (det[..., 7] < 0.99)).any()
        cam_prev = cam


def test_a_constant_image_stays_that_image_exactly_with_variance_zero(L, V):
    check_constant_image(L, V)


def check_alternating_values(L, cam, plant=None, frames=6):
    """a = am = 1 / N' under a static camera: after K frames m1 and m2 are the means of Y and Y * Y over the frames and the variance
    their spread / (K - 1), the variance of the mean. The reprojected weights are (1, ~1e-5, ...) and every pixel holds the same
    values, so a previous quantity is its value within the 14 roundings of T3; K frames compound to 40 K EPS, relatively."""
    g = sphere(cam, np.asarray(cam[2])[:3], 20.0, W, H)
    t = TW.temporal_of(cam, alpha_min=0.0, alpha_moments_min=0.0, max_history=1000)
    hist, ys = None, []
    for k in range(frames):
        v = 0.5 if k % 2 == 0 else 2.0
        ys.append(v)
        hist, out, var = T.temporal(L, cam, grey(v), g, hist, t, plant=plant)
        K = k + 1
        m1, m2 = np.mean(ys), np.mean(np.square(ys))
        tol = 40 * K * EPS
        assert np.abs(hist[0, ..., 3] / K - 1).max() <= tol, f"N' after {K} frames"
        assert np.abs(out / m1 - 1).max() <= tol and np.abs(hist[1, ..., 0] / m1 - 1).max() <= tol, f"m1 after {K} frames"
        assert np.abs(hist[1, ..., 1] / m2 - 1).max() <= tol, f"m2 after {K} frames"
        if K >= 2:
            want = (m2 - m1 * m1) / (K - 1)
            assert np.abs(var - want).max() <= 3 * tol * (m2 + m1 * m1) / (K - 1), f"variance after {K} frames"


def test_two_alternating_values_give_the_closed_form_moments(L, cams):
    check_alternating_values(L, cams[0])


# ---- taps across an edge ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", ["depth", "normal"])
def test_an_edge_fails_exactly_the_taps_across_it(L, cams, edge):
    cam = cams[0]
    g = sphere(cam, np.asarray(cam[2])[:3], 20.0, W, H)
    side = np.zeros((H, W), bool)
    side[:, 17:] = True
    side[9:, :] ^= True                                    # a corner as well: taps across it in both directions
    if edge == "depth":
        g["depth"] = np.where(side, g["depth"] * np.float32(1.5), g["depth"])     # far beyond depth_tol from either side
    else:
        g["normal"] = np.where(side[..., None], -g["normal"], g["normal"])
    t = TW.temporal_of(cam, depth_tol=0.05, normal_min=0.9)
    # the depth is the distance along the ray, so under the same camera Zexp is the pixel's own depth on either side
    h1 = T.temporal(L, cam, grey(1.0), g, None, t)[0]
    det = T.temporal(L, cam, grey(1.0), g, h1, t, details=True)[3]
    x0, y0 = np.floor(det[..., 0]).astype(int), np.floor(det[..., 1]).astype(int)
    ys, xs = np.mgrid[0:H, 0:W]
    assert (np.abs(x0 - xs) <= 1).all() and (np.abs(y0 - ys) <= 1).all()
    crossed = 0
    for k in range(4):
        qx, qy = x0 + (k & 1), y0 + (k >> 1)
        inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        want = inside & (side[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)] == side)
        assert np.array_equal(det[..., 3 + k] != 0, want), f"tap {k}"
        crossed += int((inside & ~want).sum())
    assert crossed > 50


# ---- leaving the previous image -----------------------------------------------------------------------------------------------------
def test_a_yaw_past_the_border_and_a_camera_facing_away_start_again(L, V, cams):
    pose = TW.poses("room")[0]
    cam = cams[0]
    centre = np.asarray(cam[2])[:3]
    g = sphere(cam, centre, 20.0, W, H)
    for dyaw, dpitch in ((12.0, 0.0), (-12.0, 0.0), (0.0, 9.0), (0.0, -9.0)):
        prev = TW.camera(V, (pose[0], pose[1], pose[2], pose[3] + dyaw, pose[4] + dpitch), (W, H))
        t = TW.temporal_of(prev)
        h1 = T.temporal(L, prev, grey(1.0), sphere(prev, centre, 20.0, W, H), None, t)[0]
        h2 = T.temporal(L, cam, grey(1.0), g, h1, t)[0]
        fx, fy, _, _ = T.position64(cam, g, t)
        out = (fx.v < -1 - fx.e) | (fx.v > W + fx.e) | (fy.v < -1 - fy.e) | (fy.v > H + fy.e)
        inside = (fx.v > 0.5) & (fx.v < W - 1.5) & (fy.v > 0.5) & (fy.v < H - 1.5)
        assert out.sum() > W and inside.sum() > W
        assert (h2[0, ..., 3][out] == 1).all() and (h2[0, ..., 3][inside] == 2).all()
    away = TW.camera(V, (pose[0], pose[1], pose[2], pose[3] + 180.0, -pose[4]), (W, H))
    t = TW.temporal_of(away)
    h1 = T.temporal(L, away, grey(1.0), sphere(away, centre, 20.0, W, H), None, t)[0]
    h2, _, _, det = T.temporal(L, cam, grey(1.0), g, h1, t, details=True)
    assert (h2[0, ..., 3] == 1).all() and not det.any(), "clip.w <= 0: T2 ends at once"


# ---- the parameters -----------------------------------------------------------------------------------------------------------------
def test_max_history_and_the_two_alphas_bind_where_they_should(L, cams):
    cam = cams[0]
    g = sphere(cam, np.asarray(cam[2])[:3], 20.0, W, H)

    def run(frames, **kw):
        hist, t = None, TW.temporal_of(cam, **kw)
        for k in range(frames):
            hist, out, var = T.temporal(L, cam, grey(1.0 if k < frames - 1 else 2.0), g, hist, t)
        return hist, out

    hist, out = run(6, max_history=4, alpha_min=0.0, alpha_moments_min=0.0)
    assert (hist[0, ..., 3] == 4).all()                                   # N' stops at the cap ...
    assert np.abs(out - 1.25).max() <= 1e-5                                # ... and a = 1 / 4 from there on
    hist, out = run(6, max_history=64, alpha_min=0.5, alpha_moments_min=0.0)
    assert np.abs(hist[0, ..., 3] - 6).max() <= 1e-4
    assert np.abs(out - 1.5).max() <= 1e-5                                 # a = alpha_min, not 1 / 6 ...
    assert np.abs(hist[1, ..., 0] - (1 + 1 / 6)).max() <= 1e-5             # ... while the moments still take 1 / 6
    hist, out = run(6, max_history=64, alpha_min=0.0, alpha_moments_min=0.5)
    assert np.abs(out - (1 + 1 / 6)).max() <= 1e-5 and np.abs(hist[1, ..., 0] - 1.5).max() <= 1e-5
    assert np.abs(hist[1, ..., 1] - 2.5).max() <= 1e-5
    hist, out = run(3, max_history=1)
    assert (hist[0, ..., 3] == 1).all() and (out == 2).all()               # a history of one frame is no history


def test_normal_min_and_depth_tol_decide_the_taps(L, cams):
    cam = cams[0]
    g = sphere(cam, np.asarray(cam[2])[:3], 20.0, W, H)
    tilted = dict(g, normal=(g["normal"] * np.float32(0.8)))                # n . n' = 0.8 against the history's unit normals
    deeper = dict(g, depth=g["depth"] * np.float32(1.04))
    h1 = T.temporal(L, cam, grey(1.0), g, None, TW.temporal_of(cam))[0]
    for planes, kw, found in ((tilted, dict(normal_min=0.9), False), (tilted, dict(normal_min=0.7), True),
                              (deeper, dict(depth_tol=0.03), False), (deeper, dict(depth_tol=0.05), True)):
        h2 = T.temporal(L, cam, grey(1.0), planes, h1, TW.temporal_of(cam, **kw))[0]
        assert (h2[0, ..., 3] == (2 if found else 1)).all(), kw


# ---- bad inputs ---------------------------------------------------------------------------------------------------------------------
def test_nan_inf_and_negative_entries_come_out_finite(L, cams):
    rng = np.random.default_rng(7)
    rgb, g = random_planes(rng, H, W)
    bad = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0, 1e30], np.float32)
    for a in (rgb, g["normal"], g["depth"], g["coverage"]):
        m = rng.random(a.shape) < 0.08
        a[m] = bad[rng.integers(0, len(bad), int(m.sum()))]
    hist = random_history(rng, H, W)
    for cam_prev in (cams[0], cams[1]):
        h2, out, var, det = T.temporal(L, cams[0], rgb, g, hist, TW.temporal_of(cam_prev, depth_tol=0.5, normal_min=-1.0), details=True)
        assert det[..., 3:7].any()
        for a in (h2, out, var):
            assert np.isfinite(a).all() and (a[..., :3] >= 0).all() if a is out else np.isfinite(a).all()
        assert (h2[0] >= 0).all() and (h2[1, ..., :2] >= 0).all() and (var >= 0).all() and (h2[0, ..., 3] <= 32).all()


# ---- the float64 restatement on real frames -----------------------------------------------------------------------------------------
_planes = {}


def real_planes(LG, V, O, name, i, size=(GW.W, GW.H)):
    """the checker's guide planes of pose i of `name` (corner rays, two samples), computed once"""
    if (name, i, size) not in _planes:
        w = GW.world(V, name)
        tex, dim = w.flatten()
        w.close()
        cam = TW.camera(V, TW.poses(name)[i], size)
        _planes[name, i, size] = (cam, G.planes(LG, O.make_scene(tex, dim, *cam), size[0], size[1], GW.FIRST, 2)[0])
    return _planes[name, i, size]


STRICT = dict(normal_min=0.9, depth_tol=0.05, alpha_min=0.1, alpha_moments_min=0.2, max_history=32)   # SVGF's neighbourhood


def check_against_float64(L, cam_prev, g_prev, cam, g, plant=None, seed=0, **kw):
    """-> the share of pixels left out. Stage one: fx, fy and Zexp within position64's bounds wherever T2 was reached for certain.
    Stage two: every history word and the variance within integrate64's bounds wherever no decision lies inside its own bound."""
    h, w = g["depth"].shape
    rng = np.random.default_rng(seed)
    rgb = (rng.random((h, w, 3)) * 4).astype(np.float32)
    t = TW.temporal_of(cam_prev, **kw)
    hist = T.temporal(L, cam_prev, (rng.random((h, w, 3)) * 4).astype(np.float32), g_prev, None, t)[0]
    # histories of many lengths, some of none (N = 0: never a tap); none of 1, whose N' is 2.0f exactly and which the N' >= 2
    # decision of the restatement, knowing only the bound, would have to leave out
    hist[0, ..., 3] = rng.integers(2, 12, (h, w)) * (hist[0, ..., 3] > 0) * (rng.random((h, w)) > 0.05)
    h2, out, var, det = T.temporal(L, cam, rgb, g, hist, t, plant=plant, details=True)
    fx, fy, zexp, reached = T.position64(cam, g, t)
    live = F.g_of(g["coverage"]) > 0
    sure = live & reached
    assert sure.sum() > 0.5 * live.sum()
    for got, want, name in ((det[..., 0], fx, "fx"), (det[..., 1], fy, "fy"), (det[..., 2], zexp, "Zexp")):
        worst = (np.abs(got - want.v) / (1.1 * want.e + 1e-30))[sure].max()
        assert worst <= 1.0, f"{name}: {worst:.2f} of its bound"
    w64, v64, bw, bv, unsure = T.integrate64(rgb, g, hist, t, det)
    keep = ~unsure
    assert (np.abs(h2 - w64) <= bw)[:, keep].all(), "history"
    assert (np.abs(out - w64[0, ..., :3]) <= bw[0, ..., :3])[keep].all(), "out_rgb"
    assert (np.abs(var - v64) <= bv)[keep].all(), "variance"
    assert (h2[0, ..., 3] >= 2)[live].mean() > 0.3, "most pixels keep a history"
    return float(unsure[live].mean())


@pytest.mark.parametrize("name", ["room", "lamp", "outside"])
def test_the_checker_is_its_float64_restatement_on_real_frames(L, LG, V, O, name):
    """from each pose to the next, and back to the first: a yaw of a few degrees, a translation of a fraction of a voxel, both"""
    shares = []
    for i, j in ((0, 1), (1, 2), (2, 0), (1, 1)):
        cam_prev, g_prev = real_planes(LG, V, O, name, i)
        cam, g = real_planes(LG, V, O, name, j)
        shares.append(check_against_float64(L, cam_prev, g_prev, cam, g, seed=10 * i + j, **(STRICT if (i + j) % 2 else {})))   # STRICT, or the defaults
    print(f"{name}: share of live pixels left out per step {['%.4f' % s for s in shares]}")
    assert max(shares) <= 0.02, shares


# ---- planted misreadings ------------------------------------------------------------------------------------------------------------
def test_planted_misreadings_are_caught(L, LG, V, O, cams):
    with pytest.raises(AssertionError):
        check_identical_camera(L, cams[0], (0.5, 0.5), plant="offset_kept")
    with pytest.raises(AssertionError):
        check_constant_image(L, V, plant="not_renormalised")
    cam_prev, g_prev = real_planes(LG, V, O, "room", 1)
    cam, g = real_planes(LG, V, O, "room", 2)
    with pytest.raises(AssertionError, match="Zexp"):
        check_against_float64(L, cam_prev, g_prev, cam, g, plant="zexp_from_current_eye")
    with pytest.raises(AssertionError, match="variance"):
        check_alternating_values(L, cams[0], plant="variance_of_one_sample")
    for plant in ("not_renormalised", "variance_of_one_sample"):        # ... and the float64 restatement sees these two as well
        with pytest.raises(AssertionError):
            check_against_float64(L, cam_prev, g_prev, cam, g, plant=plant)


# ---- what needs no device -----------------------------------------------------------------------------------------------------------
def test_the_defaults_and_the_struct(V):
    d = V.default_temporal()
    assert set(d) == set(V.TEMPORAL_KEYS) and d["offset_x"] == d["offset_y"] == 0.0 and 1 <= d["max_history"] <= 32768
    assert 0 <= d["alpha_min"] <= 1 and 0 <= d["alpha_moments_min"] <= 1 and -1 <= d["normal_min"] <= 1 and d["depth_tol"] > 0
    t = V.Temporal()
    t.prev_view_proj[0] = 5.0
    V.hip_lib().vrt_temporal_default(C.byref(t))
    assert not any(t.prev_view_proj) and not any(t.prev_camera_pos), "the matrices are zeroed: the caller fills them"
    assert C.sizeof(V.Temporal) == C.sizeof(T.Temporal) == 108
    made = T.make(**{k: v for k, v in d.items() if k not in ("offset_x", "offset_y")})
    for k in V.TEMPORAL_KEYS:
        assert getattr(made, k) == getattr(t, k), k                             # the checker's defaults are the library's
    assert V.HISTORY_BYTES == 4 * T.HISTORY_FLOATS
