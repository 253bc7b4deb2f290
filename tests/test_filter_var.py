"""The variance-guided filter's checker (tests/oracle_filter_var.c) on the CPU: its reduction to the guide-only checker, the two
identities of include/vrt.h, closed forms of the initial variance (V2), of the variance's propagation and of the leak across a
luminance step (V3), the checker against float64 restatements with derived bounds, four planted misreadings those catch, the
quality measurement against a 256-sample reference, and the validation that needs no device."""
import ctypes as C

import numpy as np
import pytest

import filter_quality as Q
import filter_var_quality as QV
import oracle_filter_hdr as F
import oracle_filter_var as FV
import oracle_guides
from test_filter_hdr import flat_guides, random_case

EPS = F.EPS


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return FV.build(tmp_path_factory.mktemp("oracle_filter_var"))


def random_variance(rng, h, w):
    """a plane with every kind of entry: NaN, Inf, negative, -0, 0, huge, and ordinary ones"""
    v = (rng.random((h, w)) ** 2 * 4.0).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0, 0.0, 1e30, 5e9], np.float32)
    m = rng.random((h, w)) < 0.08
    v[m] = bad[rng.integers(0, len(bad), int(m.sum()))]
    return v


# ---- the reduction and the identities ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,demod,plane", [(0, True, False), (1, True, True), (2, False, False), (3, True, False), (5, True, True),
                                                (8, False, True)])
def test_without_the_luminance_term_the_colours_are_the_guide_only_checkers(L, levels, demod, plane):
    rng = np.random.default_rng(100 + levels)
    rgb, g = random_case(rng, 29, 37, negative_depth=True)
    f = FV.make(levels, demod, 0.5, 0.25, 1.0, 2.0)
    var = random_variance(rng, 29, 37) if plane else None
    got = FV.filter(L, rgb, g, f, var, "reinhard", 0.6, plant="no_lum")
    want = F.filter(L, rgb, g, FV.guide_only(f), "reinhard", 0.6)
    F.same(got[0], want[0], "floats")
    F.same(got[1], want[1], "bytes")
    if levels:
        assert (FV.filter(L, rgb, g, f, var, "reinhard", 0.6)[0] != want[0]).any()      # and with it they are not


@pytest.mark.parametrize("levels", [0, 1, 2, 3, 5, 8])
def test_one_colour_without_demodulation_is_the_guide_only_filter(L, levels):
    """dl = 0 at every tap of level 0: e gains +0 there for any colour. A later level sees dl = 0 again where the level before
    reproduced the colour exactly, which it does where every channel is 0 or a power of two: each w * c is then exact, their sum is
    c times sumw's own rounded sums, and the quotient is c. So: any colour up to one level, such a colour at every level count. The
    guides are random, so the weights are not trivial."""
    rng = np.random.default_rng(3)
    rgb, g = random_case(rng, 29, 37)
    live = F.g_of(g["coverage"]) > 0
    for colour in ((0.5, 2.0, 0.125), (0.0, 1.0, 1024.0)) + (((0.7, 2.5, 0.3),) if levels <= 1 else ()):
        rgb[live] = colour
        for var in (None, random_variance(rng, 29, 37)):
            got = FV.filter(L, rgb, g, FV.make(levels, False, 0.5, 0.25, 1.0, 1.0), var)
            want = F.filter(L, rgb, g, F.make(levels, False, 0.5, 0.25, 1.0))
            F.same(got[0], want[0], f"floats, levels {levels}, {colour}")
            F.same(got[1], want[1], f"bytes, levels {levels}, {colour}")


@pytest.mark.parametrize("demod", [False, True])
def test_levels_0_is_the_guide_only_filter_at_levels_0(L, demod):
    rng = np.random.default_rng(4)
    rgb, g = random_case(rng, 29, 37, negative_depth=True)
    for var in (None, random_variance(rng, 29, 37)):
        got = FV.filter(L, rgb, g, FV.make(0, demod), var)
        want = F.filter(L, rgb, g, F.make(0, demod))
        F.same(got[0], want[0], "floats")
        F.same(got[1], want[1], "bytes")


# ---- V2 ----------------------------------------------------------------------------------------------------------------------------
def _grey(y):
    """an image of luminance y (up to Y's own three roundings: the coefficients add up to 1 within 1 EPS)"""
    y = np.asarray(y, np.float32)
    return np.repeat(y[..., None], 3, axis=2)


def test_a_flat_image_has_no_variance(L):
    h, w = 12, 17
    rgb = np.broadcast_to(np.array([0.1, 7.3, 1234.567], np.float32), (h, w, 3)).copy()
    for demod in (False, True):
        out = FV.filter(L, rgb, flat_guides(h, w), FV.make(0, demod), details=True)
        # equal l at every tap, unit weights: m1 = l and m2 = l^2 up to 100 roundings each, v0 their difference (l <= 1234.567 / m, m >= 1/4)
        assert (out[4] <= 4 * 100 * EPS * 1234.567 ** 2).all() and (out[4] >= 0).all()
        assert (out[2] <= 4 * 100 * EPS * 1234.567 ** 2).all()
    zero = FV.filter(L, np.zeros((h, w, 3), np.float32), flat_guides(h, w), FV.make(0, False), details=True)
    assert not zero[4].any() and not zero[2].any()
    ones = FV.filter(L, np.ones((h, w, 3), np.float32) * 0.5, flat_guides(h, w), FV.make(0, False), details=True)
    # l is the same float at every tap, n l and n l^2 (n <= 49, l = 1/2 up to its own rounding) are sums of equal terms
    assert (ones[4] <= 100 * EPS).all()


def test_a_checkerboard_on_one_surface(L):
    """Two values a, b by pixel parity, every guide equal: unit weights. A window of n taps with k of them a has
    v0 = (k / n)(1 - k / n)(a - b)^2. In row 0 the window is 4 rows of 7: 14 and 14, v0 = (a - b)^2 / 4; in the interior it is 7 x 7
    = 49, which no pattern splits evenly: 25 and 24, v0 = (600 / 2401)(a - b)^2. Float rounding: s1, s2 at most 49 products and 48
    additions, two divisions, a square and a difference of numbers below a^2: 110 EPS a^2 covers it."""
    h, w, a, b = 16, 17, 3.0, 1.0
    yy, xx = np.mgrid[0:h, 0:w]
    y = np.where((yy + xx) % 2 == 0, a, b).astype(np.float32)
    v0 = FV.filter(L, _grey(y), flat_guides(h, w), FV.make(0, False), details=True)[4].astype(np.float64)
    tol = 110 * EPS * a * a
    assert abs(v0[0, 8] - (a - b) ** 2 / 4) <= tol and abs(v0[h - 1, 5] - (a - b) ** 2 / 4) <= tol
    assert (np.abs(v0[3:h - 3, 3:w - 3] - 600 / 2401 * (a - b) ** 2) <= tol).all()
    # and the output plane at levels 0 is v0 itself without demodulation
    assert np.array_equal(FV.filter(L, _grey(y), flat_guides(h, w), FV.make(0, False))[2], v0.astype(np.float32))


def test_across_a_normal_edge_the_far_side_counts_for_its_weight(L):
    """Two half planes of normals (0,1,0) and (1,0,0), luminance a left and b right. At a pixel d columns left of the edge, away from
    the image's sides, the window's 7 columns are 3 + d + 1 on its own side (weight 1) and 3 - d across (weight k = exp(-2 kn)):
    with share p = k (3 - d) / ((4 + d) + k (3 - d)) of the far side, v0 = p (1 - p)(a - b)^2 <= k (a - b)^2 (3 - d) / (4 + d)."""
    h, w, x0, a, b = 16, 20, 10, 2.0, 0.5
    g = flat_guides(h, w)
    g["normal"][:, x0:] = (1.0, 0.0, 0.0)
    y = np.where(np.arange(w) < x0, a, b).astype(np.float32)[None, :].repeat(h, axis=0)
    for sn in (0.5, 1.0, 2.0):
        v0 = FV.filter(L, _grey(y), g, FV.make(0, False, sigma_normal=sn), details=True)[4].astype(np.float64)
        k = np.exp(-2.0 / sn ** 2)
        for d in (0, 1, 2):
            p = k * (3 - d) / ((4 + d) + k * (3 - d))
            assert abs(v0[h // 2, x0 - 1 - d] - p * (1 - p) * (a - b) ** 2) <= 1e-5 * (a - b) ** 2, (sn, d)
            assert v0[h // 2, x0 - 1 - d] <= k * (a - b) ** 2 * (3 - d) / (4 + d) * (1 + 1e-5)
        assert v0[h // 2, x0 - 4] <= 110 * EPS * a * a                                    # out of reach: flat


# ---- V3 ----------------------------------------------------------------------------------------------------------------------------
SB2 = 9 / 64 + 2 / 16 + 2 / 256            # sum of B^2 over -2..2
SB2_CORNER = 9 / 64 + 1 / 16 + 1 / 256     # ... over 0..2
SB_CORNER = 3 / 8 + 1 / 4 + 1 / 16         # sum of B over 0..2


def _propagation(L, plant=None):
    """one colour, equal guides, a constant variance plane v: every weight is its B product and dl = 0, so
    v' = v sum(B^2 x B^2) / (sum B x B)^2 over the taps present: v SB2^2 in the interior, v (SB2_CORNER / SB_CORNER^2)^2 in a corner.
    Float rounding: 25 products of two and 24 additions, a square and a division: 80 EPS."""
    h, w, v = 12, 13, 0.75
    rgb = np.broadcast_to(np.array([0.5, 1.5, 0.25], np.float32), (h, w, 3)).copy()
    out = FV.filter(L, rgb, flat_guides(h, w), FV.make(1, False), np.full((h, w), v, np.float32), plant=plant)[2].astype(np.float64)
    assert abs(out[h // 2, w // 2] - v * SB2 ** 2) <= 80 * EPS * v
    for cy, cx in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        assert abs(out[cy, cx] - v * (SB2_CORNER / SB_CORNER ** 2) ** 2) <= 80 * EPS * v


def test_the_variance_propagates_with_the_squared_weights(L):
    _propagation(L)


def test_planted_weight_not_squared_is_caught(L):
    with pytest.raises(AssertionError):
        _propagation(L, plant="w_not_squared")


H1, W1, X0 = 9, 16, 8          # two half planes as tests/test_filter_hdr.py has them: columns < X0 and >= X0


def _leak(k):
    """test_filter_hdr._leak_closed_form: the share that crosses when every tap across has weight k"""
    return k * (5 / 16) / (11 / 16 + k * (5 / 16))


def _luminance_step(L, a, b, v, sigma_lum, plant=None):
    """One plane, luminance a left and b right, variance v everywhere, no demodulation: at the column next to the edge vbar = v and
    every tap across has k = exp(-|a - b| / (sigma_lum sqrt(v) + 2^-20)); the colour there is a - leak (a - b)."""
    y = np.where(np.arange(W1) < X0, a, b).astype(np.float32)[None, :].repeat(H1, axis=0)
    out = FV.filter(L, _grey(y), flat_guides(H1, W1), FV.make(1, False, sigma_lum=sigma_lum), np.full((H1, W1), v, np.float32), plant=plant)[0]
    k = np.exp(-abs(a - b) / (sigma_lum * np.sqrt(v) + 2.0 ** -20))
    assert (np.abs(out[H1 // 2, X0 - 1].astype(np.float64) - (a - _leak(k) * (a - b))) <= 2e-6 * max(a, b)).all(), (a, b, v, sigma_lum)
    assert (np.abs(out[H1 // 2, X0].astype(np.float64) - (b + _leak(k) * (a - b))) <= 2e-6 * max(a, b)).all()
    return k


def test_a_luminance_step_leaks_its_closed_form_share(L):
    ks = [_luminance_step(L, a, b, v, sl) for a, b, v, sl in ((1.0, 0.0, 0.25, 1.0), (1.0, 0.5, 0.0625, 4.0), (0.25, 2.0, 1.0, 2.0),
                                                             (1.0, 0.5, 0.0, 4.0), (1.0, 0.5, 0.01, 1e6))]
    assert ks[0] == pytest.approx(np.exp(-2.0), rel=1e-5) and ks[3] == 0.0 and ks[4] > 0.9999       # no variance: a hard edge; huge sigma: none


def _demodulated_step(L, plant=None):
    """The same step seen through demodulation: albedo 1/2 left and 1/4 right (sigma_albedo so large that the albedo term is 1e-7),
    colours chosen so that u is 1 left and 1/2 right, a caller's plane var. m is the albedo (coverage 1), Ym = Y(m): v0 = var / Ym^2 is
    4 var left and 16 var right; at the column next to the edge the 3 x 3 has its right column across: vbar = (3/4) 4 var + (1/4) 16 var
    = 7 var, dl = 1/2 -- of u, not of the colour the caller sees (1/2 against 1/8) -- and the output there is m (1 - leak / 2)."""
    g = flat_guides(H1, W1)
    g["albedo"][:, :X0] = (0.5, 0.5, 0.5, 1.0)
    g["albedo"][:, X0:] = (0.25, 0.25, 0.25, 1.0)
    rgb = np.zeros((H1, W1, 3), np.float32)
    rgb[:, :X0], rgb[:, X0:] = 0.5, 0.125
    var, sl = 0.01, 2.0
    out, _, outv, _, v0 = FV.filter(L, rgb, g, FV.make(1, True, sigma_albedo=1000.0, sigma_lum=sl), np.full((H1, W1), var, np.float32),
                                    plant=plant, details=True)
    assert abs(v0[H1 // 2, 2] - 4 * var) <= 1e-6 and abs(v0[H1 // 2, W1 - 3] - 16 * var) <= 1e-6
    k = np.exp(-0.5 / (sl * np.sqrt(7 * var) + 2.0 ** -20))
    assert (np.abs(out[H1 // 2, X0 - 1].astype(np.float64) - 0.5 * (1 - _leak(k) / 2)) <= 2e-6).all(), (out[H1 // 2, X0 - 1], k)
    # far from the edge the variance comes back re-modulated: var sum(B^2)^2, since 4 var Ym^2 = var
    assert abs(outv[H1 // 2, 2] - var * SB2 ** 2) <= 1e-6 * var


def test_a_demodulated_luminance_step(L):
    _demodulated_step(L)


def test_planted_dl_of_the_remodulated_colour_is_caught(L):
    with pytest.raises(AssertionError):
        _demodulated_step(L, plant="dl_remodulated")


def test_planted_ym_forgotten_is_caught(L):
    with pytest.raises(AssertionError):
        _demodulated_step(L, plant="no_ym")


def test_a_callers_plane_comes_back_at_levels_0(L):
    """hv(hv(var) / Ym^2 * Ym^2): two roundings; pixels that are not live yield +0"""
    rng = np.random.default_rng(9)
    rgb, g = random_case(rng, 29, 37)
    g["albedo"] = F.g_of(np.clip(np.nan_to_num(g["albedo"], nan=0.0), 0, 1))
    g["coverage"] = F.g_of(np.clip(np.nan_to_num(g["coverage"], nan=0.0), 0, 1))
    var = random_variance(rng, 29, 37)
    live = g["coverage"] > 0
    want = FV.hv_of(var).astype(np.float64)
    for demod in (False, True):
        out = FV.filter(L, rgb, g, FV.make(0, demod), var)[2]
        assert (np.abs(out - want)[live] <= 2.01 * EPS * want[live]).all()
        assert not out[~live].any() and not np.signbit(out).any()
        if not demod:
            F.same(out[live], FV.hv_of(var)[live], "no demodulation: hv(var) itself")


# ---- the checker against float64 ---------------------------------------------------------------------------------------------------
def _noisy_case(seed, h=29, w=37):
    """random_case's guides with depths >= 0, and an image noisy enough that no pixel's variance is tiny against its luminance"""
    rng = np.random.default_rng(seed)
    rgb, g = random_case(rng, h, w)
    rgb = (0.5 + rng.random((h, w, 3)) * 2.0).astype(np.float32)
    return rng, rgb, g


def test_spatial_estimate_against_float64(L):
    _, rgb, g = _noisy_case(21)
    for demod in (False, True):
        f = FV.make(0, demod, 0.5, 0.25, 1.0)
        v0 = FV.filter(L, rgb, g, f, details=True)[4]
        want, bound = FV.v0_64(FV.prep64(rgb, g, f))
        assert np.isfinite(v0).all() and (np.abs(v0 - want) <= bound + 1e-30).all()
        assert (want[F.g_of(g["coverage"]) > 0] > 0.01).mean() > 0.8                        # and it is an estimate of something


def _levels_against_float64(L, levels, demod, plane, plant=None, seed=30):
    """every level of the checker against level64() on the checker's own inputs of that level, within level64's bound"""
    rng, rgb, g = _noisy_case(seed + levels)
    h, w = rgb.shape[:2]
    var = None
    if plane:                                              # a plane that differs between neighbours: 0.01 or 1 by column parity
        var = np.where(np.arange(w) % 2 == 0, 0.01, 1.0).astype(np.float32)[None, :].repeat(h, axis=0)
    f = FV.make(levels, demod, 0.5, 0.25, 1.0, 2.0)
    out, _, outv, lv, v0 = FV.filter(L, rgb, g, f, var, plant=plant, details=True)
    P = FV.prep64(rgb, g, f)
    u, v = P["u0"], v0.astype(np.float64)
    worst = 0.0
    for i in range(levels):
        wu, wv, bu, bv = FV.level64(P, u, v, 1 << i, f.sigma_lum)
        gu, gv = lv[i, ..., :3].astype(np.float64), lv[i, ..., 3].astype(np.float64)
        assert (np.abs(gu - wu) <= bu).all(), (i, float((np.abs(gu - wu) - bu).max()))
        assert (np.abs(gv - wv) <= bv).all(), (i, float((np.abs(gv - wv) - bv).max()))
        worst = max(worst, float(np.median(bu[P["live"]] / np.maximum(wu[P["live"]], 1e-30))))
        u, v = gu, gv
    assert worst < 1e-4                                    # the bound says something: a median of 1e-4 of the value, not of its size
    live = P["live"]
    want = np.clip(u * P["M"], 0.0, 65504.0)
    assert (np.abs(out - want)[live] <= 3.01 * EPS * want[live]).all()
    wantv = np.clip(v * P["ym2"], 0.0, float(FV.VAR_MAX))
    assert (np.abs(outv - wantv)[live] <= 8.01 * EPS * wantv[live]).all()      # Ym: 2 + 3, its square 2 more, the product 1
    F.same(out[~live], F.h_of(rgb)[~live], "dead pixels")
    assert not outv[~live].any()


@pytest.mark.parametrize("levels,demod,plane", [(1, True, False), (3, False, True), (3, True, False), (5, True, True)])
def test_checker_against_float64(L, levels, demod, plane):
    _levels_against_float64(L, levels, demod, plane)


def test_planted_vbar_at_spacing_1_is_caught(L):
    """invisible at level 0 (s = 1); at level 1 the 3 x 3 must take the variance two columns away, which the 25 taps at step 2 made
    alike within a parity class and different between them"""
    _levels_against_float64(L, 1, True, True, plant="vbar_spacing_1")
    with pytest.raises(AssertionError):
        _levels_against_float64(L, 2, True, True, plant="vbar_spacing_1")


# ---- quality -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quality(V, O, L, tmp_path_factory):
    LG = oracle_guides.build(tmp_path_factory.mktemp("oracle_guides"))
    return {n: QV.inputs(V, O, L, LG, n) for n in Q.WORLDS}                           # the reference once per world


def test_the_defaults_are_no_worse_than_the_guide_only_defaults(V, L, quality):
    """summed over both worlds, both from this run: deterministic CPU arithmetic, no margin"""
    fv, f = FV.make(**V.default_filter_var()), F.make(**V.default_filter())
    var = sum(QV.error(L, quality[n], fv, "spatial") for n in Q.WORLDS)
    guide = sum(QV.error_guide_only(L, quality[n], f) for n in Q.WORLDS)
    print(f"variance-guided defaults {var:.5f} guide-only defaults {guide:.5f}")
    assert var <= guide


@pytest.mark.parametrize("levels", [3, 5])
def test_more_levels_are_better_with_the_luminance_term_than_without(L, quality, levels):
    """the best swept row at this level count against the guide-only filter's best row at the same count (profiles/filter_quality.txt),
    both computed here"""
    rows = QV.sweep(L, quality, levels=(levels,), sigmas=(QV.PARENT_BEST[levels], (0.5, 0.05, 2.0)))
    best, parent = QV.best(rows), QV.parent_best(L, quality, levels)
    print(f"levels {levels}: best {best[0]:.4f} ({best[2]}, sigmas {best[3]}, sigma_lum {best[4]:g}) guide-only best {parent:.4f}")
    assert best[0] < parent
    assert QV.best(rows, source="spatial")[0] < parent


# ---- validation that needs no device -----------------------------------------------------------------------------------------------
def test_defaults_and_null_context(V):
    lib = V.hip_lib()
    d = V.default_filter_var()
    assert set(d) == set(V.default_filter()) | {"sigma_lum"}
    assert 0 <= d["levels"] <= V.FILTER_MAX_LEVELS and all(d[k] > 0 for k in d if k.startswith("sigma"))
    mine = FV.make(d["levels"])                                                      # the checker module's defaults are the library's
    assert (mine.flags, mine.sigma_normal, mine.sigma_albedo, mine.sigma_depth, mine.sigma_lum) == (
        int(d["demodulate"]), np.float32(d["sigma_normal"]), np.float32(d["sigma_albedo"]), np.float32(d["sigma_depth"]), np.float32(d["sigma_lum"]))
    lib.vrt_filter_var_default(None)                                                 # tolerated
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert lib.vrt_filter_hdr_var(None, 8, 8, p, p, p, p, p, p, None, None, p, p, p, None) == -1
    assert lib.vrt_filter_hdr_var_host(None, 8, 8, p, p, p, p, p, p, None, None, p, p, p) == -1
    assert lib.vrt_accum_resolve_hdr_filtered_var(None, None, None, p, p, p) == -1
    assert lib.vrt_accum_resolve_hdr_filtered_var_device(None, None, None, p, p, p, None) == -1


@pytest.mark.parametrize("bad", [{"levels": -1}, {"levels": 9}, {"sigma_lum": 0.0}, {"sigma_lum": -1.0}, {"sigma_lum": float("nan")},
                                 {"sigma_lum": float("inf")}, {"sigma_lum": 1e39}, {"sigma_lum": "4"}, {"sigma_normal": 0.0}, {"sigma": 1.0}])
def test_the_binding_refuses_a_bad_filter(V, bad):
    with pytest.raises(ValueError):
        V.Context._filter_var(bad)
    f = V.Context._filter_var({"levels": 3, "demodulate": False, "sigma_lum": 2.5})
    assert (f.levels, f.flags, f.sigma_lum) == (3, 0, 2.5) and V.Context._filter_var(None) is None
