"""The guided filter's checker (tests/oracle_filter_hdr.c) on the CPU: levels = 0, the B3 kernel on equal guides, the checker against
a float64 restatement of the whole rule, edge stopping against closed forms, four planted misreadings those closed forms catch, the
quality measurement against a 256-sample reference, and the validation that needs no device."""
import ctypes as C

import numpy as np
import pytest

import filter_quality as Q
import oracle_filter_hdr as F
import oracle_guides
import oracle_hdr

EPS = F.EPS


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return F.build(tmp_path_factory.mktemp("oracle_filter_hdr"))


def flat_guides(h, w, normal=(0.0, 1.0, 0.0), albedo=(0.5, 0.25, 0.75, 1.0), depth=64.0, coverage=1.0):
    """the same guides everywhere: every edge term is 0"""
    return {"normal": np.broadcast_to(np.array(normal, np.float32), (h, w, 3)).copy(),
            "albedo": np.broadcast_to(np.array(albedo, np.float32), (h, w, 4)).copy(),
            "depth": np.full((h, w), depth, np.float32), "coverage": np.full((h, w), coverage, np.float32)}


def random_case(rng, h, w, negative_depth=False):
    """random planes with structure (a few normals and albedos, a slanted depth with steps), dead blocks, and NaN, Inf and negative
    entries in colour and guides. A negative depth on a live pixel makes den cancel: bit-exact comparisons take it, bounds do not."""
    normals = np.array([[0, 1, 0], [1, 0, 0], [0, 0, -1], [0.6, 0.8, 0]], np.float32)
    albedos = rng.random((4, 4)).astype(np.float32)
    albedos[:, 3] = [1.0, 1.0, 0.5, 1.0]
    kind = rng.integers(0, 4, (h // 6 + 1, w // 6 + 1)).repeat(6, axis=0).repeat(6, axis=1)[:h, :w]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    g = {"normal": (normals[kind] + rng.normal(0, 0.05, (h, w, 3))).astype(np.float32),
         "albedo": np.clip(albedos[kind] + rng.normal(0, 0.02, (h, w, 4)), 0, 1).astype(np.float32),
         "depth": (40.0 + 0.5 * xx + 0.25 * yy + 12.0 * kind + rng.random((h, w))).astype(np.float32),
         "coverage": np.where(rng.random((h, w)) < 0.7, 1.0, rng.random((h, w))).astype(np.float32)}
    rgb = (rng.random((h, w, 3)) ** 4 * 20.0).astype(np.float32)
    g["coverage"][rng.random((h, w)) < 0.1] = 0.0                                    # dead pixels, singly ...
    g["coverage"][2:9, 3:11] = 0.0                                                   # ... and a dead block
    bad = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0], np.float32)
    for a in (rgb, g["normal"], g["albedo"], g["coverage"]):
        m = rng.random(a.shape) < 0.03
        a[m] = bad[rng.integers(0, len(bad), int(m.sum()))]
    m = rng.random((h, w)) < 0.03
    g["depth"][m] = np.array([np.nan, np.inf], np.float32)[rng.integers(0, 2, int(m.sum()))]   # -> 0 and 65504
    g["coverage"][5, 6], rgb[5, 6] = 1.0, (2.0, 3.0, 4.0)                            # inside the block: no live tap but itself at step 1
    dead = ~(F.g_of(g["coverage"]) > 0)
    g["depth"][dead & (rng.random((h, w)) < 0.5)] = -7.0                             # negative where nobody reads it
    if negative_depth:
        g["depth"][rng.random((h, w)) < 0.03] = -5.0
    return rgb, g


# ---- levels = 0 --------------------------------------------------------------------------------------------------------------------
def test_levels_0_is_h_of_c(L):
    rgb, g = random_case(np.random.default_rng(1), 29, 37)
    out, out8 = F.filter(L, rgb, g, F.make(0, demodulate=False))
    F.same(out, F.h_of(rgb), "levels 0, no demodulation")
    F.same(out8, oracle_hdr.tonemap(L, F.h_of(rgb)), "its bytes")
    # with demodulation: h(c) / m * m, two roundings (EPS each, first order; 2^-148 covers a subnormal quotient times m <= 2)
    g["albedo"] = F.g_of(np.clip(np.nan_to_num(g["albedo"], nan=0.0), 0, 1))
    g["coverage"] = F.g_of(np.clip(np.nan_to_num(g["coverage"], nan=0.0), 0, 1))
    out, _ = F.filter(L, rgb, g, F.make(0, demodulate=True))
    hc = F.h_of(rgb).astype(np.float64)
    assert (np.abs(out - hc) <= 2.01 * EPS * hc + 2.0 ** -148).all()
    live = g["coverage"] > 0
    assert (out != F.h_of(rgb))[live].any()                                          # the two roundings do show
    F.same(out[~live], F.h_of(rgb)[~live], "pixels that are not live yield h(c)")


# ---- equal guides: the B3 kernel ---------------------------------------------------------------------------------------------------
def test_impulse_gives_the_separable_b3_product_per_level(L):
    """65 x 65, an impulse at the centre, 3 levels: the impulse's support after level i stays 18 pixels clear of the border, so no tap
    that matters is outside and sumw is exactly 1. Each level is the dilated B3 (x) B3 convolution; against float64 the float32 error
    is one rounding per product and 24 per sum (the first addition is to 0): 25 EPS per level, first order, of a sum of terms >= 0."""
    n, levels = 65, 3
    rgb = np.zeros((n, n, 3), np.float32)
    rgb[32, 32] = (3.0, 0.7, 11.0)
    _, _, lv = F.filter(L, rgb, flat_guides(n, n), F.make(levels, demodulate=False), levels_out=True)
    want = rgb.astype(np.float64)
    for i in range(levels):
        s = 1 << i
        rows = sum(F.B3[o + 2] * np.roll(want, s * o, axis=0) for o in range(-2, 3))
        want = sum(F.B3[o + 2] * np.roll(rows, s * o, axis=1) for o in range(-2, 3))
        assert (np.abs(lv[i] - want) <= 1.01 * 25 * (i + 1) * EPS * want).all(), i
        assert np.count_nonzero(want[..., 0]) == (4 * (2 ** (i + 1) - 1) + 1) ** 2 and want[32, 32, 0] < rgb[32, 32, 0]
        assert abs(want[..., 2].sum() - 11.0) < 1e-12                              # the kernel sums to 1


def test_constant_image_stays_constant(L):
    """Every weight is a B product: multiples of 1/256 whose partial sums are exact, so sumw is exact (1 inside, less at the border).
    sum = 25 products w * c (one rounding each) added one by one (24 roundings), then one division: the result is c within
    26 EPS per level, first order."""
    h, w, levels = 29, 37, 4
    c = np.array([0.1, 7.3, 1234.567], np.float32)
    rgb = np.broadcast_to(c, (h, w, 3)).copy()
    for demod in (False, True):
        out, _ = F.filter(L, rgb, flat_guides(h, w), F.make(levels, demodulate=demod))
        ends = 6 if demod else 0                                                     # m: 2, h(c) / m: 1, u * m: 1 + m's 2
        assert (np.abs(out - c) <= 1.01 * (26 * levels + ends) * EPS * c).all()


# ---- the whole rule against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,demod", [(1, True), (3, False), (3, True), (5, True)])
def test_checker_against_float64(L, levels, demod):
    """random 37 x 29 planes with dead pixels, NaN, Inf and negative inputs; the bound is oracle_filter_hdr.rel_bound()"""
    rgb, g = random_case(np.random.default_rng(7 + levels), 29, 37)
    f = F.make(levels, demod, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=1.0)
    got, _ = F.filter(L, rgb, g, f)
    want = F.filter64(rgb, g, f)
    assert np.isfinite(got).all() and (got >= 0).all()
    err = np.abs(got - want)
    assert (err <= F.rel_bound(levels) * want + 1e-30).all(), float((err / np.maximum(want, 1e-30)).max())
    live = F.g_of(g["coverage"]) > 0
    F.same(got[~live], F.h_of(rgb)[~live], "dead pixels")
    assert (np.abs(got - F.h_of(rgb))[live] > 1e-3).mean() > 0.5                      # the filter did something
    alone, _ = F.filter(L, rgb, g, F.make(1, False))                                 # no live tap but itself: (9/64 u) / (9/64)
    assert (np.abs(alone[5, 6] - rgb[5, 6]) <= 2.01 * EPS * rgb[5, 6]).all()


# ---- edge stopping -----------------------------------------------------------------------------------------------------------------
H1, W1, X0 = 9, 16, 8          # two half planes: columns < X0 and >= X0; rows are all alike


def _halves(left, right, key):
    g = flat_guides(H1, W1)
    g[key][:, :X0] = np.array(left, np.float32)
    g[key][:, X0:] = np.array(right, np.float32)
    rgb = np.zeros((H1, W1, 3), np.float32)
    rgb[:, :X0] = 1.0                                                               # 1 on the left, 0 on the right
    return rgb, g


def _leak_closed_form(k):
    """Level 0 at the left column next to the edge (x = X0 - 1), away from the image's sides: the column weights B3 put 3/8 + 1/4 +
    1/16 = 11/16 on the left and 1/4 + 1/16 = 5/16 across, the rows factor out, every tap across has weight k: the share that
    leaks is k * (5/16) / (11/16 + k * 5/16)"""
    return k * (5 / 16) / (11 / 16 + k * (5 / 16))


def _check_step(L, rgb, g, f, k, plant=None):
    out, _ = F.filter(L, rgb, g, f, plant=plant)
    leak = 1.0 - out[H1 // 2, X0 - 1].astype(np.float64)
    assert (np.abs(leak - _leak_closed_form(k)) <= 1e-6).all(), (leak, _leak_closed_form(k))
    assert (leak <= k).all()
    gain = out[H1 // 2, X0].astype(np.float64)                                       # and the right side gains the mirror share
    assert (np.abs(gain - _leak_closed_form(k)) <= 1e-6).all()


def test_a_normal_step_leaks_its_closed_form_share(L):
    rgb, g = _halves((0, 1, 0), (1, 0, 0), "normal")
    for sn in (0.5, 1.0, 2.0):
        _check_step(L, rgb, g, F.make(1, False, sigma_normal=sn), np.exp(-2.0 / sn ** 2))


def test_an_albedo_step_leaks_its_closed_form_share(L):
    rgb, g = _halves((0.5, 0.25, 0.75, 1.0), (0.5, 0.5, 0.75, 1.0), "albedo")        # G differs by 1/4
    for sa in (0.125, 0.25):
        _check_step(L, rgb, g, F.make(1, False, sigma_albedo=sa), np.exp(-0.0625 / sa ** 2))
    rgb, g = _halves((0.5, 0.25, 0.75, 1.0), (0.5, 0.25, 0.75, 0.5), "albedo")       # glass beside opaque: alpha alone
    _check_step(L, rgb, g, F.make(1, False, sigma_albedo=0.25), np.exp(-4.0))


def test_planted_alpha_left_out_is_caught(L):
    rgb, g = _halves((0.5, 0.25, 0.75, 1.0), (0.5, 0.25, 0.75, 0.5), "albedo")
    with pytest.raises(AssertionError):
        _check_step(L, rgb, g, F.make(1, False, sigma_albedo=0.25), np.exp(-4.0), plant="no_alpha")


# a slanted plane with a step: Z = Z0 + A * x, plus D from column X0 on; rows all alike, so the rows factor out of every level and the
# rule is the 1-D one below
Z0, SLOPE, STEP = 64.0, 0.25, 2.0


def _slanted():
    g = flat_guides(H1, W1)
    x = np.arange(W1, dtype=np.float64)
    z = Z0 + SLOPE * x + np.where(x >= X0, STEP, 0.0)
    g["depth"][:] = z.astype(np.float32)                                             # quarters: exact in float32
    rgb = np.zeros((H1, W1, 3), np.float32)
    rgb[:, :X0] = 1.0
    return rgb, g, z


def _slanted_closed_form(z, sd, levels):
    """float64, one row: every pixel's slope is SLOPE (the one-sided minimum, also next to the step; the image's two end columns have
    one neighbour, on their own side of the step), gy = 0, and u'(x) = sum_ox B[ox] k u(x + s ox) / sum_ox B[ox] k with
    k = exp(-|Z(x + s ox) - Z(x)| / (sd * (SLOPE * |ox| * s + Z(x) / 256) + 2^-20))"""
    u = np.where(np.arange(W1) < X0, 1.0, 0.0)
    for i in range(levels):
        s = 1 << i
        v = np.zeros(W1)
        for x in range(W1):
            num = den = 0.0
            for ox in range(-2, 3):
                t = x + s * ox
                if 0 <= t < W1:
                    k = F.B3[ox + 2] * np.exp(-abs(z[t] - z[x]) / (sd * (SLOPE * abs(ox) * s + z[x] / 256.0) + 2.0 ** -20))
                    num, den = num + k * u[t], den + k
            v[x] = num / den
        u = v
    return u


def _check_slanted(L, levels, plant=None):
    rgb, g, z = _slanted()
    sd = 1.0
    out, _ = F.filter(L, rgb, g, F.make(levels, False, sigma_depth=sd), plant=plant)
    want = _slanted_closed_form(z, sd, levels)
    for y in (0, H1 // 2, H1 - 1):
        assert (np.abs(out[y, :, 0] - want) <= 1e-5).all(), (levels, y, out[y, :, 0], want)
    return out, want


def test_a_depth_step_on_a_slanted_plane(L):
    """taps along the plane keep most of their B x B weight -- e = dzq / den stays below 1 / sigma_depth however far the tap -- and
    taps across the step do not: at level 0 the tap next door has dzq = 2.25 against den = 0.25 + 63.75 / 256 + 2^-20, e = 4.5"""
    out, want = _check_slanted(L, 1)
    x = X0 - 1
    k_across = np.exp(-(STEP + SLOPE) / (SLOPE + (Z0 + SLOPE * x) / 256.0 + 2.0 ** -20))
    assert 1.0 - want[x] <= k_across and k_across < 0.012
    # on the plane alone (no step in reach) the colour is untouched whatever the weights are, and the weights are not small
    assert abs(out[H1 // 2, 2, 0] - 1.0) <= 4 * EPS and np.exp(-2 * SLOPE / (2 * SLOPE + Z0 / 256.0)) > 0.5
    _check_slanted(L, 2)
    _check_slanted(L, 3)


def test_planted_two_sided_slope_is_caught(L):
    """the maximum takes the step for the slope next to it: den grows ninefold and the step leaks"""
    with pytest.raises(AssertionError):
        _check_slanted(L, 1, plant="slope_max")


def test_planted_step_left_out_of_den_is_caught(L):
    """invisible at level 0 (s = 1); at level 1 the taps two pixels along the plane are held to one pixel's slope"""
    _check_slanted(L, 1, plant="no_step")
    with pytest.raises(AssertionError):
        _check_slanted(L, 2, plant="no_step")


def _sky():
    """a surface of colour 1 left of a dead region (coverage 0) of colour 1000"""
    g = flat_guides(H1, W1)
    g["coverage"][:, X0:] = 0.0
    rgb = np.ones((H1, W1, 3), np.float32)
    rgb[:, X0:] = 1000.0
    return rgb, g


def _check_sky(L, plant=None):
    rgb, g = _sky()
    for levels in (1, 3):
        out, _ = F.filter(L, rgb, g, F.make(levels, False), plant=plant)
        assert (np.abs(out[:, :X0] - 1.0) <= 26 * levels * EPS).all()                # a mean of ones: test_constant_image's bound
        F.same(out[:, X0:], rgb[:, X0:], "sky passes through")


def test_sky_is_never_mixed_into_a_surface(L):
    _check_sky(L)


def test_planted_dead_taps_are_caught(L):
    with pytest.raises(AssertionError):
        _check_sky(L, plant="dead_taps")


# ---- quality -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quality(V, O, L, tmp_path_factory):
    LG = oracle_guides.build(tmp_path_factory.mktemp("oracle_guides"))
    return {n: Q.inputs(V, O, L, LG, n) for n in Q.WORLDS}                           # the reference once per world


@pytest.mark.parametrize("world", Q.WORLDS)
def test_filtered_4_samples_beat_unfiltered_and_the_id_blur(V, L, quality, world):
    """the defaults on the mean of 4 samples, against the mean of 256 other samples (profiles/filter_quality.txt has the figures)"""
    f = F.make(**V.default_filter())
    unfiltered, blur, filtered = Q.errors(L, quality[world], f)
    print(f"{world}: unfiltered {unfiltered:.5f} id-blur {blur:.5f} guided {filtered:.5f}")
    assert filtered < unfiltered
    assert filtered < blur


# ---- validation that needs no device -----------------------------------------------------------------------------------------------
def test_defaults_and_null_context(V):
    lib = V.hip_lib()
    d = V.default_filter()
    assert set(d) == {"levels", "demodulate", "sigma_normal", "sigma_albedo", "sigma_depth"}
    assert 0 <= d["levels"] <= V.FILTER_MAX_LEVELS == F.MAX_LEVELS and all(d[k] > 0 for k in d if k.startswith("sigma"))
    mine = F.make(d["levels"])                                                       # the checker module's defaults are the library's
    assert (mine.flags, mine.sigma_normal, mine.sigma_albedo, mine.sigma_depth) == (
        int(d["demodulate"]), np.float32(d["sigma_normal"]), np.float32(d["sigma_albedo"]), np.float32(d["sigma_depth"]))
    lib.vrt_filter_default(None)                                                     # tolerated
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert lib.vrt_filter_hdr(None, 8, 8, p, p, p, p, p, None, None, p, p, None) == -1
    assert lib.vrt_filter_hdr_host(None, 8, 8, p, p, p, p, p, None, None, p, p) == -1
    assert lib.vrt_accum_resolve_hdr_filtered(None, None, None, p, p) == -1
    assert lib.vrt_accum_resolve_hdr_filtered_device(None, None, None, p, p, None) == -1


@pytest.mark.parametrize("bad", [{"levels": -1}, {"levels": 9}, {"levels": 1.5}, {"levels": True}, {"sigma_normal": 0.0},
                                 {"sigma_albedo": -1.0}, {"sigma_depth": float("nan")}, {"sigma_depth": float("inf")},
                                 {"sigma_normal": 1e39}, {"sigma_albedo": "0.1"}, {"sigma": 1.0}])
def test_the_binding_refuses_a_bad_filter(V, bad):
    with pytest.raises(ValueError):
        V.Context._filter(bad)
    f = V.Context._filter({"levels": 3, "demodulate": False})
    assert (f.levels, f.flags) == (3, 0) and V.Context._filter(None) is None
