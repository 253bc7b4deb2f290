"""The guided upsampling pass's checker (tests/oracle_upsample.c) on the CPU: the r = 1 identity against the guided filter's checker,
a constant image, the float32 bilinear interpolation where every guide agrees, a depth step, a normal flip and an alpha step with
their closed-form leaks, sky beside surfaces, pixels no tap serves, min_weight, the borders, demodulation, the checker against its
float64 restatement with derived bounds on the guide planes of real frames and on a depth ramp, four planted misreadings those catch,
and the struct, the defaults and the validation that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import guide_worlds as GW
import oracle_filter_hdr as F
import oracle_guides as G
import oracle_upsample as U
from conftest import ROOT

EPS = F.EPS
f32 = np.float32


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return U.build(tmp_path_factory.mktemp("oracle_upsample"))


@pytest.fixture(scope="module")
def LG(tmp_path_factory):
    return G.build(tmp_path_factory.mktemp("oracle_guides"))


def flat(h, w, depth=10.0, albedo=0.5):
    """one surface: every guide agrees"""
    n = np.zeros((h, w, 3), f32)
    n[..., 2] = 1
    a = np.full((h, w, 4), albedo, f32)
    a[..., 3] = 1
    return {"normal": n, "albedo": a, "depth": np.full((h, w), depth, f32), "coverage": np.ones((h, w), f32)}


def random_planes(rng, h, w, dead=True, bad=0.0):
    """depths of 5-40, axis normals, random albedo, blocks of pixels that are not live, a colour plane; with `bad` that share of
    every plane replaced by NaN, Inf, negative, zero and huge entries"""
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    g = {"normal": axes[rng.integers(0, 6, (h, w))].copy(), "albedo": rng.random((h, w, 4)).astype(f32),
         "depth": (5 + 35 * rng.random((h, w))).astype(f32), "coverage": (0.25 + 0.75 * rng.random((h, w))).astype(f32)}
    if dead:
        for _ in range(3):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            g["coverage"][y:y + 3, x:x + 4] = 0.0
    rgb = (rng.random((h, w, 3)) * 4).astype(f32)
    if bad:
        vals = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0, 0.0, 1e30, 7e4], f32)
        for a in (rgb, *g.values()):
            m = rng.random(a.shape) < bad
            a[m] = vals[rng.integers(0, len(vals), int(m.sum()))]
    return rgb, g


def repeat(g, r):
    """low planes -> the high planes that show the same surfaces: every low pixel r x r times"""
    return {k: np.ascontiguousarray(np.repeat(np.repeat(v, r, axis=0), r, axis=1)) for k, v in g.items()}


# ---- identities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("offset", [(0.0, 0.0), (0.5, 0.5), (1.0, 0.25)])
def test_factor_one_is_the_guided_filter_at_levels_zero(L, demodulate, offset):
    rgb, g = random_planes(np.random.default_rng(11), 19, 35, bad=0.05)
    for op, exposure in (("clamp", 1.0), ("reinhard", 0.7)):
        want = F.filter(L, rgb, g, F.make(0, demodulate), op, exposure)
        got = U.upsample(L, rgb, g, g, U.make(1, demodulate, offset_lo=offset, offset_hi=offset), op, exposure, details=True)
        U.same(got[0], want[0], "out_rgb")
        U.same(got[1], want[1], "out_rgba8")
    ys, xs = np.mgrid[0:19, 0:35]
    assert np.array_equal(got[3][..., 0], xs) and np.array_equal(got[3][..., 1], ys), "fx, fy are the pixel's own"
    clean = np.isfinite(got[3][..., 6])
    assert clean.mean() > 0.6 and (got[3][..., 6][clean] == 1).all() and not got[2][clean].any(), "one tap of weight 1"


def check_constant_image(L, r, min_weight, plant=None):
    """Every channel a power of two: each w * u is exact, a sum is u times sumw's own rounded sums and the quotient u, whatever the
    weights; a pixel no tap serves takes the nearest low pixel's, the same value. Without demodulation m = 1."""
    rng = np.random.default_rng(r)
    _, g = random_planes(rng, 9, 13)
    hi = repeat(g, r)                                          # the same surfaces, another albedo on every high pixel ...
    hi["albedo"] = rng.random((9 * r, 13 * r, 4)).astype(f32)
    g["coverage"][0:2, 0:2] = 0.0                              # ... and a surface where the low image saw sky
    hi["coverage"][0:2 * r, 0:2 * r] = 1.0
    rgb = np.full((9, 13, 3), 4.0, f32)
    out, _, mask, det = U.upsample(L, rgb, g, hi, U.make(r, False, sigma_albedo=2.0, min_weight=min_weight), plant=plant, details=True)
    U.same(out, np.full((9 * r, 13 * r, 3), 4.0, f32), "the image")
    assert mask.any() and not mask.all() and ((det[..., 6] > 0) & (det[..., 6] < 0.9)).any(), "the weights are not trivial"


@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("min_weight", [0.0, 0.25])
def test_a_constant_image_is_returned_exactly(L, r, min_weight):
    check_constant_image(L, r, min_weight)


def check_bilinear(L, r, offset_lo, offset_hi, demodulate, plant=None):
    """e = +0 on every tap, det_expf(-0) = 1: w = b. With albedo 0.5 and coverage 1 m = 0.5 exactly, so u = 2 h(c) and the output
    half the interpolation of u: the interpolation of h(c), exactly."""
    h, w = 7, 11
    rgb = (np.random.default_rng(r).random((h, w, 3)) * 4).astype(f32)
    u = U.make(r, demodulate, offset_lo=offset_lo, offset_hi=offset_hi)
    out, _, mask, det = U.upsample(L, rgb, flat(h, w), flat(h * r, w * r), u, plant=plant, details=True)
    U.same(out, U.bilinear32(rgb, r, offset_lo, offset_hi), f"r {r} offsets {offset_lo} {offset_hi}")
    assert not mask.any()
    assert (det[..., 0] < 0).any() == (offset_lo[0] > 0) and (np.floor(det[..., 0]) + 1 >= w).any(), "border taps on both sides"


@pytest.mark.parametrize("r", [2, 3, 4])
@pytest.mark.parametrize("offsets", [((0.0, 0.0), (0.0, 0.0)), ((0.5, 0.5), (0.0, 0.0)), ((0.5, 0.5), (0.5, 0.5))], ids=["0_0", "0.5_0", "0.5_0.5"])
def test_equal_guides_give_the_float32_bilinear_interpolation(L, r, offsets):
    check_bilinear(L, r, offsets[0], offsets[1], demodulate=r != 3)


def test_the_position_is_exact_for_the_accumulation_forms_offsets(L):
    """U3 for r = 2, 4 and the offsets the accumulation forms use: x / r - 0.5 is exact in float32"""
    for r in (2, 4):
        det = U.upsample(L, np.zeros((3, 5, 3), f32), flat(3, 5), flat(3 * r, 5 * r), U.make(r, offset_lo=(0.5, 0.5)), details=True)[3]
        ys, xs = np.mgrid[0:3 * r, 0:5 * r]
        assert np.array_equal(det[..., 0], xs / r - 0.5) and np.array_equal(det[..., 1], ys / r - 0.5)


# ---- closed forms -------------------------------------------------------------------------------------------------------------------
H0, W0, R0 = 4, 8, 2      # the low frame of the closed forms and their factor; the step lies between low columns 3 and 4


def step_planes(kind):
    """two surfaces side by side that differ in one guide only, the same in both sizes; colours 1 (left) and 3 (right)"""
    g = flat(H0, W0)
    if kind == "depth":
        g["depth"][:, W0 // 2:] = 20.0
    elif kind == "normal":
        g["normal"][:, W0 // 2:, 2] = -1.0
    elif kind == "alpha":
        g["albedo"][:, W0 // 2:, 3] = 0.5
    elif kind == "sky":
        g["coverage"][:, W0 // 2:] = 0.0
    rgb = np.ones((H0, W0, 3), f32)
    rgb[:, W0 // 2:] = 3.0
    return rgb, g, repeat(g, R0)


def step_exponent(kind, u, left):
    """e of a tap across the step seen from a pixel on the left / right, in float64 (the slopes are 0: one-sided minima)"""
    if kind == "depth":
        return 10.0 / (u.sigma_depth * ((10.0 if left else 20.0) / 256.0) + 2.0 ** -20)
    if kind == "normal":
        return 4.0 / float(u.sigma_normal) ** 2
    return 0.25 / float(u.sigma_albedo) ** 2


LEAKY = {"depth": dict(sigma_depth=64.0), "normal": dict(sigma_normal=1.0), "alpha": dict(sigma_albedo=0.25)}      # e about 4
SHARP = {"depth": dict(sigma_depth=2.0), "normal": dict(sigma_normal=0.1), "alpha": dict(sigma_albedo=0.05)}       # e of 100 and more


def check_step(L, kind, plant=None):
    rgb, g, hi = step_planes(kind)
    xs = np.arange(W0 * R0)
    left = xs < W0 * R0 // 2
    side = np.where(left, 1.0, 3.0)
    for kw, sharp in ((SHARP[kind], True), (LEAKY[kind], False)):
        u = U.make(R0, False, **kw)
        out, _, mask, det = U.upsample(L, rgb, g, hi, u, plant=plant, details=True)
        assert not mask.any()
        fx = det[0, :, 0].astype(np.float64)
        x0 = np.floor(fx)
        tx = fx - x0
        want = np.zeros(W0 * R0)
        for x in xs:
            num = den = 0.0
            for X, b in ((int(x0[x]), 1.0 - tx[x]), (int(x0[x]) + 1, tx[x])):
                if 0 <= X < W0:
                    e = 0.0 if (X < W0 // 2) == left[x] else step_exponent(kind, u, left[x])
                    wt = b * (np.exp(-e) if e <= 87.0 else 0.0)
                    num, den = num + wt * (1.0 if X < W0 // 2 else 3.0), den + wt
            want[x] = num / den
        e_max = 0.0 if sharp else max(step_exponent(kind, u, True), step_exponent(kind, u, False))
        tol = 1.05 * (2 * (F.E_EXP + e_max * 9 * EPS + EPS) + 12 * EPS)       # oracle_filter_hdr.rel_bound()'s terms for four taps
        assert (np.abs(out[..., 0] - want[None, :]) <= tol * want[None, :]).all(), f"{kind} {kw}: the closed form"
        if sharp:
            U.same(out[..., 0], np.broadcast_to(side.astype(f32), out.shape[:2]).copy(), f"{kind}: each side takes only its own taps")
        else:
            assert (np.abs(out[..., 0] - side[None, :]) > 1e-3).any(), f"{kind}: the leak is there"


@pytest.mark.parametrize("kind", ["depth", "normal", "alpha"])
def test_a_step_in_one_guide_separates_the_two_sides(L, kind):
    check_step(L, kind)


def check_sky(L, plant=None):
    rgb, g, hi = step_planes("sky")
    for min_weight in (0.0, 0.2):       # the last row's taps have b = 0.25 each: below 0.25 every pixel keeps one of its own side
        out, _, mask = U.upsample(L, rgb, g, hi, U.make(R0, True, min_weight=min_weight), plant=plant)
        want = np.where(np.arange(W0 * R0) < W0 * R0 // 2, f32(1), f32(3))
        U.same(out[..., 0], np.broadcast_to(want, out.shape[:2]).copy(), "sky is never mixed into surfaces, nor surfaces into sky")
        assert not mask.any()


def test_sky_and_surfaces_never_mix(L):
    check_sky(L)


def test_a_live_pixel_with_only_sky_taps_is_flagged_and_takes_the_nearest(L):
    rng = np.random.default_rng(3)
    rgb, g = random_planes(rng, 5, 6, dead=False)
    g["coverage"][:] = 0.0                                   # the low image saw only sky ...
    _, hi = random_planes(rng, 15, 18, dead=False)            # ... every high pixel a surface
    for demodulate in (False, True):
        out, _, mask, det = U.upsample(L, rgb, g, hi, U.make(3, demodulate), details=True)
        assert mask.all() and not det[..., 2:7].any()
        ys, xs = np.mgrid[0:15, 0:18]
        ny, nx = np.clip(np.floor(ys / f32(3) + f32(0.5)), 0, 4).astype(int), np.clip(np.floor(xs / f32(3) + f32(0.5)), 0, 5).astype(int)
        m = np.maximum(hi["albedo"][..., :3] + (f32(1) - hi["coverage"])[..., None], f32(1) / f32(255)) if demodulate else f32(1)
        U.same(out, F.h_of(rgb[ny, nx] * m), "u_N with m_N = 1, times the high pixel's m")
    g["coverage"][1, 2] = 1.0                                 # the reverse: a sky pixel that lies on a low pixel that is a surface
    hi["coverage"][:] = 0.0                                   # (tx = ty = 0: the other three taps have b = 0)
    out, _, mask = U.upsample(L, rgb, g, hi, U.make(3, False))
    assert mask[3, 6] and not mask[4, 7] and not mask[0, 0]
    U.same(out[3, 6], rgb[1, 2], "the nearest low pixel, whatever its liveness")


def test_min_weight_binds_where_it_should(L):
    """low pixels right of column 3 and below row 1 are sky, every high pixel a surface: high (7, 3) has one live tap of b = 0.25,
    high (7, 2) one of b = 0.5"""
    g = flat(H0, W0)
    g["coverage"][:, 4:] = 0.0
    g["coverage"][2:, :] = 0.0
    rgb = (np.random.default_rng(4).random((H0, W0, 3)) * 4).astype(f32)
    hi = flat(H0 * R0, W0 * R0)
    for min_weight, flagged in ((0.0, (False, False)), (0.25, (True, False)), (0.5, (True, True))):
        out, _, mask, det = U.upsample(L, rgb, g, hi, U.make(R0, False, min_weight=min_weight), details=True)
        assert det[3, 7, 6] == 0.25 and det[2, 7, 6] == 0.5
        assert (bool(mask[3, 7]), bool(mask[2, 7])) == flagged, min_weight
        U.same(out[2, 7], rgb[1, 3] if not flagged[1] else rgb[1, 4], "one tap: its colour; none: the nearest pixel's")
        U.same(out[3, 7], rgb[1, 3] if not flagged[0] else rgb[2, 4], "one tap: its colour; none: the nearest pixel's")


def test_border_pixels_take_the_taps_inside(L):
    """offset_lo 0.5, offset_hi 0, r = 2: x = 0 has x0 = -1, and with offset_lo 0 the last column has x0 + 1 = w"""
    h, w = 3, 5
    rgb = (np.random.default_rng(5).random((h, w, 3)) * 4).astype(f32)
    out, _, mask, det = U.upsample(L, rgb, flat(h, w), flat(2 * h, 2 * w), U.make(2, False, offset_lo=(0.5, 0.5)), details=True)
    assert det[0, 0, 0] == -0.5 and det[0, 0, 1] == -0.5 and np.array_equal(det[0, 0, 2:6], [0, 0, 0, 0.25])
    U.same(out[0, 0], rgb[0, 0], "one tap inside at the top left corner")
    U.same(out[0, 1], rgb[0, 0], "x0 = 0, tx = 0, y0 = -1")
    out, _, mask, det = U.upsample(L, rgb, flat(h, w), flat(2 * h, 2 * w), U.make(2, False), details=True)
    assert det[5, 9, 0] == 4.5 and np.array_equal(det[5, 9, 2:6], [0.25, 0, 0, 0])
    U.same(out[5, 9], rgb[2, 4], "one tap inside at the bottom right corner")
    assert not mask.any()


def check_demodulation(L, plant=None):
    """constant irradiance E on albedo patterns of powers of two: u = E on every low pixel, exactly; the weights differ from tap to
    tap (the albedos do) and the quotient is still E; the output E times the HIGH pixel's albedo, exactly"""
    rng = np.random.default_rng(6)
    pw = np.array([1.0, 0.5, 0.25, 0.125], f32)
    g, hi = flat(5, 7), flat(10, 14)
    g["albedo"][..., :3] = pw[rng.integers(0, 4, (5, 7, 3))]
    hi["albedo"][..., :3] = pw[rng.integers(0, 4, (10, 14, 3))]
    E_ = f32(2.0)
    rgb = E_ * g["albedo"][..., :3]
    u = U.make(2, True, sigma_albedo=1.0)
    out, _, _, det = U.upsample(L, rgb, g, hi, u, plant=plant, details=True)
    assert ((det[..., 6] > 0) & (det[..., 6] < 0.9)).any(), "the weights are not trivial"
    U.same(out, E_ * hi["albedo"][..., :3], "E * albedo_hi")
    plain = U.upsample(L, rgb, g, hi, U.make(2, False, sigma_albedo=1.0))[0]
    assert (plain != out).mean() > 0.3, "without the flag the low albedo stays in the image"


def test_demodulation_returns_the_high_albedo_at_full_sharpness(L):
    check_demodulation(L)


# ---- the float64 restatement --------------------------------------------------------------------------------------------------------
def check_against_float64(L, rgb, g, hi, u, plant=None):
    """-> the share of high pixels left out: every colour within upsample64's bound wherever no decision lies inside its own bound,
    and the flags equal there"""
    out, _, mask, det = U.upsample(L, rgb, g, hi, u, plant=plant, details=True)
    want, bound, unresolved, unsure = U.upsample64(rgb, g, hi, u, det)
    keep = ~unsure
    worst = (np.abs(out - want) / bound)[keep].max()
    assert worst <= 1.0, f"out_rgb: {worst:.2f} of its bound"
    assert np.array_equal(mask[keep] != 0, unresolved[keep]), "unresolved"
    return float(unsure.mean())


def ramp_planes(r=4, h=6, w=9):
    """a plane receding along x: Z = 10 + 0.5 per high pixel, the low planes its samples at the same corner rays; colours vary"""
    g, hi = flat(h, w), flat(h * r, w * r)
    hi["depth"][:] = 10.0 + 0.5 * np.arange(w * r, dtype=f32)[None, :]
    g["depth"][:] = 10.0 + 0.5 * r * np.arange(w, dtype=f32)[None, :]
    return (np.random.default_rng(8).random((h, w, 3)) * 4).astype(f32), g, hi


def test_the_checker_is_its_float64_restatement_on_a_depth_ramp(L):
    """dzq = gx * ddx on every tap: e = dzq / den stays below 1 / sigma_depth only with the tap's distance in HIGH pixels"""
    rgb, g, hi = ramp_planes()
    out, _, _, det = U.upsample(L, rgb, g, hi, U.make(4, False, sigma_depth=0.5), details=True)
    assert check_against_float64(L, rgb, g, hi, U.make(4, False, sigma_depth=0.5)) == 0.0
    inner = det[:, 4:-4, 2:6]
    assert (inner[inner > 0] > np.exp(-2.0) / 16 * 0.9).all() and (inner > 0).any(), "every tap on the ramp counts: e < 1 / sigma_depth = 2"


_real = {}


def real_frames(LG, V, O, name, jitter):
    """the checker's guide planes of `name` at low 40 x 24 (four samples, corner or jittered) and high 80 x 48 (one corner sample)"""
    if (name, jitter) not in _real:
        w = GW.world(V, name)
        tex, dim = w.flatten()
        w.close()
        lo = G.planes(LG, O.make_scene(tex, dim, *GW.camera(V, name, (40, 24))), 40, 24, 0, 4, jitter=jitter)[0]
        hi = G.planes(LG, O.make_scene(tex, dim, *GW.camera(V, name, (80, 48))), 80, 48, 0, 1)[0]
        _real[name, jitter] = (lo, hi)
    return _real[name, jitter]


LOOSE = dict(sigma_normal=1.0, sigma_albedo=0.25, sigma_depth=4.0, min_weight=0.1)


@pytest.mark.parametrize("name", ["room", "lamp"])
def test_the_checker_is_its_float64_restatement_on_real_frames(L, LG, V, O, name):
    shares = []
    for jitter, kw, demodulate in ((False, {}, True), (True, LOOSE, True), (True, {}, False)):
        lo, hi = real_frames(LG, V, O, name, jitter)
        rgb = (np.random.default_rng(12).random((24, 40, 3)) * 4).astype(f32)
        u = U.make(2, demodulate, offset_lo=(0.5, 0.5) if jitter else (0.0, 0.0), **kw)
        shares.append(check_against_float64(L, rgb, lo, hi, u))
        mask = U.upsample(L, rgb, lo, hi, u)[2]
        assert mask.mean() < 0.5, "most pixels are rebuilt"
    print(f"{name}: share of high pixels left out {['%.4f' % s for s in shares]}")
    assert max(shares) <= 0.02, shares


# ---- planted misreadings ------------------------------------------------------------------------------------------------------------
def test_planted_misreadings_are_caught(L):
    with pytest.raises(AssertionError):
        check_bilinear(L, 2, (0.5, 0.5), (0.0, 0.0), False, plant="offsets_swapped")
    with pytest.raises(AssertionError):
        check_demodulation(L, plant="low_albedo_out")
    with pytest.raises(AssertionError):
        check_sky(L, plant="liveness_ignored")
    rgb, g, hi = ramp_planes()
    with pytest.raises(AssertionError, match="out_rgb"):
        check_against_float64(L, rgb, g, hi, U.make(4, False, sigma_depth=0.5), plant="ddx_unscaled")
    for plant in ("low_albedo_out", "liveness_ignored"):          # ... and the float64 restatement sees these two as well
        rng = np.random.default_rng(9)
        rgb, g = random_planes(rng, 6, 9)
        with pytest.raises(AssertionError):
            check_against_float64(L, rgb, g, random_planes(rng, 12, 18)[1], U.make(2, True, **LOOSE), plant=plant)


# ---- what needs no device -----------------------------------------------------------------------------------------------------------
def test_the_struct_mirror_is_the_headers(V):
    text = open(os.path.join(ROOT, "include", "vrt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"struct\s+vrt_upsample\s*\{(.*?)\}\s*;", text, flags=re.S).group(1)
    assert re.search(r"typedef\s+struct\s+vrt_upsample\s+vrt_upsample\s*;", text)
    ctypes_of = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    fields = [(name.strip(), ctypes_of[d.split(None, 1)[0]]) for d in (d.strip() for d in body.split(";")) if d
              for name in d.split(None, 1)[1].split(",")]
    assert fields == list(V.Upsample._fields_) == list(U.Upsample._fields_)
    assert C.sizeof(V.Upsample) == C.sizeof(U.Upsample) == 40
    assert V.UPSAMPLE_MAX_FACTOR == U.MAX_FACTOR == int(re.search(r"#define VRT_UPSAMPLE_MAX_FACTOR (\d+)", text).group(1))
    assert V.UPSAMPLE_DEMODULATE == U.DEMODULATE == int(re.search(r"#define VRT_UPSAMPLE_DEMODULATE (\d+)u", text).group(1))


def test_the_defaults(V):
    d = V.default_upsample()
    assert set(d) == set(U.KEYS) and 1 <= d["factor"] <= V.UPSAMPLE_MAX_FACTOR and 0 <= d["min_weight"] < 1
    assert all(d[k] == 0.0 for k in U.KEYS[6:]) and all(d[k] > 0 for k in U.KEYS[2:5])
    u = V.Upsample()
    V.hip_lib().vrt_upsample_default(C.byref(u))
    made = U.make()
    for k, _ in V.Upsample._fields_:
        assert getattr(made, k) == getattr(u, k), k              # the checker's defaults are the library's
    assert U.keys(made) == d
    best = open(os.path.join(ROOT, "profiles", "upsample_quality.txt")).read().splitlines()
    best = [l for l in best if l.startswith("# best:")][0].split()
    swept = {best[i]: float(f32(best[i + 1])) for i in range(2, 12, 2)}              # the sweep's best row is the default
    assert swept == {"demodulate": float(d["demodulate"]), **{k: d[k] for k in ("sigma_normal", "sigma_albedo", "sigma_depth", "min_weight")}}


@pytest.mark.parametrize("bad", [{"factor": 0}, {"factor": 5}, {"factor": 2.0}, {"sigma_depth": 0.0}, {"sigma_normal": float("nan")},
                                 {"min_weight": 1.0}, {"min_weight": -0.1}, {"offset_lo_x": 1.5}, {"offset_hi_y": -0.5}, {"sigma": 1.0}])
def test_the_binding_refuses_bad_parameters_before_the_library(V, bad):
    with pytest.raises(ValueError):
        V.Context._upsample(bad)
    assert V.Context._upsample(None) is None and V.Context._upsample({"factor": 3, "demodulate": False}).flags == 0
