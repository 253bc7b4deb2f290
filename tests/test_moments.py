"""Luminance moments of an HDR accumulation (vrt_accum_keep_moments, vrt_accum_variance; M1-M3 of include/vrt.h): what holds without
a GPU. The checker (tests/oracle_moments.c) against closed forms -- equal samples give exactly +0 at any count, one sample gives
"unknown", two alternating values their textbook variance, NaN / Inf / negative colours go through h --, the products that stand for
k equal samples, 3 + 5 adds equal to 8, the plane against a float64 variance of the same luminances within a bound derived from the
rule, three planted misreadings each caught, and the filtered chain. The library exports the calls and the wrapper refuses bad
values before any device is involved. The kernels are held to the checker on the MI355X (test_gpu_moments.py)."""
import subprocess

import numpy as np
import pytest

import filter_quality as Q
import oracle_filter_var as FV
import oracle_guides
import oracle_hdr
import oracle_moments as OM

W, H = Q.W, Q.H          # 40 x 24
FIRST, N = Q.FIRST, Q.N_IN
LUMA = (np.float32(0.2126), np.float32(0.7152), np.float32(0.0722))


@pytest.fixture(scope="module")
def ML(tmp_path_factory):
    return OM.build(tmp_path_factory.mktemp("oracle_moments"))


@pytest.fixture(scope="module")
def frames(ML, V, O):
    """the checker's own float samples FIRST .. FIRST + 7 of the room and the lamp room, jittered VRT_MODE_FULL, rendered once"""
    out = {}
    for name in Q.WORLDS:
        w, pose = Q._world(V, name)
        tex, dim = w.flatten()
        w.close()
        scene = O.make_scene(tex, dim, *V.camera_block(pose[:3], pose[3], pose[4], W, H)[:3])
        out[name] = (scene, [oracle_hdr.render(ML, scene, W, H, Q.MODE_FULL, FIRST + k, jitter=True) for k in range(8)])
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _y32(c):
    """M1 in numpy float32, every operation rounded on its own"""
    h = np.minimum(np.maximum(np.float32(0.0), np.nan_to_num(np.asarray(c, np.float32), nan=0.0, posinf=np.inf, neginf=-np.inf)), np.float32(65504.0))
    return np.float32(np.float32(np.float32(LUMA[0] * h[..., 0]) + np.float32(LUMA[1] * h[..., 1])) + np.float32(LUMA[2] * h[..., 2]))


def _pixel(ML, colours, plant=None):
    """the accumulation of one pixel that takes `colours` in order -> (Accum, variance)"""
    acc = OM.Accum(ML, 1, 1, plant=plant)
    for c in colours:
        acc.add(np.array(c, np.float32).reshape(1, 1, 3))
    return acc, acc.variance(plant)[0, 0]


def _bound(y, n):
    """|M3's plane - the float64 variance of the mean of the float luminances y[0..n)| is at most this.
    Exact: d* = m2* - m1*^2 with m1* = sum(y) / n, m2* = sum(y^2) / n, ref = max(0, d*) / (n - 1). The rule differs from it by
      q = fl32(y * y):        |q - y^2| <= 2^-24 y^2 (or 2^-150 where the product is subnormal), so |m2 - m2*| <= 2^-24 m2* + 2^-150
      m1f = fl32(m1):         |m1f - m1*| <= 2^-24 m1*, so |m1f^2 - m1*^2| <= (2^-23 + 2^-48) m1*^2
      sq = fl32(m1f * m1f):   |sq - m1f^2| <= 2^-24 m1f^2 + 2^-150
    and m1*^2 <= m2* (Cauchy-Schwarz): |d - d*| <= (2^-24 + 2^-23 + 2^-24) m2* + slack = 2^-22 m2* + slack, where the slack covers
    the float64 roundings of the n adds of each sum, the two divisions and the subtraction (at most (n + 4) 2^-53 m2* each side:
    2^-40 m2* is ample for n <= 2^12) and the two subnormal terms. max(0, .) and the division by n - 1 do not enlarge it, and the
    final cast to float32 adds 2^-24 of the value (2^-149 where subnormal); hv is the identity below 65504^2."""
    y = np.asarray(y, np.float64)
    m2 = (y * y).sum(axis=0) / n
    m1 = y.sum(axis=0) / n
    ref = np.maximum(0.0, m2 - m1 * m1) / (n - 1)
    e = ((2.0 ** -22 + 2.0 ** -40) * m2 + 2.0 ** -148) / (n - 1)
    return ref, e + 2.0 ** -24 * (ref + e) + 2.0 ** -149


# ---- closed forms --------------------------------------------------------------------------------------------------------------------

COLOURS = [(0.3, 0.7, 0.1), (1.0, 1.0, 1.0), (1.0 / 3.0, 2.0 / 3.0, 0.123456), (9.75, 0.001, 31.5), (65504.0, 65504.0, 65504.0),
           (1e-20, 3e-21, 0.0), (0.0, 0.0, 0.0)]


@pytest.mark.parametrize("n", [2, 3])
def test_equal_samples_have_exactly_no_variance(ML, n):
    for c in COLOURS:
        assert _bits(_pixel(ML, [c] * n)[1]) == 0, (c, n)


def test_equal_samples_have_no_variance_at_the_cap_through_the_products(ML):
    rng = np.random.default_rng(11)
    cs = [np.array(c, np.float32) for c in COLOURS] + list((rng.random((6, 3), dtype=np.float32) * np.float32(12.0)))
    for c in cs:
        for k in (1, 2, 3, 255, 4097):      # the product is the k sequential adds ...
            assert np.array_equal(OM.sum_repeat(ML, c, k).view(np.uint64), OM.add_product(ML, c, k).view(np.uint64)), (c, k)
        s = OM.add_product(ML, c, 1000, OM.sum_repeat(ML, c, 24))     # ... also continued from a sum
        assert np.array_equal(s.view(np.uint64), OM.sum_repeat(ML, c, 1024).view(np.uint64)), c
        full = OM.add_product(ML, c, 2 ** 24)                         # ... and at 2^24 it is exact: y and q are floats
        y = np.float64(OM.luminance(ML, c))
        q = np.float64(np.float32(np.float32(y) * np.float32(y)))
        assert full[0] == y * 2.0 ** 24 and full[1] == q * 2.0 ** 24
        var = OM.variance_of(ML, full.reshape(1, 1, 2), np.full((1, 1), 2 ** 24, np.uint32))
        assert _bits(var)[0, 0] == 0, c


def test_one_sample_is_unknown(ML):
    acc, var = _pixel(ML, [(0.3, 0.7, 0.1)])
    assert _bits(var) == _bits(OM.VAR_UNKNOWN)
    assert _bits(OM.variance_of(ML, np.zeros((1, 1, 2)), np.zeros((1, 1), np.uint32)))[0, 0] == _bits(OM.VAR_UNKNOWN)   # no sample at all


@pytest.mark.parametrize("n", [2, 4, 8, 64])
def test_two_alternating_values(ML, n):
    for a, b in (((0.2, 0.2, 0.2), (0.9, 0.9, 0.9)), ((3.5, 0.25, 0.0), (0.0, 0.75, 12.0)), ((1.0, 1.0, 1.0), (1.0000001, 1.0, 1.0)),
                 ((65504.0, 65504.0, 65504.0), (0.0, 0.0, 0.0))):
        acc, var = _pixel(ML, [a, b] * (n // 2))
        ya, yb = np.float64(OM.luminance(ML, np.float32(a))), np.float64(OM.luminance(ML, np.float32(b)))
        want = ((ya - yb) / 2.0) ** 2 / (n - 1)
        ref, bound = _bound(np.array([ya, yb] * (n // 2)), n)
        assert abs(ref - want) <= 1e-12 * want + 1e-300
        assert abs(np.float64(var) - want) <= bound + 1e-12 * want, (a, b, n, var, want, bound)


def test_luminance_is_v1_on_h(ML):
    rng = np.random.default_rng(12)
    c = (rng.random((500, 3), dtype=np.float32) * np.float32(40.0) - np.float32(4.0)).astype(np.float32)
    assert np.array_equal(_bits(OM.luminance(ML, c)), _bits(_y32(c)))


def test_nan_inf_and_negative_colours_go_through_h(ML):
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    assert _bits(OM.luminance(ML, np.array([nan, -1.0, -inf], np.float32))) == 0                       # all three to +0
    assert _bits(OM.luminance(ML, np.array([inf, 1e30, 70000.0], np.float32))) == _bits(_y32(np.full(3, 65504.0, np.float32)))
    assert _bits(OM.luminance(ML, np.array([-0.0, nan, 2.0], np.float32))) == _bits(np.float32(LUMA[2] * np.float32(2.0)))
    acc, var = _pixel(ML, [(nan, nan, nan), (inf, inf, inf)] * 2)          # 0 and Y(65504, 65504, 65504) alternating: finite
    ymax = np.float64(_y32(np.full(3, 65504.0, np.float32)))
    ref, bound = _bound(np.array([0.0, ymax, 0.0, ymax]), 4)
    assert np.isfinite(var) and abs(np.float64(var) - ref) <= bound
    acc, var = _pixel(ML, [(nan, -3.0, -inf)] * 3)                          # every sample h's to black: equal samples
    assert _bits(var) == 0 and not acc.msum.any()


# ---- splitting -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", [None, (2, 6, 24)], ids=["plain", "adaptive"])
def test_three_plus_five_adds_equal_eight(ML, frames, rule):
    """the sums continue: an accumulation resolved after 3 samples and then given 5 more holds what 8 at once give"""
    _, samples = frames["room"]
    whole = OM.Accum(ML, H, W, rule)
    for s in samples:
        whole.add(s)
    split = OM.Accum(ML, H, W, rule)
    for s in samples[:3]:
        split.add(s)
    three = split.variance().copy()
    for s in samples[3:]:
        split.add(s)
    assert np.array_equal(split.msum.view(np.uint64), whole.msum.view(np.uint64))
    assert np.array_equal(_bits(split.variance()), _bits(whole.variance()))
    assert not np.array_equal(_bits(three), _bits(whole.variance()))
    assert np.array_equal(split.hsum.view(np.uint64), whole.hsum.view(np.uint64))      # and the colour sums never saw the moments
    plain = oracle_hdr.Accum(ML, H, W, rule)
    for s in samples:
        plain.add(s)
    assert np.array_equal(plain.hsum.view(np.uint64), whole.hsum.view(np.uint64)) and np.array_equal(plain.counts(), whole.counts())


# ---- against float64 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("name", Q.WORLDS)
def test_plane_against_a_float64_variance_of_the_same_luminances(ML, frames, name, n):
    _, samples = frames[name]
    acc = OM.Accum(ML, H, W)
    for s in samples[:n]:
        acc.add(s)
    y = np.stack([OM.luminance(ML, s) for s in samples[:n]]).astype(np.float64)
    ref, bound = _bound(y, n)
    assert np.allclose(ref, np.var(y, axis=0, ddof=1) / n, rtol=1e-9, atol=1e-18)     # it is numpy's variance of the mean
    got = acc.variance().astype(np.float64)
    miss = np.abs(got - ref) > bound
    print(f"{name} n {n}: max |plane - float64| / bound {np.max(np.abs(got - ref) / bound):.3f}, pixels with variance {int((ref > 0).sum())} of {W * H}")
    assert int(miss.sum()) == 0          # the share of pixels left out is 0
    assert (ref > 0).sum() > W * H // 4  # ... and the frames are not flat


# ---- planted misreadings ---------------------------------------------------------------------------------------------------------------

def _misses(ML, samples, n, plant):
    acc = OM.Accum(ML, H, W, plant=plant)
    for s in samples[:n]:
        acc.add(s)
    y = np.stack([OM.luminance(ML, s) for s in samples[:n]]).astype(np.float64)
    ref, bound = _bound(y, n)
    return int((np.abs(acc.variance(plant).astype(np.float64) - ref) > bound).sum())


@pytest.mark.parametrize("name", Q.WORLDS)
def test_planted_divisor_n_is_caught(ML, frames, name):
    assert _misses(ML, frames[name][1], 4, None) == 0
    assert _misses(ML, frames[name][1], 4, "divisor_n") > W * H // 4


@pytest.mark.parametrize("name", Q.WORLDS)
def test_planted_luminance_of_the_clamped_bytes_is_caught(ML, frames, name):
    assert _misses(ML, frames[name][1], 4, "y_of_bytes") > W * H // 8


def test_planted_square_of_the_mean_in_double_is_caught(ML):
    """with the mean squared in double, equal samples no longer cancel: m2 is the float32-rounded q, m1 * m1 is not"""
    rng = np.random.default_rng(13)
    cs = rng.random((64, 3), dtype=np.float32) * np.float32(8.0)
    noisy = 0
    for c in cs:
        for n in (2, 3, 7):
            assert _bits(_pixel(ML, [c] * n)[1]) == 0
            noisy += int((_bits(_pixel(ML, [c] * n, plant="square_in_double")[1]) != 0).any())
    assert noisy > len(cs)       # about half of all colours round q upwards


# ---- the filtered chain ----------------------------------------------------------------------------------------------------------------

def test_filtered_chain_takes_the_plane_from_two_samples_on(ML, frames, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("oracle_chain")
    LV, LG = FV.build(tmp), oracle_guides.build(tmp)
    scene, samples = frames["lamp"]
    f = FV.make(2, True, 0.5, 0.05, 0.5, 4.0)
    acc = OM.Accum(ML, H, W)
    acc.add(samples[0])
    g1 = oracle_guides.planes(LG, scene, W, H, FIRST, 1, jitter=True)[0]
    one = OM.resolve_filtered_var(LV, acc, g1, f)
    for a, b in zip(one, FV.filter(LV, acc.mean(), g1, f, None)):       # one sample: the spatial estimate
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    for s in samples[1:N]:
        acc.add(s)
    g = oracle_guides.planes(LG, scene, W, H, FIRST, N, jitter=True)[0]
    got = OM.resolve_filtered_var(LV, acc, g, f, "reinhard", 1.5)
    want = FV.filter(LV, acc.mean(), g, f, acc.variance(), "reinhard", 1.5)
    spatial = FV.filter(LV, acc.mean(), g, f, None, "reinhard", 1.5)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert not np.array_equal(_bits(got[0]), _bits(spatial[0])) and not np.array_equal(_bits(got[2]), _bits(spatial[2]))
    # the plane is what the quality sweep's numpy variance is, within the bound above
    y = np.stack([OM.luminance(ML, s) for s in samples[:N]]).astype(np.float64)
    ref, bound = _bound(y, N)
    assert np.all(np.abs(acc.variance().astype(np.float64) - ref) <= bound)


# ---- the library and the wrapper -------------------------------------------------------------------------------------------------------

def test_library_exports_the_moments_calls(V):
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"vrt_accum_keep_moments", "vrt_accum_variance", "vrt_accum_variance_device"} <= names


def test_hip_code_object_holds_the_moments_kernels(V):
    blob = open(V.HIP_LIB, "rb").read()
    for kernel in (b"mom_variance_kernel", b"repeat_mom_kernel"):
        assert kernel in blob, kernel


def _unopened(V):
    return object.__new__(V.Context)


def test_accum_begin_rejects_bad_moments_before_the_device(V):
    for bad in (2, "yes", None, 1.0):
        with pytest.raises(ValueError):
            _unopened(V).accum_begin(8, 8, hdr=True, moments=bad)
    with pytest.raises(ValueError):
        _unopened(V).accum_begin(8, 8, moments=True)                 # moments without hdr
    with pytest.raises(ValueError):
        _unopened(V).accum_begin(8, 8, hdr=False, moments=1)
