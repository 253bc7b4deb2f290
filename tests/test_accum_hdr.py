"""HDR accumulation (vrt_accum_keep_hdr, vrt_accum_resolve_hdr): what holds without a GPU. The checker's float colours
(tests/oracle_hdr.c) store the bytes of the byte checkers in every mode and for every ray source; h(c) keeps every float's byte;
k sequential float64 adds of a float equal the one product the repeat shortcuts take; the tone maps are the header's formulas;
and on a committed scene the mean of the unclamped colours is visibly not the mean of the clamped bytes. The library exports
the calls and the Python wrapper refuses bad values before any device is involved. The kernels are held to the checker on the
MI355X (test_gpu_accum_hdr.py)."""
import subprocess

import numpy as np
import pytest

import oracle_hdr
import oracle_lens
import oracle_samples

POSES = {   # tests/test_accum_jitter.py's poses
    "dragon": ("dragon", (63.5, 60.5, 140.5, -90.0, -10.0)),
    "room_inside": ("room", (14.5, 30.5, 16.5, 32.0, -10.0)),
    "room_outside": ("room", (98.5, 34.5, 52.5, 197.0, -8.0)),
}
EDGE = np.array([np.nan, -np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1e-45, -1e-45, 1e-39, 1.17549435e-38, 0.5 / 255.0, 0.5, 1.0,
                 1.0000001, 10.0, 65503.996, 65504.0, 65504.004, 65536.0, 1e30, 3.4028235e38, -3.4028235e38], np.float32)


@pytest.fixture(scope="module")
def HL(tmp_path_factory):
    return oracle_hdr.build(tmp_path_factory.mktemp("oracle_hdr"))


@pytest.fixture(scope="module")
def LL(tmp_path_factory):
    return oracle_lens.build(tmp_path_factory.mktemp("oracle_lens"))


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    return oracle_samples.build(tmp_path_factory.mktemp("oracle_samples"))


def _scene(O, V, product_scenes, name, W, H):
    m, pose = POSES[name]
    tex, dim = product_scenes[m]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    return O.make_scene(tex, dim, ip, iv, cp)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(POSES))
def test_unorm8_of_the_checkers_floats_is_the_byte_checkers_sample(HL, LL, S, O, V, product_scenes, name):
    W, H = 40, 25
    s = _scene(O, V, product_scenes, name, W, H)
    for mode in (0, 1, 2):
        for k in (0, 3, 2 ** 32 - 1):
            ref, _ = oracle_samples.render_sample(S, s, W, H, mode, k)
            assert np.array_equal(oracle_hdr.rgba_of(HL, oracle_hdr.render(HL, s, W, H, mode, k)), ref), (mode, k, "corner")
            for jitter, ap in ((True, 0.0), (False, 1.5), (True, 1.5)):
                ref, _ = oracle_lens.render(LL, s, W, H, mode, k, ap, 30.0, jitter=jitter)
                got = oracle_hdr.render(HL, s, W, H, mode, k, jitter=jitter, aperture=ap, focus=30.0)
                assert np.array_equal(oracle_hdr.rgba_of(HL, got), ref), (mode, k, jitter, ap)


def test_h_keeps_every_floats_byte(HL):
    rng = np.random.default_rng(5)
    vals = np.concatenate([EDGE, rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                           rng.random(2000, dtype=np.float32) * np.float32(1.2)])
    h = np.array([oracle_hdr.value(HL, v) for v in vals], np.float32)
    assert np.array_equal(oracle_hdr.unorm8(HL, h), oracle_hdr.unorm8(HL, vals))
    assert np.all(h >= 0.0) and np.all(h <= np.float32(65504.0)) and not np.isnan(h).any()
    assert _bits(h[np.isnan(vals)]).tolist() == [0] * int(np.isnan(vals).sum())     # NaN -> +0
    inside = (vals >= 0.0) & (vals <= np.float32(65504.0))
    assert np.array_equal(_bits(h[inside & (vals != 0)]), _bits(vals[inside & (vals != 0)]))


def test_k_sequential_adds_are_the_product(HL):
    rng = np.random.default_rng(6)
    cs = np.concatenate([np.array([0.0, 1e-45, 1.0 / 3.0, 1.0, 9.999999, 65504.0, 1e9], np.float32),
                         (rng.random(6, dtype=np.float32) * np.float32(12.0))])
    for c in cs:
        for k in (1, 2, 3, 255, 4097, 2 ** 24):
            a, b = HL.o_hdr_sum_repeat(float(c), k), HL.o_hdr_product(float(c), k)
            assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64), (c, k)
    # ... and continued: m samples already in the sum, k more
    for c in cs[:8]:
        m, k = 1000, 2 ** 24 - 1000
        assert HL.o_hdr_product(float(c), m) + HL.o_hdr_product(float(c), k) == HL.o_hdr_sum_repeat(float(c), m + k)


def test_tone_maps_are_the_headers_formulas(HL):
    rng = np.random.default_rng(7)
    x = np.concatenate([EDGE[~np.isnan(EDGE) & (EDGE >= 0) & (EDGE <= 65504.0)],
                        rng.random(3000, dtype=np.float32) * np.float32(20.0)]).astype(np.float32)
    x = np.resize(x, (x.size // 3) * 3).reshape(1, -1, 3)
    for e in (np.float32(1.0), np.float32(0.37), np.float32(2.5)):
        xe = (e * x).astype(np.float32)
        for op, y in (("clamp", xe), ("reinhard", (xe / (np.float32(1.0) + xe)).astype(np.float32))):
            want = np.rint(np.minimum(np.maximum(y, np.float32(0.0)), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)
            got = oracle_hdr.tonemap(HL, x, op, e)
            assert np.array_equal(got[..., :3], want) and np.all(got[..., 3] == 255), (op, e)


def test_mean_is_the_float64_quotient_rounded_once(HL):
    rng = np.random.default_rng(8)
    H, W = 4, 5
    acc = oracle_hdr.Accum(HL, H, W)
    total = np.zeros((H, W, 3), np.float64)
    for _ in range(7):
        rgb = (rng.random((H, W, 3), dtype=np.float32) * np.float32(30.0) - np.float32(2.0)).astype(np.float32)
        acc.add(rgb)
        total = total + np.minimum(np.maximum(rgb, np.float32(0.0)), np.float32(65504.0)).astype(np.float64)
    assert np.array_equal(acc.hsum.view(np.uint64), total.view(np.uint64))
    assert np.array_equal(_bits(acc.mean()), _bits((total / np.float64(7)).astype(np.float32)))


def test_the_room_shows_what_clamped_bytes_lose(HL, O, V, product_scenes):
    """The reference's room seen from outside (pose room_outside): the sky behind the diffuse bounce, on top of the direct light,
    puts samples above 1 on its lit faces (from inside, and on the dragon and the terrain, no sample of the checker exceeds 1).
    There the HDR resolve under the clamp operator at exposure 1 -- unorm8 of the mean of the colours -- is not the mean of the
    stored bytes."""
    W, H, n = 48, 30, 8
    s = _scene(O, V, product_scenes, "room_outside", W, H)
    acc = oracle_hdr.Accum(HL, H, W)
    bright = 0
    for k in range(n):
        rgb = oracle_hdr.render(HL, s, W, H, 2, k, jitter=True)
        bright += int((rgb > 1.0).any(axis=2).sum())
        acc.add(rgb)
    hdr_bytes = oracle_hdr.tonemap(HL, acc.mean(), "clamp", 1.0)
    differ = int((hdr_bytes != acc.resolve_bytes()).any(axis=2).sum())
    print(f"samples above 1: {bright}; pixels whose HDR resolve differs from the byte resolve: {differ} of {W * H}")
    assert bright > 0
    assert differ > 0


def test_library_exports_the_hdr_calls(V):
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"vrt_accum_keep_hdr", "vrt_accum_resolve_hdr", "vrt_accum_resolve_hdr_device"} <= names


def _unopened(V):
    return object.__new__(V.Context)


@pytest.mark.parametrize("kw", [dict(tonemap="aces"), dict(tonemap=1), dict(exposure=0.0), dict(exposure=-1.0),
                                dict(exposure=float("nan")), dict(exposure=float("inf")), dict(exposure=1e39),
                                dict(exposure=1e-50), dict(exposure=True), dict(exposure=None)])
def test_resolve_hdr_rejects_bad_values_before_the_device(V, kw):
    with pytest.raises(ValueError):
        _unopened(V).accum_resolve_hdr(**kw)


def test_accum_begin_rejects_a_bad_hdr_flag_before_the_device(V):
    for bad in (2, "yes", None, 1.0):
        with pytest.raises(ValueError):
            _unopened(V).accum_begin(8, 8, hdr=bad)
