"""The HDR display pass's checker (tests/oracle_denoise_hdr.c, include/vrt.h vrt_denoise_hdr) held to what it restates, on the CPU:
it is the byte pass on byte / 255.0f images; its floats are the float64 evaluation of the same sums within the summation bound;
h(c) at its edges; and two planted misreadings -- sums across ids, the tone map before the blur -- that the comparisons catch."""
import numpy as np
import pytest

import oracle_denoise_hdr as D
import oracle_hdr

DISTS = [0, 1, 2, 50, 99, 100, 101, 400, 2047, 40000]


@pytest.fixture(scope="module")
def DL(tmp_path_factory):
    return D.build(tmp_path_factory.mktemp("oracle_denoise_hdr"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _random_ids(rng, W, H):
    idd = np.zeros((H, W, 2), np.int32)
    idd[..., 0] = rng.integers(-3, 4, size=(H, W))
    idd[..., 1] = rng.choice(DISTS, size=(H, W))
    return idd


def _faces(rng, W, H):
    """ids in patches a few pixels across, as voxel faces are: windows that hold many taps of the centre's id"""
    yy, xx = np.mgrid[0:H, 0:W]
    idd = np.zeros((H, W, 2), np.int32)
    idd[..., 0] = 1 + (yy // 9) * 16 + xx // 13
    idd[..., 0][rng.random((H, W)) < 0.05] = 0
    idd[..., 1] = rng.choice([90, 100, 150, 400, 2047], size=(H, W))
    return idd


def test_byte_identity(DL, V, O, product_scenes):
    """On byte / 255.0f images with the NULL tone map the checker's bytes are the byte pass's (contract point 4)."""
    cases = []
    tex, dim = product_scenes["dragon"]
    for pose, (W, H) in (((63.5, 60.5, 140.5, -90.0, -10.0), (96, 54)), ((60.3, 64.7, 75.2, -100.0, -25.0), (80, 48))):
        ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
        rgba, idd = O.render(O.make_scene(tex, dim, ip, iv, cp), W, H, 2)[:2]
        assert np.all(rgba[..., 3] == 255)
        cases.append((f"dragon {W}x{H}", rgba, idd))
    rng = np.random.default_rng(3)
    for W, H in ((150, 90), (67, 35)):
        rgba = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
        rgba[..., 3] = 255          # what every image of the library carries; the HDR pass writes 255 (point 4)
        cases.append((f"random ids {W}x{H}", rgba, _random_ids(rng, W, H)))
        cases.append((f"random faces {W}x{H}", rgba, _faces(rng, W, H)))
    for what, rgba, idd in cases:
        rgb = rgba[..., :3].astype(np.float32) / np.float32(255.0)
        assert rgb.dtype == np.float32
        got = D.denoise(DL, rgb, idd, None)[1]
        want = O.denoise(rgba, idd)
        assert np.array_equal(got, want), (what, int(np.sum(np.any(got != want, axis=-1))))
    assert any(np.any(O.denoise(rgba, idd) != rgba) for _, rgba, idd in cases)   # and the pass did blur something


def test_floats_against_float64(DL):
    """Every summed pixel: relative error of the checker's float against the float64 evaluation of the same sum and division at
    most count * 2^-24 * (1 + 1e-3) -- the recursive-summation bound for `count` non-negative terms (count - 1 additions) and one
    division. Non-negative terms make it a pure relative bound, so no pixel is left out."""
    rng = np.random.default_rng(17)
    worst = 0.0
    for W, H, ids in ((70, 50, "faces"), (61, 47, "one"), (40, 30, "random")):
        rgb = np.exp2(rng.uniform(-20, 16, size=(H, W, 3))).astype(np.float32)
        rgb[rng.random((H, W)) < 0.02] = np.float32(1e5)      # beyond 65504
        if ids == "faces":
            idd = _faces(rng, W, H)
        elif ids == "random":
            idd = _random_ids(rng, W, H)
        else:
            idd = np.zeros((H, W, 2), np.int32)
            idd[..., 0] = 7
            idd[..., 1] = 100                                  # radius 20: up to 1681 taps
        got = D.denoise(DL, rgb, idd)[0].astype(np.float64)
        ref, count = D.denoise64(DL, rgb, idd)
        summed = count > 0
        assert summed.any() and (ids != "one" or count.max() == 1681)
        assert np.all(ref[summed] > 0.0)
        rel = np.abs(got - ref) / np.where(ref > 0.0, ref, 1.0)
        bound = (count * 2.0 ** -24 * (1 + 1e-3))[..., None]
        print(f"{ids} {W}x{H}: worst relative error / bound = {float(np.max((rel / np.maximum(bound, 1e-300))[summed])):.3f}")
        assert np.all(rel[summed] <= np.broadcast_to(bound, rel.shape)[summed]), ids
        # pixels that pass through are h(c) exactly
        assert np.array_equal(_bits(got.astype(np.float32)[~summed]), _bits(D.h_of(DL, rgb)[~summed]))
        worst = max(worst, float(rel[summed].max()))
    assert worst > 0.0     # float32 sums of 1681 terms do round: the comparison is not vacuous


def test_h_at_its_edges(DL):
    sub = np.float32(1e-41)
    assert sub != 0 and sub < np.finfo(np.float32).tiny
    cases = [(np.nan, 0.0), (np.inf, 65504.0), (-np.inf, 0.0), (-1.5, 0.0), (-1e-41, 0.0), (-0.0, 0.0), (65504.0, 65504.0),
             (65505.0, 65504.0), (sub, sub), (0.0, 0.0), (0.25, 0.25)]
    for c, want in cases:
        got = oracle_hdr.value(DL, np.float32(c))
        assert _bits(got) == _bits(np.float32(want)), (c, got, want)      # bits: -0 must come out as +0
    # ... and through the pass: as a pass-through pixel, as the centre and as a tap
    vals = np.array([c for c, _ in cases], np.float32)
    n = len(vals)
    rgb = np.zeros((3, n, 3), np.float32)
    rgb[1, :, 0] = vals
    rgb[1, :, 1] = vals[::-1]
    rgb[1, :, 2] = 0.5
    idd = np.zeros((3, n, 2), np.int32)
    out, out8 = D.denoise(DL, rgb, idd)                                     # all sky
    assert np.array_equal(_bits(out), _bits(D.h_of(DL, rgb)))
    assert np.all(np.isfinite(out)) and np.all(out >= 0) and not np.any(np.signbit(out))
    assert np.array_equal(out8, oracle_hdr.tonemap(DL, out))
    idd[..., 0] = 4
    idd[..., 1] = 40000                                                    # radius 1
    out, _ = D.denoise(DL, rgb, idd)
    ref, count = D.denoise64(DL, rgb, idd)
    assert np.all(np.isfinite(out)) and np.all(out >= 0)
    assert np.all(np.abs(out - ref) <= ref * (count * 2.0 ** -24 * (1 + 1e-3))[..., None])


def test_planted_misreading_sum_across_ids(DL):
    """A restatement that ignores the id test must fail the float comparison: the check can fail."""
    rng = np.random.default_rng(5)
    W, H = 60, 40
    rgb = np.exp2(rng.uniform(-6, 6, size=(H, W, 3))).astype(np.float32)
    idd = _faces(rng, W, H)
    got = D.denoise(DL, rgb, idd)[0]
    wrong = D.misread_across_ids(DL, rgb, idd)
    ref, count = D.denoise64(DL, rgb, idd)
    bound = (count * 2.0 ** -24 * (1 + 1e-3))[..., None]
    summed = count > 0
    assert np.all((np.abs(got - ref) <= ref * bound)[summed])
    assert np.any((np.abs(wrong - ref) > ref * bound)[summed])
    assert not np.array_equal(_bits(got), _bits(wrong))


@pytest.mark.parametrize("op,e", [("clamp", 1.0), ("reinhard", 1.0)])
def test_planted_misreading_tonemap_before_blur(DL, O, op, e):
    """One 10.0 emitter pixel inside a face of 0.2 grey: blurring the tone-mapped bytes (the emitter already clamped / compressed)
    gives other bytes than tone-mapping the blurred floats."""
    W, H = 24, 16
    rgb = np.full((H, W, 3), 0.2, np.float32)
    rgb[8, 12] = 10.0
    idd = np.zeros((H, W, 2), np.int32)
    idd[4:12, 6:18, 0] = 11          # the face; sky around it
    idd[..., 1] = 2047               # radius 4
    got = D.denoise(DL, rgb, idd, op, e)[1]
    wrong = D.misread_tonemap_first(DL, O, rgb, idd, op, e)
    face = idd[..., 0] != 0
    assert np.array_equal(got[~face], wrong[~face])         # sky passes through either way
    assert np.any(got[face] != wrong[face])
    # the emitter's own pixel: the filtered estimate is brighter than the blur of a clamped sample
    assert int(got[8, 12, 0]) > int(wrong[8, 12, 0])
