"""Adaptive accumulation without a GPU (include/vrt.h vrt_accum_begin_adaptive): the stopping rule and the round semantics in
Python integers (tests/oracle_adaptive.py) on per-sample frames of the checkers, the library's own rule (the test library's
host probe of vrt_accum.h adaptive_active) against Python integers at the extremes and one either side of the threshold, the
exports, and the Python wrapper's argument checks before any device call."""
import os
import subprocess

import numpy as np
import pytest

import oracle_adaptive as A
import oracle_jitter

TOP = 1 << 24


@pytest.fixture(scope="module")
def J(tmp_path_factory):
    return oracle_jitter.build(tmp_path_factory.mktemp("oracle_jitter"))


def _py_rule(n, s, q, lo, hi, tol):
    return n < lo or (n < hi and 256 * (n * q - s * s) > tol * tol * n * n * (n - 1))


# ---- the rule ----

def _const(n, L):
    return n, n * L, n * L * L


@pytest.mark.parametrize("tol", [0, 1, 24, 200, 65535])
def test_probe_at_the_extremes(V, tol):
    # n = 2^24 samples of L = 765 (white): S = 765 * 2^24, Q = 765^2 * 2^24 -- the largest state the rule ever sees
    for lo, hi in ((2, TOP), (TOP, TOP), (2, TOP - 1), (TOP - 1, TOP - 1)):
        for n in (TOP, TOP - 1, 2, 1, 0):
            n_, s, q = _const(n, 765)
            assert V.adaptive_rule(n_, s, q, lo, hi, tol) == _py_rule(n_, s, q, lo, hi, tol) == A.active(n_, s, q, lo, hi, tol)
    # the largest spread: half the samples 0, half 765 at n = 2^24 - 2, below max
    n = TOP - 2
    s, q = (n // 2) * 765, (n // 2) * 765 * 765
    for hi in (TOP, TOP - 1):
        assert V.adaptive_rule(n, s, q, 2, hi, tol) == _py_rule(n, s, q, 2, hi, tol)
    # a standard error of 0.093 L units: tolerance 1 (1/16 = 0.0625 units) goes on, 24 (1.5 units) stops
    assert V.adaptive_rule(n, s, q, 2, TOP, tol) == (tol <= 1)
    assert not V.adaptive_rule(n, s, q, 2, n, tol)                # n == max stops whatever the spread


def _threshold_states(tol, n):
    """(S, Q) pairs of n samples whose spread 256 * (nQ - S^2) lies one below, at and one above tol^2 n^2 (n - 1)"""
    rhs = tol * tol * n * n * (n - 1)
    out = []
    # samples: n - 1 of value a, one of value a + d -> nQ - S^2 = (n - 1) * d^2; vary d around the threshold
    for d in range(0, 766):
        lhs = 256 * (n - 1) * d * d
        if abs(lhs - rhs) <= 256 * (n - 1) * (2 * d + 1):
            a = 0
            if a + d <= 765:
                out.append((n, (n - 1) * a + a + d, (n - 1) * a * a + (a + d) ** 2))
    return out


@pytest.mark.parametrize("tol", [1, 16, 24, 200, 4096])
def test_probe_one_either_side_of_the_threshold(V, tol):
    seen = {True: 0, False: 0}
    for n in (2, 3, 4, 16, 17, 255, 4096, 65536, TOP - 1):
        rhs = tol * tol * n * n * (n - 1)
        # exact states near the threshold from two-valued samples
        for n_, s, q in _threshold_states(tol, n):
            want = _py_rule(n_, s, q, 2, TOP, tol)
            assert V.adaptive_rule(n_, s, q, 2, TOP, tol) == want
            seen[want] += 1
        # and synthetic (S, Q) with n*Q - S^2 = floor(rhs / 256) + {-1, 0, +1}: one either side of the strict comparison
        s = 382 * n
        for delta in (-1, 0, 1):
            spread = rhs // 256 + delta
            if spread < 0 or (s * s + spread) % n:
                base = s * s + spread
                q = -(-base // n)           # the smallest Q with nQ - S^2 >= spread
            else:
                q = (s * s + spread) // n
            if n * q - s * s < 0 or q > 765 * 765 * n:   # states that n samples of L in [0, 765] cannot reach
                continue
            want = _py_rule(n, s, q, 2, TOP, tol)
            assert V.adaptive_rule(n, s, q, 2, TOP, tol) == want, (n, s, q, tol)
            seen[want] += 1
    assert seen[True] and seen[False]


def test_probe_min_and_max(V):
    n, s, q = _const(5, 300)
    assert V.adaptive_rule(n, s, q, 6, 10, 0)          # below min: active whatever the spread
    assert not V.adaptive_rule(n, s, q, 5, 10, 0)      # at min, all samples identical: stopped
    assert not V.adaptive_rule(5, 300 * 4 + 301, 300 * 300 * 4 + 301 * 301, 5, 5, 0)   # n == max: stopped
    assert V.adaptive_rule(5, 300 * 4 + 301, 300 * 300 * 4 + 301 * 301, 5, 6, 0)       # one byte differs, tol 0: active


def test_tolerance_in_words():
    # the standard error of the mean of L against tol / 16: for n samples with variance v (population), the rule is
    # 256 * n * (n * v) > tol^2 * n^2 * (n - 1), i.e. v / (n - 1) > (tol / 16)^2
    for n in (4, 16, 64):
        for tol in (8, 16, 160):
            # half 0, half d: population variance d^2 / 4
            for d in range(0, 766, 5):
                s, q = (n // 2) * d, (n // 2) * d * d
                want = (d * d / 4) / (n - 1) > (tol / 16) ** 2
                if abs((d * d / 4) / (n - 1) - (tol / 16) ** 2) > 1e-9:
                    assert A.active(n, s, q, 2, 1 << 24, tol) == want


# ---- rounds on the checkers' samples ----

@pytest.fixture(scope="module")
def frames(J, O, V, product_scenes):
    """16 jittered samples (from 5) of a small VRT_MODE_FULL dragon frame and of mode 0, from tests/oracle_jitter.c"""
    tex, dim = product_scenes["dragon"]
    W, H = 24, 16
    ip, iv, cp, _ = V.camera_block((63.5, 60.5, 140.5), -90.0, -10.0, W, H)
    scene = O.make_scene(tex, dim, ip, iv, cp)
    out = {}
    for mode in (0, 2):
        out[mode] = {k: oracle_jitter.render(J, scene, W, H, mode, k)[0] for k in range(5, 5 + 16)}
    return W, H, out


def _plain(frames_by_k, ks):
    s = sum(frames_by_k[k][..., :3].astype(np.int64) for k in ks)
    n = len(ks)
    out = np.full(s.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = ((s + n // 2) // n).astype(np.uint8)
    return out


@pytest.mark.parametrize("mode", [0, 2])
def test_min_equal_max_is_the_plain_accumulation(frames, mode):
    W, H, fr = frames
    for N in (2, 5, 16):
        st = A.accumulate(lambda k: fr[mode][k], H, W, 5, 16, (N, N, 0))
        assert (st.counts() == N).all()
        assert np.array_equal(st.resolve(), _plain(fr[mode], range(5, 5 + N)))


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("tol", [0, 24, 200])
def test_rounds_on_checker_samples(frames, mode, tol):
    W, H, fr = frames
    rule = (2, 12, tol)
    st = A.accumulate(lambda k: fr[mode][k], H, W, 5, 16, rule)
    c = st.counts()
    assert c.min() >= 2 and c.max() <= 12
    # each pixel's samples are a prefix: the pixel stopped at the first count where the rule failed, and its sums are the
    # plain sums of samples 5 .. 5 + c - 1
    for y in range(H):
        for x in range(W):
            n = int(c[y, x])
            Ls = [int(fr[mode][k][y, x, :3].astype(np.int64).sum()) for k in range(5, 5 + n)]
            for m in range(2, n):
                assert A.active(m, sum(Ls[:m]), sum(v * v for v in Ls[:m]), *rule)
            assert n == 12 or not A.active(n, sum(Ls), sum(v * v for v in Ls), *rule)
            want = sum(fr[mode][k][y, x, :3].astype(np.int64) for k in range(5, 5 + n))
            assert list(st.sums[y, x]) == [int(v) for v in want]
    if tol == 0:
        # tolerance 0: a pixel whose first two samples agree and whose later ones never differ stops at 2
        flat = np.all(np.stack([fr[mode][k] for k in range(5, 5 + 16)]) == fr[mode][5], axis=(0, 3))
        assert (c[flat] == 2).all()
    if tol == 200:
        assert (c < 12).any()


def test_chunking_is_the_same_rounds(frames):
    W, H, fr = frames
    rule = (3, 16, 24)
    whole = A.accumulate(lambda k: fr[2][k], H, W, 5, 16, rule)
    st = A.State(H, W)
    k = 5
    for chunk in (3, 5, 8):
        for _ in range(chunk):
            st.add_round(fr[2][k], rule)
            k += 1
    assert np.array_equal(st.counts(), whole.counts()) and np.array_equal(st.resolve(), whole.resolve())


# ---- exports, argument checks ----

def test_library_exports_the_adaptive_calls(V):
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"vrt_accum_begin_adaptive", "vrt_accum_counts"} <= names
    assert "vrt_test_adaptive_rule" not in names and "vrt_test_adaptive_rule_device" not in names
    header = open(os.path.join(os.path.dirname(os.path.dirname(V.HIP_LIB)), "include", "vrt.h")).read()
    assert "int vrt_accum_begin_adaptive(" in header and "int vrt_accum_counts(" in header


def _unopened(V):
    # a Context whose vrt_create never ran: a wrapper that reached the library would fail on the missing handle
    return object.__new__(V.Context)


@pytest.mark.parametrize("adaptive", [(1, 8, 0), (0, 8, 0), (9, 8, 0), (2, TOP + 1, 0), (2, 8, -1), (2, 8, 65536), (2, 8),
                                      (2, 8, 0, 1), 5, "2,8,0", (2.0, 8, 0), (2, True, 0), (2, 8, None), [2, 8, 1.5]])
def test_accum_begin_rejects_bad_rules_before_the_device(V, adaptive):
    with pytest.raises(ValueError):
        _unopened(V).accum_begin(16, 16, 0, mode=V.MODE_FULL, adaptive=adaptive)


def test_accum_counts_needs_an_accumulation(V):
    with pytest.raises(V.VrtError):
        _unopened(V).accum_counts()
