"""The rebuilt v4 march step on the device against the arithmetic it replaced (csrc/test/vrt_test.hip march_step_probe_kernel):
the position after one DDA step, its floor as integers, the exit axis and the planes of the node there, bit for bit, on
adversarial rays -- corner ties, axis-parallel rays, direction components in (-1e-8, 0], positions on node faces,
negative coordinates and signed zeros."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run(V, rp, plane, d, inv, push, t, dpos):
    L = V.test_lib()
    L.vrt_test_march_step.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    n = len(rp)
    inp = np.zeros((n, 16), np.float32)
    inp[:, 0:3], inp[:, 3:6], inp[:, 6:9], inp[:, 9:12], inp[:, 12:15] = rp, plane, d, inv, push
    inp[:, 15] = t.astype(np.uint32).view(np.float32)
    dp = np.ascontiguousarray(dpos.astype(np.int32))
    out = np.zeros((n, 20), np.uint32)
    assert L.vrt_test_march_step(0, inp.ctypes.data, dp.ctypes.data, out.ctypes.data, n) == 0
    return out[:, :10], out[:, 10:]


def _rays(rng, n, d):
    """Rays set up as march() does: inv with the shader's 1e-8 rule, push of the direction's sign, planes of the node of
    side 2^t around the position."""
    d = d.astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(np.abs(d) < np.float32(1e-8), np.float32(1e20), np.float32(1.0) / d).astype(np.float32)
    sgn = np.where(d > 0, 1.0, np.where(d < 0, -1.0, 0.0)).astype(np.float32)
    push = (sgn * np.float32(0.0001)).astype(np.float32)
    dpos = (d > 0).astype(np.int32)
    t = rng.integers(0, 8, n)
    return inv, push, dpos, t


def _planes_of(rp, dpos, t):
    p = np.floor(rp).astype(np.int64)
    side = (1 << t)[:, None]
    return (((p >> t[:, None]) + dpos) * side).astype(np.float32)


def _check(new, old, mp_ok):
    assert np.array_equal(new[:, 0:3], old[:, 0:3]), "position after the step"
    assert np.array_equal(new[:, 3:6], old[:, 3:6]), "floor of the position"
    assert np.array_equal(new[:, 6], old[:, 6]), "exit axis"
    assert np.array_equal(new[mp_ok, 7:10], old[mp_ok, 7:10]), "node planes"


def _in_world(out):
    # find() makes planes only for a cell in the world; a position far outside ends the ray at that lookup instead
    mp = out[:, 3:6].view(np.int32).astype(np.int64)
    return np.all(np.abs(mp) < (1 << 20), axis=1)


def _unit(v):
    v = v.astype(np.float32)
    return (v / np.sqrt((v.astype(np.float64) ** 2).sum(1))[:, None]).astype(np.float32)


def test_step_random_and_face_positions(V):
    rng = np.random.default_rng(11)
    n = 1 << 16
    d = _unit(rng.normal(size=(n, 3)))
    inv, push, dpos, t = _rays(rng, n, d)
    rp = rng.uniform(-2048, 2048, (n, 3)).astype(np.float32)
    # a third of the positions exactly on a node face (the eye on a face, a step that landed on one)
    face = rng.random((n, 3)) < 0.33
    side = (1 << t)[:, None]
    rp = np.where(face, (np.floor(rp / side) * side).astype(np.float32), rp).astype(np.float32)
    plane = _planes_of(rp, dpos, t)
    new, old = _run(V, rp, plane, d, inv, push, t, dpos)
    _check(new, old, _in_world(new))


def test_step_corner_ties(V):
    # tx == ty == tz (and pairs): |d| equal on the tied axes and the position equally far from the tied planes
    rng = np.random.default_rng(12)
    n = 1 << 15
    s = rng.choice([-1.0, 1.0], (n, 3)).astype(np.float32)
    pair = rng.integers(0, 4, n)
    d = s.copy()
    d[pair == 1, 0] *= 2.0
    d[pair == 2, 1] *= 2.0
    d[pair == 3, 2] *= 2.0
    d = _unit(d)
    inv, push, dpos, t = _rays(rng, n, d)
    side = (1 << t).astype(np.float32)[:, None]
    cell = np.floor(rng.uniform(-64, 64, (n, 3))).astype(np.float32) * side
    f = rng.choice([0.25, 0.5, 0.75], n).astype(np.float32)[:, None] * side
    rp = np.where(dpos == 1, cell + side - f, cell + f).astype(np.float32)
    plane = _planes_of(rp, dpos, t)
    new, old = _run(V, rp, plane, d, inv, push, t, dpos)
    _check(new, old, _in_world(new))
    assert set(np.unique(new[:, 6])) <= {0, 1, 2}


def test_step_axis_parallel_and_backward_components(V):
    # components 0, -0 and in (-1e-8, 0] (their reciprocal is replaced by 1e20 while their plane is the near face: the
    # step can go backwards), and tiny positive ones
    rng = np.random.default_rng(13)
    n = 1 << 15
    tiny = np.array([0.0, -0.0, -1e-9, -5e-9, -9.99e-9, -1e-8, 1e-9, 1e-30, -1e-30, -1e-45], np.float32)
    d = _unit(rng.normal(size=(n, 3)))
    k = rng.integers(0, 3, n)
    d[np.arange(n), k] = tiny[rng.integers(0, len(tiny), n)]
    k2 = (k + 1 + rng.integers(0, 2, n)) % 3
    two = rng.random(n) < 0.3
    d[np.arange(n)[two], k2[two]] = tiny[rng.integers(0, len(tiny), two.sum())]
    inv, push, dpos, t = _rays(rng, n, d)
    rp = rng.uniform(-256, 256, (n, 3)).astype(np.float32)
    # positions near 0 from both sides: the floor of -tiny is -1
    near0 = rng.random((n, 3)) < 0.2
    rp = np.where(near0, rng.choice(np.array([-0.0, 0.0, -1e-40, 1e-40, -1e-7, 1e-7], np.float32), (n, 3)), rp).astype(np.float32)
    plane = _planes_of(rp, dpos, t)
    new, old = _run(V, rp, plane, d, inv, push, t, dpos)
    _check(new, old, _in_world(new))


def test_floor_conversion_matches_floor_then_convert(V):
    # floor_i(): v_cvt_flr_i32_f32 against v_floor_f32 + v_cvt_i32_f32 (math probe ops 13 and 3 / 7), infinities and
    # saturation included. Not NaN: there the two differ (the second gives 0), and a ray position is never NaN (see floor_i())
    L = V.test_lib()
    rng = np.random.default_rng(14)
    x = np.concatenate([rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        np.array([0.0, -0.0, -1e-45, 1e-45, -0.5, -1.0, -1.0000001, 2147483520.0, -2147483648.0, 3e9, -3e9,
                                  np.inf, -np.inf], np.float32)]).astype(np.float32)
    x = np.ascontiguousarray(x[~np.isnan(x)])
    y = np.zeros_like(x)
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    assert L.vrt_test_math(0, 13, x.ctypes.data, y.ctypes.data, a.ctypes.data, len(x)) == 0
    assert L.vrt_test_math(0, 3, x.ctypes.data, y.ctypes.data, b.ctypes.data, len(x)) == 0
    assert L.vrt_test_math(0, 7, b.ctypes.data, y.ctypes.data, c.ctypes.data, len(x)) == 0
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
