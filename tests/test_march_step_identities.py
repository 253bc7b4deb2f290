"""The floating-point identities the v4 march step relies on (csrc/vrt_kernels_v4.hip.h: planes(), axis_of(), dda_step()),
checked on the CPU with numpy float32 over the whole reachable range, exhaustively where that is feasible.

* planes(): a node's planes as ((p >> t) + dpos) << t in integers, converted once, equal bit for bit the float form
  (floor(floor(x) * 2^-t) + dposf) * 2^t the kernel used before, +0 included, for every integer cell coordinate p a
  lookup can see and every node size 2^t.
* axis_of(): the exit axis read off the selected floats (t, m, tz) by comparing bits equals the axis taken from the
  comparisons tx < m and ty < tz, ties, signed zeros, infinities and NaN included.
"""
import itertools

import numpy as np

# cell coordinates: the world is sign-extended from bit 11, so |p| < 2^11; the check covers 32 times that
P = np.arange(-(1 << 16), 1 << 16, dtype=np.int32)
T_MAX = 16   # node sides up to 2^16 (the world's root is 2^12)


def _float_planes(p, dpos, t):
    pf = p.astype(np.float32)   # floor(x) of a ray position: integer-valued
    side = np.float32(2.0 ** t)
    inv_side = np.float32(2.0 ** -t)
    dposf = np.float32(1.0 if dpos else 0.0)
    with np.errstate(all="ignore"):
        return ((np.floor(pf * inv_side) + dposf) * side).astype(np.float32)


def _int_planes(p, dpos, t):
    q = ((p >> np.int32(t)) + np.int32(dpos)).astype(np.uint32) << np.uint32(t)
    return q.view(np.int32).astype(np.float32)


def test_planes_integer_form_equals_float_form():
    for t in range(T_MAX + 1):
        for dpos in (0, 1):
            a = _float_planes(P, dpos, t)
            b = _int_planes(P, dpos, t)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (t, dpos)


def test_planes_have_no_negative_zero():
    # the float form gives +0 where floor(p * 2^-t) + dposf is 0: -0 + 0 and -1 + 1 round to +0 in round-to-nearest
    for t in range(T_MAX + 1):
        for dpos in (0, 1):
            a = _float_planes(P, dpos, t)
            assert not np.any(a.view(np.uint32) == 0x80000000), (t, dpos)


def test_planes_bracket_the_cell():
    # the plane a ray leaves through is the node's far face in its direction: p lies in [plane - side, plane) for
    # dpos = 1 and in [plane, plane + side) for dpos = 0
    for t in range(T_MAX + 1):
        side = 1 << t
        hi = _int_planes(P, 1, t).astype(np.int64)
        lo = _int_planes(P, 0, t).astype(np.int64)
        assert np.all(hi - side == lo)
        assert np.all((lo <= P) & (P < hi))


def _select(c, a, b):   # v_cndmask_b32 c ? a : b, bits copied
    return np.where(c, a.view(np.uint32), b.view(np.uint32)).view(np.float32)


def _axis_both(tx, ty, tz):
    with np.errstate(invalid="ignore"):
        myz = ty < tz
        m = _select(myz, ty, tz)
        mx = tx < m
        t = _select(mx, tx, m)
    ref = np.where(mx, 0, np.where(myz, 1, 2))
    tb, mb, zb = t.view(np.uint32), m.view(np.uint32), tz.view(np.uint32)
    new = np.where(tb != mb, 0, np.where(mb != zb, 1, 2))
    return ref, new


SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 1e-8, -1e-8, 1e20, -1e20, 3.4028235e38, -3.4028235e38, np.inf, -np.inf,
                    np.nan, 1e-45, -1e-45, 1.17549435e-38, 2.0, 0.99999994, 1.0000001], dtype=np.float32)


def test_axis_from_bits_special_values_exhaustive():
    trip = np.array(list(itertools.product(range(len(SPECIAL)), repeat=3)))
    tx, ty, tz = SPECIAL[trip[:, 0]], SPECIAL[trip[:, 1]], SPECIAL[trip[:, 2]]
    ref, new = _axis_both(tx, ty, tz)
    assert np.array_equal(ref, new)


def test_axis_from_bits_ties_and_random():
    rng = np.random.default_rng(7)
    n = 1 << 20
    base = rng.uniform(-4.0, 4.0, n).astype(np.float32)
    # corner ties: two or three of the distances equal, or one ulp apart
    ulp = np.nextafter(base, np.float32(np.inf)).astype(np.float32)
    pick = rng.integers(0, 4, (3, n))
    cand = np.stack([base, ulp, rng.uniform(-4.0, 4.0, n).astype(np.float32), -base])
    tx, ty, tz = (cand[pick[k], np.arange(n)] for k in range(3))
    ref, new = _axis_both(tx, ty, tz)
    assert np.array_equal(ref, new)
    # every 32-bit pattern class: random bits (NaNs, subnormals, infinities)
    bits = rng.integers(0, 1 << 32, (3, n), dtype=np.uint64).astype(np.uint32)
    ref, new = _axis_both(*(b.view(np.float32) for b in bits))
    assert np.array_equal(ref, new)


def test_ray_positions_floor_sign():
    # floor_i(): one v_cvt_flr_i32_f32 replaces v_floor_f32 + v_cvt_i32_f32. On the CPU side the claim is the
    # mathematical one the device probe (test_gpu_march_step.py) confirms on the hardware: floor then truncate of an
    # integer-valued float is floor, for negative values, -0 and values below one ulp of an integer alike
    x = np.array([-0.0, 0.0, -1e-45, 1e-45, -1e-40, -0.5, -1.0, -1.0000001, -0.99999994, 2047.9999, -2048.0001,
                  16777215.0, -16777215.0], dtype=np.float32)
    assert np.array_equal(np.floor(x).astype(np.int64), np.floor(x.astype(np.float64)).astype(np.int64))
