"""What the path depth, the sun disc and the emitter rules add to pathTrace, restated for tests/path_ref64.py (test helper,
not a test): the sun's basis and sampled direction, the emitter list with its integer weights and thresholds, and the
discrete choices of a connection.

Written from the text of include/vrt.h ("Sun disc", "Emitter sampling", "Emitter importance", "Emitter MIS") alone; numpy
and shader_ref64 only, nothing under oracle/, none of the checkers and nothing of the product
(tests/test_shader_reference64.py enforces that).

What is restated:
  * The basis of the sun (point 1): ll = |L|, Ln = L / ll, up by |Ln.z| < 0.999f, T = normalize(cross(up, Ln)),
    B = cross(Ln, T), in float64 from the float32 lightDir.
  * The concentric map (vrt_set_lens step 3, the one tests/lens_ref64.py restates for the lens) with lu = u1, lv = u2.
    There lu is a 24-bit integer and a = 2 lu - 1 is exact; here u1 is rand()'s float32 value and 2 u1 - 1 may round, so
    a and b are computed in np.float32 -- their inputs are exact float32 values, the float32 result is therefore defined,
    not bounded -- and a == b == 0 and |a| > |b| are decided on them. phi, cos, sin and the products are float64.
  * L' = normalize((Ln + (s dx) T) + (s dy) B) * ll (point 3).
  * The emitter list: the decoded leaves with alpha > 0 and illumination > 0, cubes as entries, other boxes as their unit
    cells, sorted by (lo.x, lo.y, lo.z); W_j = size^2 * illum * (R + G + B) and the thresholds T_j in Python integers.
  * The discrete choices of a connection in exact float32 arithmetic (their inputs are exact float32 values, as rand()
    is): j = min((int)(u0 * (float)N), N - 1), f = min((int)(uf * 6.0f), 5), t = min((uint32)(u0 * 2^24), 2^24 - 1),
    the threshold search, p = ticks * 2^-24, i = min((int)(uf * (float)m), m - 1). They are decided, never bounded.

Error model. sun_dir_err(s, ll) bounds the absolute float32 error of each component of L' (u = 2^-24):
  * Ln = normalize3(L) has relative error <= 4.5u per component (shader_ref64.GIVEN_DIR_ERR: dot, sqrt, reciprocal or
    quotient, product) and ll = len3(L) relative error <= 2.5u.
  * cross(up, Ln) with an axis `up` is made of exact copies, negations and zeros of Ln's float32 components, so its
    components carry Ln's 4.5u relative; normalising moves a unit vector by at most twice the relative error of its
    argument's length-scaled components (9u) and rounds (4.5u): e_T = 13.5u absolute (|T_i| <= 1).
  * B_i = Ln_a T_b - Ln_c T_d: each product is off by e_Ln + e_T + u (factors <= 1), the difference rounds once:
    e_B = 2 (4.5u + 13.5u + u) + u = 39u.
  * (dx, dy): lens_ref64's bound, |r| (E_SINCOS + PHI_ERR) + u |dx| <= e_d = E_SINCOS + 5u (|r| <= 1).
  * v_i = (Ln_i + (s dx) T_i) + (s dy) B_i with |s dx|, |s dy| <= s: s dx is off by s e_d + u s; the products add
    s e_T (s e_B) and u s; the two sums round relative to at most 1 + 2s each:
    e_v = 4.5u + 2 s (e_d + 2u) + s (e_T + e_B) + 2u (1 + 2s).
  * |v| >= 1 up to rounding (Ln is orthogonal to T and B). n = v / |v| moves by (I - n n^T) dv / |v|, and the projection
    does not lengthen a vector: each component by at most |dv|_2 <= sqrt(3) e_v; normalize3 adds 4.5u relative; the
    product with ll its 2.5u and one rounding: sun_dir_err = ll (sqrt(3) e_v + 8u).
    At s = 0.05 and ll = 1 that is 1.4e-6: 12u of roundings and 0.1 * E_SINCOS from the Cephes sin / cos, times sqrt(3).
The connection's bounds are derived where they are applied (path_ref64, "Emitter connections")."""
import numpy as np

import shader_ref64 as R

U = R.U
E_SINCOS = 1.2e-7           # absolute, det_sinf / det_cosf (path_ref64.E_SINCOS; measured there)
PHI_ERR = 4.0 * U           # lens_ref64.PHI_ERR, derived there
TICKS = 1 << 24
_F = np.float32


def sun_basis(light_dir):
    """point 1 -> (ll, Ln[3], T[3], B[3]) in float64 from the float32 lightDir"""
    L = np.array(light_dir, np.float32).astype(np.float64)[:3]
    ll = float(np.sqrt((L * L).sum()))
    Ln = L / ll
    up = np.array([0.0, 0.0, 1.0]) if abs(Ln[2]) < R._f32(0.999) else np.array([1.0, 0.0, 0.0])
    T = np.cross(up, Ln)
    T /= np.sqrt((T * T).sum())
    return ll, Ln, T, np.cross(Ln, T)


def sun_dir_err(s, ll):
    """the absolute bound on each float32 component of L' (module docstring)"""
    e_d = E_SINCOS + PHI_ERR + U
    e_v = 4.5 * U + 2.0 * s * (e_d + 2.0 * U) + s * (13.5 * U + 39.0 * U) + 2.0 * U * (1.0 + 2.0 * s)
    return ll * (np.sqrt(3.0) * e_v + 8.0 * U)


def disc_map(u1, u2):
    """the concentric map of vrt_set_lens step 3 with lu = u1, lv = u2 (float32 values held in float64) -> (dx, dy)"""
    a = (_F(2.0) * np.asarray(u1, np.float64).astype(_F) - _F(1.0)).astype(_F)
    b = (_F(2.0) * np.asarray(u2, np.float64).astype(_F) - _F(1.0)).astype(_F)
    assert a.dtype == _F and b.dtype == _F
    centre = (a == 0) & (b == 0)
    first = np.abs(a) > np.abs(b)
    a, b = a.astype(np.float64), b.astype(np.float64)
    c4, c2 = R._f32(0.785398163), R._f32(1.57079633)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(first, a, b)
        phi = np.where(first, c4 * (b / np.where(first, a, 1.0)), c2 - c4 * (a / np.where(first | centre, 1.0, b)))
    dx, dy = r * np.cos(phi), r * np.sin(phi)
    return np.where(centre, 0.0, dx), np.where(centre, 0.0, dy)


def sun_dirs(basis, s, u1, u2, flaws=()):
    """point 3 -> L'[n, 3]"""
    ll, Ln, T, B = basis
    dx, dy = disc_map(u1, u2)
    v = (Ln[None] + (s * dx)[:, None] * T[None]) + (s * dy)[:, None] * B[None]
    v /= np.sqrt((v * v).sum(1))[:, None]
    return v if "sun_unit_length" in flaws else v * ll


class Emitters:
    """the emitter list of a decoded World: lo[N, 3], size[N], node[N] (the World's leaf), W (Python integers), T (the
    thresholds, Python integers), total = Wtot, inv_power (the float32 of 1.0 / Wtot as float64, 0 at Wtot == 0)"""

    def __init__(self, world):
        w = world
        rows = []
        for i in np.nonzero(w.isleaf & (w.a > 0) & (w.p[:, 1] > 0))[0]:
            mn, mx = w.mn[i], w.mx[i]
            ext = mx - mn
            if ext.min() <= 0:
                continue
            if ext[0] == ext[1] == ext[2]:
                rows.append((int(mn[0]), int(mn[1]), int(mn[2]), int(ext[0]), int(i)))
            else:
                rows.extend((x, y, z, 1, int(i)) for x in range(mn[0], mx[0]) for y in range(mn[1], mx[1]) for z in range(mn[2], mx[2]))
        rows.sort(key=lambda e: e[:3])
        a = np.array(rows, np.int64).reshape(-1, 5)
        self.lo, self.size, self.node = a[:, :3], a[:, 3], a[:, 4]
        self.N = len(rows)
        self.W = [int(s) * int(s) * word_weight(w, n) for s, n in zip(self.size, self.node)]
        self.total = sum(self.W)
        self.T = thresholds(self.W)
        self.inv_power = float(np.float32(1.0 / float(self.total))) if self.total > 0 else 0.0

    def entries(self):
        """-> int64[N, 4]: {lo.x, lo.y, lo.z, size}"""
        return np.concatenate([self.lo, self.size[:, None]], 1)


def word_weight(world, node):
    """illum * (R + G + B) of a leaf's words as W_j reads them, a Python integer"""
    return int(world.p[node, 1]) * int(world.rgb[node].sum())


def thresholds(W):
    """T_j of "Emitter importance" in exact integers"""
    n, total = len(W), sum(W)
    out, c = [], 0
    for j, wj in enumerate(W):
        c += wj
        out.append((j + 1) + c * (TICKS - n) // total if total > 0 else (j + 1) * TICKS // n)
    return out


def _trunc32(x32):
    """(int) of a non-negative float32"""
    return np.floor(x32.astype(np.float64)).astype(np.int64)


def pick_uniform(u0, N):
    """j = min((int)(u0 * (float)N), N - 1)"""
    return np.minimum(_trunc32(u0.astype(_F) * _F(N)), N - 1)


def pick_power(u0, T):
    """-> (j, p): t = min((uint32)(u0 * 16777216.0f), 16777215), the smallest j with T_j > t, p = ticks * 2^-24"""
    t = np.minimum(_trunc32(u0.astype(_F) * _F(16777216.0)), TICKS - 1)
    Ta = np.array(T, np.int64)
    j = np.searchsorted(Ta, t, side="right")
    ticks = Ta[j] - np.where(j > 0, Ta[np.maximum(j - 1, 0)], 0)
    return j, ticks.astype(np.float64) * 2.0 ** -24


def pick_index(uf, m):
    """min((int)(uf * (float)m), m - 1) for m >= 1 (m = 6: the uniform rule's face)"""
    m = np.broadcast_to(np.asarray(m, np.int64), uf.shape)
    return np.minimum(_trunc32(uf.astype(_F) * m.astype(_F)), m - 1)
