"""The temporal pass restated in scalar C (tests/oracle_temporal.c) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_temporal.c as tests/oracle_filter_var.py compiles its library; the C file includes that one's, so the
library holds everything oracle_filter_var's holds and oracle_filter_var.filter() takes it too. temporal() is include/vrt.h
vrt_temporal_hdr T1-T6, chain() the accumulation forms' chain (the pass, then the variance-guided filter on its outputs).
position64() and integrate64() restate the rule in float64 numpy in two stages, each with a running bound on the checker's float32
error (class E: one EPS per float32 operation, carried through every operation, first order); PLANT names the checker's planted
misreadings."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_filter_hdr as F
import oracle_filter_var as FV
import oracle_hdr

PLANT = {None: 0, "offset_kept": 1, "not_renormalised": 2, "zexp_from_current_eye": 3, "variance_of_one_sample": 4}
EPS = F.EPS
VAR_MAX = FV.VAR_MAX
HISTORY_FLOATS = 12          # per pixel: three planes of four


class Temporal(C.Structure):
    """include/vrt.h vrt_temporal"""
    _fields_ = [("prev_view_proj", C.c_float * 16), ("prev_camera_pos", C.c_float * 4), ("offset_x", C.c_float), ("offset_y", C.c_float),
                ("max_history", C.c_int32), ("alpha_min", C.c_float), ("alpha_moments_min", C.c_float), ("normal_min", C.c_float),
                ("depth_tol", C.c_float)]


def make(prev_view_proj=None, prev_camera_pos=None, offset=(0.0, 0.0), max_history=8, alpha_min=0.4, alpha_moments_min=0.6, normal_min=0.0,
         depth_tol=0.4):
    t = Temporal()
    if prev_view_proj is not None:
        t.prev_view_proj[:] = [float(v) for v in np.asarray(prev_view_proj, np.float32).reshape(16)]
    if prev_camera_pos is not None:
        t.prev_camera_pos[:3] = [float(v) for v in np.asarray(prev_camera_pos, np.float32).reshape(-1)[:3]]
    t.offset_x, t.offset_y = float(offset[0]), float(offset[1])
    t.max_history = int(max_history)
    t.alpha_min, t.alpha_moments_min, t.normal_min, t.depth_tol = alpha_min, alpha_moments_min, normal_min, depth_tol
    return t


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_temporal.so")
    srcs = [os.path.join(oracle_hdr.ROOT, "tests", "oracle_temporal.c")] + [os.path.join(oracle_hdr.ORACLE, f) for f in
                                                                           ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *oracle_hdr.CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = F._declare_base(C.CDLL(out))
    L.o_filter_hdr.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.POINTER(F.Filter), C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 3
    L.o_filter_hdr.restype = C.c_int
    L.o_filter_guide.argtypes = [C.c_float]
    L.o_filter_guide.restype = C.c_float
    L.o_filter_var.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.POINTER(FV.FilterVar), C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 5
    L.o_filter_var.restype = C.c_int
    L.o_filter_var_value.argtypes = [C.c_float]
    L.o_filter_var_value.restype = C.c_float
    L.o_temporal.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_int, C.POINTER(Temporal), C.c_int] + [C.c_void_p] * 4
    L.o_temporal.restype = None
    return L


def _camera(cam):
    ip, iv, cp = (np.ascontiguousarray(v, np.float32).reshape(-1) for v in cam[:3])
    assert ip.size == 16 and iv.size == 16 and cp.size >= 3
    return ip, iv, np.ascontiguousarray(np.resize(cp, 4), np.float32)


def _planes(rgb, g):
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    n, z, c = (np.ascontiguousarray(g[k], np.float32) for k in ("normal", "depth", "coverage"))
    assert rgb.shape == (h, w, 3) and n.shape == (h, w, 3) and z.shape == (h, w) and c.shape == (h, w)
    return rgb, n, z, c


def temporal(L, cam, rgb, guides, history, t, plant=None, details=False):
    """cam (inv_projection, inv_view, camera_pos), rgb float32[H,W,3], guides with "normal", "depth", "coverage", history
    float32[3,H,W,4] or None, t a Temporal -> (history float32[3,H,W,4], integrated float32[H,W,3], variance float32[H,W]) and, with
    details, float32[H,W,8]: fx, fy, Zexp, the four tap verdicts, sw"""
    ip, iv, cp = _camera(cam)
    rgb, n, z, c = _planes(rgb, guides)
    h, w = rgb.shape[:2]
    if history is not None:
        history = np.ascontiguousarray(history, np.float32)
        assert history.shape == (3, h, w, 4)
    out_h, out, outv = np.zeros((3, h, w, 4), np.float32), np.zeros_like(rgb), np.zeros((h, w), np.float32)
    det = np.zeros((h, w, 8), np.float32)
    L.o_temporal(ip.ctypes.data, iv.ctypes.data, cp.ctypes.data, rgb.ctypes.data, n.ctypes.data, z.ctypes.data, c.ctypes.data,
                 history.ctypes.data if history is not None else None, w, h, C.byref(t), PLANT[plant], out_h.ctypes.data, out.ctypes.data,
                 outv.ctypes.data, det.ctypes.data)
    return (out_h, out, outv, det) if details else (out_h, out, outv)


def chain(L, cam, mean, guides, history, t, f, op="clamp", exposure=1.0):
    """vrt_accum_resolve_hdr_temporal on the checker's own mean and planes -> (history, integrated, filtered rgb, rgba8, variance)"""
    hist, integ, var = temporal(L, cam, mean, guides, history, t)
    rgb, rgba, outv = FV.filter(L, integ, guides, f, var, op, exposure)
    return hist, integ, rgb, rgba, outv


def view_proj(inv_proj, inv_view):
    """the forward projection * view of a camera block: the float64 inverse of inv_projection times the float64 inverse of inv_view,
    rounded once to float32 (column-major, as the block's matrices are)"""
    ip = np.asarray(inv_proj, np.float64).reshape(4, 4).T
    iv = np.asarray(inv_view, np.float64).reshape(4, 4).T
    return np.ascontiguousarray((np.linalg.inv(ip) @ np.linalg.inv(iv)).T.reshape(16).astype(np.float32))


# ---- float64 restatements with their bounds ------------------------------------------------------------------------------------------
class E:
    """A float64 value with an absolute bound on the error of the float32 evaluation of the same expression: every operation adds
    one rounding, EPS times its result, to what its operands' errors become (first order; the callers put 1.1 in front)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) + e

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    def _rounded(self, v, e):
        return E(v, e + EPS * np.abs(v))

    def __add__(self, o):
        o = E.of(o)
        return self._rounded(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = E.of(o)
        return self._rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return E.of(o) - self

    def __mul__(self, o):
        o = E.of(o)
        return self._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.of(o)
        v = self.v / o.v
        return self._rounded(v, (self.e + np.abs(v) * o.e) / np.maximum(np.abs(o.v) - o.e, 1e-300))

    def __rtruediv__(self, o):
        return E.of(o) / self

    def sqrt(self):
        v = np.sqrt(self.v)
        return self._rounded(v, self.e / np.maximum(v + np.sqrt(np.maximum(self.v - self.e, 0.0)), 1e-300))

    def abs(self):
        return E(np.abs(self.v), self.e)

    def at_least(self, c):
        """max with an exact constant: 1-Lipschitz, the bound stays"""
        return E(np.maximum(self.v, c), self.e)

    def at_most(self, c):
        return E(np.minimum(self.v, c), self.e)

    def where(self, cond, other):
        other = E.of(other)
        return E(np.where(cond, self.v, other.v), np.where(cond, self.e, other.e))


def _mat_vec(m, x, y, z, w):
    """mat_vec's order on a column-major float32 matrix -> four E"""
    m = np.asarray(m, np.float64).reshape(16)
    return [(float(m[r]) * x + float(m[4 + r]) * y) + (float(m[8 + r]) * z + float(m[12 + r]) * w) for r in range(4)]


def _normalize(v):
    inv = 1.0 / ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]).sqrt()
    return [v[0] * inv, v[1] * inv, v[2] * inv]


def _rays(ip, iv, w, h, offset):
    """T1's direction of every pixel's ray -> three E [H,W]"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    one = np.ones((h, w))
    fxp, fyp = E(xs) + float(np.float32(offset[0])), E(ys) + float(np.float32(offset[1]))
    u, v = (fxp / float(w)) * 2.0 - 1.0, (fyp / float(h)) * 2.0 - 1.0
    view = _mat_vec(ip, u, v, E(-one), E(one))
    persp = np.abs(view[3].v) > 1e-6
    view = [(c / view[3]).where(persp, c) for c in view[:3]]
    vd = _normalize(view)
    wd = _mat_vec(iv, vd[0], vd[1], vd[2], E(0.0 * one))
    return _normalize(_normalize(wd[:3]))


def rays64(cam, w, h, offset=(0.0, 0.0)):
    """the float64 directions float64[H,W,3] of the rays through every pixel at `offset`: what a test builds a scene's planes from"""
    ip, iv, _ = _camera(cam)
    return np.stack([c.v for c in _rays(ip, iv, w, h, offset)], axis=2)


def position64(cam, guides, t):
    """Stage one: T1-T2 in float64 on the float32 inputs -> (fx, fy, Zexp) as E [H,W], and reached: where clip.w > 1e-6 by more than
    its own bound. The bounds come from T1-T2's operations one by one: the pixel's position, u and v, two mat_vec, the perspective
    divide, three normalisations, P, the projection, its divide, the map to pixels, and the root of Zexp."""
    ip, iv, cp = _camera(cam)
    z = F.g_of(guides["depth"]).astype(np.float64)
    h, w = z.shape
    d = _rays(ip, iv, w, h, (t.offset_x, t.offset_y))
    P = [float(cp[i]) + E(z) * d[i] for i in range(3)]
    clip = _mat_vec(np.ctypeslib.as_array(t.prev_view_proj), P[0], P[1], P[2], E(np.ones_like(z)))
    old = np.seterr(all="ignore")
    fx = (((clip[0] / clip[3]) + 1.0) * 0.5) * float(w) - float(np.float32(t.offset_x))
    fy = (((clip[1] / clip[3]) + 1.0) * 0.5) * float(h) - float(np.float32(t.offset_y))
    np.seterr(**old)
    dp = [P[i] - float(t.prev_camera_pos[i]) for i in range(3)]
    zexp = ((dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2]).sqrt()
    return fx, fy, zexp, clip[3].v - 1.1 * clip[3].e > 1e-6


def lum64(c):
    return (FV.LUMA[0] * c[0] + FV.LUMA[1] * c[1]) + FV.LUMA[2] * c[2]


def integrate64(rgb, guides, history, t, det):
    """Stage two: T3-T6 in float64 on the float32 inputs and on the checker's own float32 fx, fy and Zexp (det: its details) ->
    (history float64[3,H,W,4], variance float64[H,W], a bound on each, unsure bool[H,W]). unsure marks the pixels where a tap test,
    sw > 0 or N' >= 2 has a margin inside its own bound: they are left out of the comparison, and the caller states their share."""
    rgb, n, z, c = _planes(rgb, guides)
    h, w = z.shape
    hc = [F.h_of(rgb[..., k]).astype(np.float64).reshape(-1) for k in range(3)]
    Np = [F.g_of(n[..., k]).astype(np.float64).reshape(-1) for k in range(3)]
    Zp, Cp = F.g_of(z).astype(np.float64).reshape(-1), F.g_of(c).astype(np.float64).reshape(-1)
    live = Cp > 0
    fx, fy, zexp = (det[..., k].astype(np.float64).reshape(-1) for k in range(3))
    nmax = float(t.max_history)
    inside = live & (fx > -1) & (fx < w) & (fy > -1) & (fy < h) if history is not None else np.zeros(h * w, bool)
    # a pixel the checker never reached T2 for has fx = fy = 0 in its details and sw = 0: its taps are taken as failing below
    reached = (det[..., 2].reshape(-1) != 0) | (det[..., 7].reshape(-1) != 0) | (det[..., 3:7].reshape(-1, 4).any(axis=1))
    inside &= reached
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = E(fx) - x0, E(fy) - y0
    wts = [(1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty]
    unsure = np.zeros(h * w, bool)
    zero = E(np.zeros(h * w))
    sw, sc, sn, s1, s2 = zero, [zero, zero, zero], zero, zero, zero
    tol = float(np.float32(t.depth_tol)) * E(zexp) + 2.0 ** -20
    if history is not None:
        H0, H1, H2 = (np.asarray(history[k], np.float32).reshape(-1, 4) for k in range(3))
        for k in range(4):
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            ok = inside & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            q = np.where(ok, qy * w + qx, 0).astype(np.int64)
            Nq = np.minimum(np.maximum(F.g_of(H0[q, 3]).astype(np.float64), 0.0), nmax)
            Zq, Cq = F.g_of(H1[q, 2]).astype(np.float64), F.g_of(H1[q, 3]).astype(np.float64)
            nq = [F.g_of(H2[q, j]).astype(np.float64) for j in range(3)]
            nd = (E(nq[0]) * Np[0] + E(nq[1]) * Np[1]) + E(nq[2]) * Np[2]
            dz = (E(Zq) - zexp).abs()
            ok = ok & (Cq > 0) & (Nq >= 1)
            n_margin, z_margin = nd.v - float(np.float32(t.normal_min)), tol.v - dz.v
            # (a dot product of axis normals is exact, bound 0: its decision is sure even on the threshold)
            unsure |= ok & (((np.abs(n_margin) <= 1.1 * nd.e) & (nd.e > 0)) | (np.abs(z_margin) <= 1.1 * (tol.e + dz.e)))
            ok = ok & (n_margin >= 0) & (z_margin >= 0)
            wk = wts[k]
            add = lambda s, xq: (s + wk * xq).where(ok, s)   # noqa: E731
            sw = (sw + wk).where(ok, sw)
            sc = [add(sc[j], F.h_of(H0[q, j]).astype(np.float64)) for j in range(3)]
            sn = add(sn, Nq)
            s1 = add(s1, F.h_of(H1[q, 0]).astype(np.float64))
            s2 = add(s2, FV.hv_of(H1[q, 1]).astype(np.float64))
    have = sw.v > 0
    unsure |= inside & (np.abs(sw.v) <= 1.1 * sw.e) & (sw.e > 0)
    old = np.seterr(all="ignore")
    den = sw.where(have, E(np.ones(h * w)))
    prev = lambda s: (s / den).where(have, zero)   # noqa: E731
    cp, nprev, m1p, m2p = [prev(s) for s in sc], prev(sn), prev(s1), prev(s2)
    nn = (nprev + 1.0).at_most(nmax)
    inv = 1.0 / nn
    a, am = inv.at_least(float(np.float32(t.alpha_min))), inv.at_least(float(np.float32(t.alpha_moments_min)))
    cn = [cp[j] + a * (E(hc[j]) - cp[j]) for j in range(3)]
    Y = lum64([E(hc[j]) for j in range(3)])
    m1, m2 = m1p + am * (Y - m1p), m2p + am * (Y * Y - m2p)
    spread = (m2 - m1 * m1).at_least(0.0)
    var = (spread / (nn - 1.0).where(nn.v >= 2, E(np.ones(h * w)))).at_most(float(VAR_MAX))
    var = var.where(nn.v >= 2, E(np.full(h * w, float(VAR_MAX))))
    unsure |= live & (np.abs(nn.v - 2.0) <= 1.1 * nn.e) & (nn.e > 0)
    np.seterr(**old)
    dead = ~live
    out = np.zeros((3, h * w, 4))
    err = np.zeros((3, h * w, 4))
    for j in range(3):
        out[0, :, j], err[0, :, j] = np.where(dead, hc[j], cn[j].v), np.where(dead, 0.0, cn[j].e)
        out[2, :, j] = np.where(dead, 0.0, Np[j])
    out[0, :, 3], err[0, :, 3] = np.where(dead, 0.0, nn.v), np.where(dead, 0.0, nn.e)
    out[1, :, 0], err[1, :, 0] = np.where(dead, 0.0, m1.v), np.where(dead, 0.0, m1.e)
    out[1, :, 1], err[1, :, 1] = np.where(dead, 0.0, m2.v), np.where(dead, 0.0, m2.e)
    out[1, :, 2], out[1, :, 3] = np.where(dead, 0.0, Zp), np.where(dead, 0.0, Cp)
    return (out.reshape(3, h, w, 4), np.where(dead, 0.0, var.v).reshape(h, w), 1.1 * err.reshape(3, h, w, 4) + 1e-30,
            (1.1 * np.where(dead, 0.0, var.e) + 1e-30).reshape(h, w), unsure.reshape(h, w))


same = F.same
