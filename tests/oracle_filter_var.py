"""The variance-guided filter restated in scalar C (tests/oracle_filter_var.c) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_filter_var.c as tests/oracle_filter_hdr.py compiles its library; the C file includes that one's, so
the library holds everything oracle_filter_hdr's holds and oracle_filter_hdr.filter() takes it too. filter() is include/vrt.h
vrt_filter_hdr_var V1-V4; v0_64() and level64() restate V2 and one level of V3 in float64 numpy together with a first-order bound on
the checker's float32 error; PLANT names the checker's planted misreadings and "no_lum", the reduction to the guide-only filter."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_filter_hdr as F
import oracle_hdr

OPS = oracle_hdr.OPS
PLANT = {None: 0, "w_not_squared": 1, "vbar_spacing_1": 2, "no_ym": 3, "dl_remodulated": 4, "no_lum": 5}
EPS, E_EXP = F.EPS, F.E_EXP
VAR_MAX = np.float32(65504.0) * np.float32(65504.0)
G3 = np.array([[1 / 16, 1 / 8, 1 / 16], [1 / 8, 1 / 4, 1 / 8], [1 / 16, 1 / 8, 1 / 16]])
LUMA = tuple(float(np.float32(c)) for c in (0.2126, 0.7152, 0.0722))


class FilterVar(C.Structure):
    """include/vrt.h vrt_filter_var"""
    _fields_ = F.Filter._fields_ + [("sigma_lum", C.c_float)]


def make(levels, demodulate=True, sigma_normal=0.5, sigma_albedo=0.05, sigma_depth=2.0, sigma_lum=4.0):
    return FilterVar(int(levels), F.DEMODULATE if demodulate else 0, sigma_normal, sigma_albedo, sigma_depth, sigma_lum)


def guide_only(f):
    """the vrt_filter with f's levels, flags and guide sigmas"""
    return F.Filter(f.levels, f.flags, f.sigma_normal, f.sigma_albedo, f.sigma_depth)


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_filter_var.so")
    srcs = [os.path.join(oracle_hdr.ROOT, "tests", "oracle_filter_var.c")] + [os.path.join(oracle_hdr.ORACLE, f) for f in
                                                                             ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *oracle_hdr.CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = F._declare_base(C.CDLL(out))
    L.o_filter_hdr.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.POINTER(F.Filter), C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 3
    L.o_filter_hdr.restype = C.c_int
    L.o_filter_guide.argtypes = [C.c_float]
    L.o_filter_guide.restype = C.c_float
    L.o_filter_var.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.POINTER(FilterVar), C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 5
    L.o_filter_var.restype = C.c_int
    L.o_filter_var_value.argtypes = [C.c_float]
    L.o_filter_var_value.restype = C.c_float
    return L


def filter(L, rgb, guides, f, variance=None, op="clamp", exposure=1.0, plant=None, details=False):
    """rgb float32[H,W,3], guides as oracle_filter_hdr.filter takes them, variance float32[H,W] or None (the spatial estimate), f a
    FilterVar -> (filtered float32[H,W,3], tone-mapped rgba8[H,W,4], variance float32[H,W]) and, with details, u and v after every
    level float32[levels,H,W,4] and V2's v0 float32[H,W]; op None: the NULL vrt_tonemap"""
    rgb, n, a, z, c = F._planes(rgb, guides)
    h, w = rgb.shape[:2]
    if variance is not None:
        variance = np.ascontiguousarray(variance, np.float32)
        assert variance.shape == (h, w)
    out, out8, outv = np.zeros_like(rgb), np.zeros((h, w, 4), np.uint8), np.zeros((h, w), np.float32)
    lv, v0 = np.zeros((max(f.levels, 1), h, w, 4), np.float32), np.zeros((h, w), np.float32)
    if op is None:
        op, exposure = "clamp", 1.0
    r = L.o_filter_var(rgb.ctypes.data, n.ctypes.data, a.ctypes.data, z.ctypes.data, c.ctypes.data,
                       variance.ctypes.data if variance is not None else None, w, h, C.byref(f), OPS[op], float(np.float32(exposure)),
                       PLANT[plant], out.ctypes.data, out8.ctypes.data, outv.ctypes.data, lv.ctypes.data, v0.ctypes.data)
    assert r == 0
    return (out, out8, outv, lv[:f.levels], v0) if details else (out, out8, outv)


def hv_of(v):
    """hv(x) in numpy: NaN, -0 and everything negative -> +0, else at most 65504^2"""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.minimum(v, VAR_MAX), np.float32(0)).astype(np.float32)


def lum64(u):
    return (LUMA[0] * u[..., 0] + LUMA[1] * u[..., 1]) + LUMA[2] * u[..., 2]


# ---- float64 restatements with their bounds ------------------------------------------------------------------------------------------
def prep64(rgb, guides, f):
    """points 1-3 in float64 on the float32 inputs, as oracle_filter_hdr.filter64 has them"""
    rgb, n, a, z, c = F._planes(rgb, guides)
    N, A, Z, Cv = (F.g_of(v).astype(np.float64) for v in (n, a, z, c))
    live = Cv > 0
    demod = bool(f.flags & F.DEMODULATE)
    M = np.maximum(A[..., :3] + (1.0 - Cv)[..., None], float(np.float32(1.0) / np.float32(255.0))) if demod else np.ones_like(A[..., :3])

    def slope(dy, dx):
        best = np.full(Z.shape, np.inf)
        for sgn in (-1, 1):
            ok = F._shift(live, sgn * dy, sgn * dx, False)
            d = np.abs(F._shift(Z, sgn * dy, sgn * dx, 0.0) - Z)
            best = np.where(ok, np.minimum(best, d), best)
        return np.where(np.isinf(best), 0.0, best)

    return {"N": N, "A": A, "Z": Z, "live": live, "M": M, "u0": F.h_of(rgb).astype(np.float64) / M, "gx": slope(0, 1), "gy": slope(1, 0),
            "kn": float(np.float32(1.0) / (np.float32(f.sigma_normal) * np.float32(f.sigma_normal))),
            "ka": float(np.float32(1.0) / (np.float32(f.sigma_albedo) * np.float32(f.sigma_albedo))), "sd": float(np.float32(f.sigma_depth)),
            "ym2": lum64(M) ** 2 if demod else np.ones(Z.shape)}


def _guide_e(P, dy, dx):
    """point 4's e of the tap (dx, dy) pixels away -> (e, whether the tap counts)"""
    ok = F._shift(P["live"], dy, dx, False)
    dn2 = ((F._shift(P["N"], dy, dx, 0.0) - P["N"]) ** 2).sum(axis=2)
    da2 = ((F._shift(P["A"], dy, dx, 0.0) - P["A"]) ** 2).sum(axis=2)
    dzq = np.abs(F._shift(P["Z"], dy, dx, 0.0) - P["Z"])
    den = P["sd"] * ((P["gx"] * abs(dx) + P["gy"] * abs(dy)) + P["Z"] / 256.0) + 2.0 ** -20
    return (dn2 * P["kn"] + da2 * P["ka"]) + dzq / den, ok


ETA_GUIDE = E_EXP + 87 * 9 * EPS + EPS        # a guide-only weight's relative error: oracle_filter_hdr.rel_bound()


def v0_64(P):
    """V2's spatial estimate in float64 -> (v0, an absolute bound on the checker's error), for depths that are not negative.
    Every weight is within ETA_GUIDE, relatively; l is three products and two sums of values >= 0: 3 EPS, l * l: 7. s1 and s2 are
    at most 49 products (1 EPS) added one by one (48), sw 48 additions, the divisions 1: m1 is within 2 ETA_GUIDE + (3 + 98) EPS,
    m2 within 2 ETA_GUIDE + (7 + 98) EPS, relatively. m1 * m1 doubles m1's and adds 1, the difference adds 1 EPS of the larger
    operand: |dv0| <= (2 ETA_GUIDE + 105 EPS) m2 + (4 ETA_GUIDE + 204 EPS) m1^2, first order; max(0, .) does not stretch it."""
    l = lum64(P["u0"])
    sw, s1, s2 = np.zeros(l.shape), np.zeros(l.shape), np.zeros(l.shape)
    old = np.seterr(all="ignore")
    for oy in range(-3, 4):
        for ox in range(-3, 4):
            e, ok = _guide_e(P, oy, ox)
            w = np.where(ok & (e <= 87.0), np.exp(-np.minimum(e, 87.0)), 0.0)
            lq = F._shift(l, oy, ox, 0.0)
            sw, s1, s2 = sw + w, s1 + w * lq, s2 + w * lq * lq
    np.seterr(**old)
    live = P["live"]
    sw = np.where(live, sw, 1.0)
    m1, m2 = np.where(live, s1, 0.0) / sw, np.where(live, s2, 0.0) / sw
    bound = 1.05 * ((2 * ETA_GUIDE + 105 * EPS) * m2 + (4 * ETA_GUIDE + 204 * EPS) * m1 * m1)
    return np.maximum(0.0, m2 - m1 * m1), bound


def level64(P, u, v, s, sigma_lum):
    """One level of V3 in float64 on the checker's own float32 inputs u [H,W,3] and v [H,W] of that level -> (u', v', an absolute bound
    on the checker's u', one on its v'), for depths that are not negative. The inputs are exact, so the only cancellation is dl's:
      Y:    three products and two sums of values >= 0: within 3 EPS, relatively.
      dl:   |Yq - Yp| is within 3 EPS (Yq + Yp), absolutely, and 1 EPS of itself.
      sl:   at most 9 products G v (1 EPS) added one by one (8) and gs exact, the division 1: vbar within 10 EPS; its root halves that
            and adds 1, times sigma_lum 1, plus 2^-20 1: sl within 8 EPS, relatively.
      e:    the guide part within 9 EPS of itself (oracle_filter_hdr.rel_bound), t = dl / sl within (1 + 8 + 1) EPS of itself plus
            3 EPS (Yq + Yp) / sl, their sum 1 EPS of e:  de = 10 EPS e_guide + 11 EPS t + 3 EPS (Yq + Yp) / sl.
      w:    exp(-e) moves by the factor exp(+-de), det_expf adds E_EXP, the product with B 1 EPS: eta = expm1(de) + E_EXP + EPS.
      u':   N = sum w u, D = sum w: dN <= sum w eta u + 26 EPS N, dD <= sum w eta + 25 EPS D, the division 1 EPS:
            |du'| <= (sum w eta u) / D + u' ((sum w eta) / D + 52 EPS).
      v':   V = sum w^2 v: dV <= sum w^2 v (2 eta + 2 EPS) + 25 EPS V; D^2 within 2 dD / D + 1 EPS; the division 1:
            |dv'| <= (sum w^2 v 2 eta) / D^2 + v' (2 (sum w eta) / D + 80 EPS).
    All first order; the 1.1 in front covers the second."""
    sl_f = float(np.float32(sigma_lum))
    live = P["live"]
    gs, gv = np.zeros(v.shape), np.zeros(v.shape)
    for oy in range(-1, 2):
        for ox in range(-1, 2):
            ok = F._shift(live, s * oy, s * ox, False)
            gs = gs + np.where(ok, G3[oy + 1, ox + 1], 0.0)
            gv = gv + np.where(ok, G3[oy + 1, ox + 1] * F._shift(v, s * oy, s * ox, 0.0), 0.0)
    sl = sl_f * np.sqrt(gv / np.where(live, gs, 1.0)) + 2.0 ** -20
    y = lum64(u)
    D, Deta, Veta = np.zeros(v.shape), np.zeros(v.shape), np.zeros(v.shape)
    Nn, Neta, V = np.zeros(u.shape), np.zeros(u.shape), np.zeros(v.shape)
    old = np.seterr(all="ignore")
    for oy in range(-2, 3):
        for ox in range(-2, 3):
            eg, ok = _guide_e(P, s * oy, s * ox)
            yq = F._shift(y, s * oy, s * ox, 0.0)
            t = np.abs(yq - y) / sl
            e = eg + t
            de = 10 * EPS * eg + 11 * EPS * t + 3 * EPS * (yq + y) / sl
            ok = ok & (e <= 87.0)
            w = np.where(ok, F.B3[oy + 2] * F.B3[ox + 2] * np.exp(-np.minimum(e, 87.0)), 0.0)
            eta = np.where(ok, np.expm1(np.minimum(de, 50.0)) + E_EXP + EPS, 0.0)
            uq, vq = F._shift(u, s * oy, s * ox, 0.0), F._shift(v, s * oy, s * ox, 0.0)
            D, Deta = D + w, Deta + w * eta
            Nn, Neta = Nn + w[..., None] * uq, Neta + (w * eta)[..., None] * uq
            V, Veta = V + w * w * vq, Veta + w * w * vq * 2 * eta
    np.seterr(**old)
    D = np.where(live, D, 1.0)
    un, vn = Nn / D[..., None], V / (D * D)
    bu = 1.1 * (Neta / D[..., None] + un * (Deta / D + 52 * EPS)[..., None]) + 1e-30
    bv = 1.1 * (Veta / (D * D) + vn * (2 * Deta / D + 80 * EPS)) + 1e-30
    z3, z1 = np.zeros(u.shape), np.zeros(v.shape)
    return np.where(live[..., None], un, z3), np.where(live, vn, z1), np.where(live[..., None], bu, z3), np.where(live, bv, z1)


same = F.same
