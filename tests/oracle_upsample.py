"""The guided upsampling pass restated in scalar C (tests/oracle_upsample.c) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_upsample.c as tests/oracle_filter_hdr.py compiles its library; the C file includes that one's, so the
library holds everything oracle_filter_hdr's holds and oracle_filter_hdr.filter() takes it too. upsample() is include/vrt.h
vrt_upsample_hdr U1-U6. upsample64() restates U4-U6 in float64 numpy on the float32 inputs and on the checker's own float32 fx, fy
(U3 is two operations, exact for the factors and offsets the closed forms use), with a running bound on the checker's float32 error
(oracle_temporal.E: one EPS per float32 operation, carried through every operation, first order); PLANT names the checker's planted
misreadings."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_filter_hdr as F
import oracle_hdr
from oracle_temporal import E

PLANT = {None: 0, "offsets_swapped": 1, "low_albedo_out": 2, "liveness_ignored": 3, "ddx_unscaled": 4}
EPS = F.EPS
OPS = F.OPS
DEMODULATE = 1
MAX_FACTOR = 4
KEYS = ("factor", "demodulate", "sigma_normal", "sigma_albedo", "sigma_depth", "min_weight", "offset_lo_x", "offset_lo_y", "offset_hi_x",
        "offset_hi_y")


class Upsample(C.Structure):
    """include/vrt.h vrt_upsample"""
    _fields_ = [("factor", C.c_int32), ("flags", C.c_uint32), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float),
                ("sigma_depth", C.c_float), ("min_weight", C.c_float), ("offset_lo_x", C.c_float), ("offset_lo_y", C.c_float),
                ("offset_hi_x", C.c_float), ("offset_hi_y", C.c_float)]


def make(factor=2, demodulate=True, sigma_normal=0.5, sigma_albedo=0.05, sigma_depth=0.5, min_weight=0.0, offset_lo=(0.0, 0.0),
         offset_hi=(0.0, 0.0)):
    return Upsample(int(factor), DEMODULATE if demodulate else 0, sigma_normal, sigma_albedo, sigma_depth, min_weight, offset_lo[0],
                    offset_lo[1], offset_hi[0], offset_hi[1])


def keys(u):
    """an Upsample as the dict Context.upsample_hdr takes"""
    d = {k: getattr(u, k) for k in KEYS if k != "demodulate"}
    d["demodulate"] = bool(u.flags & DEMODULATE)
    return d


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_upsample.so")
    srcs = [os.path.join(oracle_hdr.ROOT, "tests", "oracle_upsample.c")] + [os.path.join(oracle_hdr.ORACLE, f) for f in
                                                                           ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *oracle_hdr.CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = F._declare_base(C.CDLL(out))
    L.o_filter_hdr.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.POINTER(F.Filter), C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 3
    L.o_filter_hdr.restype = C.c_int
    L.o_filter_guide.argtypes = [C.c_float]
    L.o_filter_guide.restype = C.c_float
    L.o_upsample.argtypes = [C.c_void_p] * 9 + [C.c_int, C.c_int, C.POINTER(Upsample), C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 4
    L.o_upsample.restype = C.c_int
    return L


def _guides(g, h, w):
    n, a = np.ascontiguousarray(g["normal"], np.float32), np.ascontiguousarray(g["albedo"], np.float32)
    z, c = np.ascontiguousarray(g["depth"], np.float32), np.ascontiguousarray(g["coverage"], np.float32)
    assert n.shape == (h, w, 3) and a.shape == (h, w, 4) and z.shape == (h, w) and c.shape == (h, w), (n.shape, a.shape, z.shape, c.shape, h, w)
    return n, a, z, c


def upsample(L, rgb, guides, hi_guides, u, op="clamp", exposure=1.0, plant=None, details=False):
    """rgb float32[h,w,3] and guides: the LOW side; hi_guides at [r h, r w]; u an Upsample -> (rgb float32[H,W,3], rgba8[H,W,4],
    unresolved uint8[H,W]) and, with details, float32[H,W,8]: fx, fy, the four tap weights, sumw, 0; op None: the NULL vrt_tonemap"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    assert rgb.shape == (h, w, 3)
    r = u.factor
    lo, hi = _guides(guides, h, w), _guides(hi_guides, r * h, r * w)
    out, out8, mask = np.zeros((r * h, r * w, 3), np.float32), np.zeros((r * h, r * w, 4), np.uint8), np.zeros((r * h, r * w), np.uint8)
    det = np.zeros((r * h, r * w, 8), np.float32)
    if op is None:
        op, exposure = "clamp", 1.0
    rc = L.o_upsample(rgb.ctypes.data, *(p.ctypes.data for p in lo), *(p.ctypes.data for p in hi), w, h, C.byref(u), OPS[op],
                      float(np.float32(exposure)), PLANT[plant], out.ctypes.data, out8.ctypes.data, mask.ctypes.data, det.ctypes.data)
    assert rc == 0
    return (out, out8, mask, det) if details else (out, out8, mask)


def bilinear32(u, r, offset_lo, offset_hi):
    """The float32 bilinear interpolation of u float32[h,w,C] at factor r by U3-U5 with every weight w = b: taps outside the image
    skipped, sums from 0 in tap order, divided by sumw -> float32[r h, r w, C] (every high pixel has a tap inside for offsets in
    [0, 1] unless all its b are 0, which the callers' offsets exclude)"""
    f = np.float32
    u = np.asarray(u, f)
    h, w = u.shape[:2]
    ys, xs = np.mgrid[0:r * h, 0:r * w]
    fx = (xs.astype(f) + f(offset_hi[0])) / f(r) - f(offset_lo[0])
    fy = (ys.astype(f) + f(offset_hi[1])) / f(r) - f(offset_lo[1])
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = fx - x0, fy - y0
    b = [(f(1) - tx) * (f(1) - ty), tx * (f(1) - ty), (f(1) - tx) * ty, tx * ty]
    sumw = np.zeros(fx.shape, f)
    acc = np.zeros(fx.shape + (u.shape[2],), f)
    for k in range(4):
        X, Y = x0.astype(np.int64) + (k & 1), y0.astype(np.int64) + (k >> 1)
        ok = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
        uq = u[np.clip(Y, 0, h - 1), np.clip(X, 0, w - 1)]
        sumw = np.where(ok, sumw + b[k], sumw).astype(f)
        acc = np.where(ok[..., None], acc + b[k][..., None] * uq, acc).astype(f)
    return (acc / sumw[..., None]).astype(f)


# ---- the float64 restatement with its bound --------------------------------------------------------------------------------------------
def _exp(e):
    """exp(-e) of an E whose value is >= 0: det_expf's own relative error and the sensitivity to e's"""
    v = np.exp(-np.minimum(e.v, 700.0))
    return E(v, v * (e.e + F.E_EXP))


def upsample64(rgb, guides, hi_guides, u, det):
    """U4-U6 in float64 on the float32 inputs and the checker's own fx, fy (det: its details) -> (f float64[H,W,3], a bound on the
    checker's float32 error of each, unresolved bool[H,W], unsure bool[H,W]). unsure marks the pixels where sumw > min_weight has a
    margin inside its own bound, or where every weight lies below det_expf's range: they are left out of the comparison, and the caller
    states their share. Depths are taken as not negative (the guide planes' are)."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    r = u.factor
    H, W = r * h, r * w
    n, a, z, c = (F.g_of(v).astype(np.float64) for v in _guides(guides, h, w))
    Nn, A, Z, Cv = (F.g_of(v).astype(np.float64) for v in _guides(hi_guides, H, W))
    demod = bool(u.flags & DEMODULATE)
    floor255 = float(np.float32(1.0) / np.float32(255.0))
    live_lo, live_hi = c > 0, Cv > 0
    one = np.ones((h, w))
    m_lo = [(E(a[..., k]) + (1.0 - E(c))).at_least(floor255).where(live_lo & demod, E(one)) for k in range(3)]
    u_lo = [E(F.h_of(rgb[..., k]).astype(np.float64)) / m_lo[k] for k in range(3)]
    m_hi = [(E(A[..., k]) + (1.0 - E(Cv))).at_least(floor255).where(live_hi & demod, E(np.ones((H, W)))) for k in range(3)]
    kn = float(np.float32(1.0) / (np.float32(u.sigma_normal) * np.float32(u.sigma_normal)))
    ka = float(np.float32(1.0) / (np.float32(u.sigma_albedo) * np.float32(u.sigma_albedo)))
    sd = float(np.float32(u.sigma_depth))

    def slope(dy, dx):
        best, err = np.full(Z.shape, np.inf), np.zeros(Z.shape)
        for sgn in (-1, 1):
            ok = F._shift(live_hi, sgn * dy, sgn * dx, False)
            d = np.abs(F._shift(Z, sgn * dy, sgn * dx, 0.0) - Z)
            best = np.where(ok, np.minimum(best, d), best)
        best = np.where(np.isinf(best), 0.0, best)
        return E(best, EPS * best)

    gx, gy = slope(0, 1), slope(1, 0)
    fx, fy = det[..., 0].astype(np.float64), det[..., 1].astype(np.float64)
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = E(fx) - x0, E(fy) - y0
    b = [(1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty]
    zero = E(np.zeros((H, W)))
    sumw, acc = zero, [zero, zero, zero]
    tiny = np.zeros((H, W), bool)
    old = np.seterr(all="ignore")
    for k in range(4):
        X, Y = x0.astype(np.int64) + (k & 1), y0.astype(np.int64) + (k >> 1)
        inside = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
        Xc, Yc = np.clip(X, 0, w - 1), np.clip(Y, 0, h - 1)
        ok = inside & (live_lo[Yc, Xc] == live_hi)
        dn2 = zero
        for j in range(3):
            d = E(n[Yc, Xc, j]) - Nn[..., j]
            dn2 = d * d if j == 0 else (dn2 + d * d)
        d = [E(a[Yc, Xc, j]) - A[..., j] for j in range(4)]
        da2 = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])
        dzq = (E(z[Yc, Xc]) - Z).abs()
        ddx, ddy = (E(X.astype(np.float64)) - fx).abs() * float(r), (E(Y.astype(np.float64)) - fy).abs() * float(r)
        den = sd * ((gx * ddx + gy * ddy) + E(Z) * (1.0 / 256.0)) + 2.0 ** -20
        e = (dn2 * kn + da2 * ka) + dzq / den
        wt = (b[k] * _exp(e)).where(live_hi, b[k])
        tiny |= ok & live_hi & (e.v > 80.0)
        sumw = (sumw + wt).where(ok, sumw)
        acc = [(acc[j] + wt * E(u_lo[j].v[Yc, Xc], u_lo[j].e[Yc, Xc])).where(ok, acc[j]) for j in range(3)]
    mw = float(np.float32(u.min_weight))
    resolved = sumw.v > mw
    unsure = (np.abs(sumw.v - mw) <= 1.1 * sumw.e) & (sumw.e > 0)
    unsure |= tiny & (sumw.v < 1e-20)
    Nx = np.clip(np.floor(fx + 0.5), 0, w - 1).astype(np.int64)
    Ny = np.clip(np.floor(fy + 0.5), 0, h - 1).astype(np.int64)
    den = sumw.where(resolved, E(np.ones((H, W))))
    out = np.zeros((H, W, 3))
    err = np.zeros((H, W, 3))
    for j in range(3):
        up = (acc[j] / den).where(resolved, E(u_lo[j].v[Ny, Nx], u_lo[j].e[Ny, Nx]))
        fo = (up * m_hi[j]).at_least(0.0).at_most(65504.0)
        out[..., j], err[..., j] = fo.v, fo.e
    np.seterr(**old)
    return out, 1.1 * err + 1e-30, ~resolved, unsure


same = F.same
