"""The temporal pass with measured variances and a 3 x 3 search restated in scalar C (tests/oracle_temporal_mom.c) -- TEST
INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_temporal_mom.c as tests/oracle_temporal.py compiles its library; the C file includes that one's, so the
library holds everything oracle_temporal's holds and oracle_temporal.temporal() and oracle_filter_var.filter() take it too.
temporal() is include/vrt.h vrt_temporal_hdr_mom (T1, T2, T3, T3s, T4, T5, T7, T6m), chain() the accumulation forms' chain.
integrate64() restates T3-T6m in float64 numpy with a running bound on the checker's float32 error, in the manner of
oracle_temporal.integrate64 and on its class E; PLANT names the checker's planted misreadings."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_filter_hdr as F
import oracle_filter_var as FV
import oracle_hdr
import oracle_temporal as T

PLANT = {None: 0, "no_decay": 1, "bilinear_in_search": 2, "centre_by_floor": 3, "switch_on_nprev": 4}
EPS, VAR_MAX, E = T.EPS, T.VAR_MAX, T.E
DETAILS = 10                 # oracle_temporal's eight, whether the search ran, how many of its taps counted
ALWAYS = 32769               # measured_below: always the measured variance


class TemporalMom(C.Structure):
    """include/vrt.h vrt_temporal_mom"""
    _fields_ = T.Temporal._fields_ + [("measured_below", C.c_int32), ("search", C.c_int32)]


def make(t=None, measured_below=1, search=0):
    """a TemporalMom from an oracle_temporal.Temporal (None: make()'s defaults)"""
    m = TemporalMom()
    C.memmove(C.byref(m), C.byref(t if t is not None else T.make()), C.sizeof(T.Temporal))
    m.measured_below, m.search = int(measured_below), int(search)
    return m


def base(m):
    """the oracle_temporal.Temporal a TemporalMom begins with"""
    t = T.Temporal()
    C.memmove(C.byref(t), C.byref(m), C.sizeof(T.Temporal))
    return t


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_temporal_mom.so")
    srcs = [os.path.join(oracle_hdr.ROOT, "tests", "oracle_temporal_mom.c")] + [os.path.join(oracle_hdr.ORACLE, f) for f in
                                                                               ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *oracle_hdr.CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = F._declare_base(C.CDLL(out))
    # oracle_temporal.build()'s declarations
    L.o_filter_hdr.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.POINTER(F.Filter), C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 3
    L.o_filter_hdr.restype = C.c_int
    L.o_filter_guide.argtypes = [C.c_float]
    L.o_filter_guide.restype = C.c_float
    L.o_filter_var.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.POINTER(FV.FilterVar), C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 5
    L.o_filter_var.restype = C.c_int
    L.o_filter_var_value.argtypes = [C.c_float]
    L.o_filter_var_value.restype = C.c_float
    L.o_temporal.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_int, C.POINTER(T.Temporal), C.c_int] + [C.c_void_p] * 4
    L.o_temporal.restype = None
    # ... and this file's
    L.o_temporal_mom.argtypes = [C.c_void_p] * 9 + [C.c_int, C.c_int, C.POINTER(TemporalMom), C.c_int] + [C.c_void_p] * 4
    L.o_temporal_mom.restype = None
    return L


def temporal(L, cam, rgb, guides, variance, history, m, plant=None, details=False):
    """oracle_temporal.temporal()'s arguments with variance float32[H,W] or None after the guides and m a TemporalMom -> (history
    float32[3,H,W,4], integrated float32[H,W,3], variance float32[H,W]) and, with details, float32[H,W,10]"""
    ip, iv, cp = T._camera(cam)
    rgb, n, z, c = T._planes(rgb, guides)
    h, w = rgb.shape[:2]
    if history is not None:
        history = np.ascontiguousarray(history, np.float32)
        assert history.shape == (3, h, w, 4)
    if variance is not None:
        variance = np.ascontiguousarray(variance, np.float32)
        assert variance.shape == (h, w)
    out_h, out, outv = np.zeros((3, h, w, 4), np.float32), np.zeros_like(rgb), np.zeros((h, w), np.float32)
    det = np.zeros((h, w, DETAILS), np.float32)
    L.o_temporal_mom(ip.ctypes.data, iv.ctypes.data, cp.ctypes.data, rgb.ctypes.data, n.ctypes.data, z.ctypes.data, c.ctypes.data,
                     variance.ctypes.data if variance is not None else None, history.ctypes.data if history is not None else None, w, h,
                     C.byref(m), PLANT[plant], out_h.ctypes.data, out.ctypes.data, outv.ctypes.data, det.ctypes.data)
    return (out_h, out, outv, det) if details else (out_h, out, outv)


def chain(L, cam, mean, guides, variance, history, m, f, op="clamp", exposure=1.0):
    """vrt_accum_resolve_hdr_temporal_mom on the checker's own mean, planes and M3 plane (None: an accumulation without moments) ->
    (history, integrated, filtered rgb, rgba8, variance)"""
    hist, integ, var = temporal(L, cam, mean, guides, variance, history, m)
    rgb, rgba, outv = FV.filter(L, integ, guides, f, var, op, exposure)
    return hist, integ, rgb, rgba, outv


# ---- the float64 restatement with its bounds -----------------------------------------------------------------------------------------
def integrate64(rgb, guides, variance, history, m, det):
    """T3, T3s, T4, T5, T7, T6m in float64 on the float32 inputs and on the checker's own float32 fx, fy and Zexp (det: its details) ->
    (history float64[3,H,W,4], variance float64[H,W], a bound on each, unsure bool[H,W], searched bool[H,W]). unsure marks the pixels where a tap test of
    T3 or T3s, sw > 0 or sw == 0, N' >= 2 or N' < measured_below has a margin inside its own bound: they are left out of the
    comparison, and the caller states their share."""
    t = base(m)
    rgb, n, z, c = T._planes(rgb, guides)
    h, w = z.shape
    px = h * w
    hc = [F.h_of(rgb[..., k]).astype(np.float64).reshape(-1) for k in range(3)]
    Np = [F.g_of(n[..., k]).astype(np.float64).reshape(-1) for k in range(3)]
    Zp, Cp = F.g_of(z).astype(np.float64).reshape(-1), F.g_of(c).astype(np.float64).reshape(-1)
    live = Cp > 0
    fx, fy, zexp = (det[..., k].astype(np.float64).reshape(-1) for k in range(3))
    nmax = float(t.max_history)
    inside = live & (fx > -1) & (fx < w) & (fy > -1) & (fy < h) if history is not None else np.zeros(px, bool)
    reached = (det[..., 2].reshape(-1) != 0) | (det[..., 7].reshape(-1) != 0) | (det[..., 3:7].reshape(-1, 4).any(axis=1))
    inside &= reached
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = E(fx) - x0, E(fy) - y0
    wts = [(1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty]
    unsure = np.zeros(px, bool)
    zero = E(np.zeros(px))
    tol = float(np.float32(t.depth_tol)) * E(zexp) + 2.0 ** -20
    H0 = H1 = H2 = None
    if history is not None:
        H0, H1, H2 = (np.asarray(history[k], np.float32).reshape(-1, 4) for k in range(3))

    def tap(qx, qy, where):
        """T3's tests of the tap (qx, qy) of every pixel in `where` -> (counts, its seven quantities), marking the unsure"""
        nonlocal unsure
        ok = where & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
        q = np.where(ok, qy * w + qx, 0).astype(np.int64)
        Nq = np.minimum(np.maximum(F.g_of(H0[q, 3]).astype(np.float64), 0.0), nmax)
        Zq, Cq = F.g_of(H1[q, 2]).astype(np.float64), F.g_of(H1[q, 3]).astype(np.float64)
        nq = [F.g_of(H2[q, j]).astype(np.float64) for j in range(3)]
        nd = (E(nq[0]) * Np[0] + E(nq[1]) * Np[1]) + E(nq[2]) * Np[2]
        dz = (E(Zq) - zexp).abs()
        ok = ok & (Cq > 0) & (Nq >= 1)
        n_margin, z_margin = nd.v - float(np.float32(t.normal_min)), tol.v - dz.v
        unsure |= ok & (((np.abs(n_margin) <= 1.1 * nd.e) & (nd.e > 0)) | (np.abs(z_margin) <= 1.1 * (tol.e + dz.e)))
        ok = ok & (n_margin >= 0) & (z_margin >= 0)
        xs = [F.h_of(H0[q, j]).astype(np.float64) for j in range(3)] + [Nq, F.h_of(H1[q, 0]).astype(np.float64),
                                                                      FV.hv_of(H1[q, 1]).astype(np.float64), FV.hv_of(H2[q, 3]).astype(np.float64)]
        return ok, xs

    sw, s = zero, [zero] * 7
    searched = np.zeros(px, bool)
    if history is not None:
        for k in range(4):                                                         # T3
            ok, xs = tap(x0 + (k & 1), y0 + (k >> 1), inside)
            wk = wts[k]
            sw = (sw + wk).where(ok, sw)
            s = [(s[j] + wk * xs[j]).where(ok, s[j]) for j in range(7)]
        # sw == 0 decides the search: a sum of counted weights that is zero within its bound but not exactly is unsure
        unsure |= inside & (np.abs(sw.v) <= 1.1 * sw.e) & (sw.e > 0)
        if m.search == 1:                                                          # T3s
            searched = inside & (sw.v == 0)
            xc, yc = np.floor(fx + 0.5), np.floor(fy + 0.5)
            # the centre: fx + 0.5f is rounded; a position within that rounding of a half-integer boundary is unsure
            for f_ in (fx, fy):
                frac = (f_ + 0.5) - np.floor(f_ + 0.5)
                unsure |= searched & (np.minimum(frac, 1.0 - frac) <= 1.1 * EPS * np.abs(f_ + 0.5))
            ssw, ss = zero, [zero] * 7
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ok, xs = tap(xc + dx, yc + dy, searched)
                    ssw = (ssw + 1.0).where(ok, ssw)
                    ss = [(ss[j] + xs[j]).where(ok, ss[j]) for j in range(7)]
            sw = ssw.where(searched, sw)
            s = [ss[j].where(searched, s[j]) for j in range(7)]
    have = sw.v > 0
    old = np.seterr(all="ignore")
    den = sw.where(have, E(np.ones(px)))
    prev = [(x / den).where(have, zero) for x in s]
    cp, nprev, m1p, m2p, vp = prev[:3], prev[3], prev[4], prev[5], prev[6]
    nn = (nprev + 1.0).at_most(nmax)
    inv = 1.0 / nn
    a, am = inv.at_least(float(np.float32(t.alpha_min))), inv.at_least(float(np.float32(t.alpha_moments_min)))
    cn = [cp[j] + a * (E(hc[j]) - cp[j]) for j in range(3)]
    Y = T.lum64([E(hc[j]) for j in range(3)])
    m1, m2 = m1p + am * (Y - m1p), m2p + am * (Y * Y - m2p)
    spread = (m2 - m1 * m1).at_least(0.0)
    t6 = (spread / (nn - 1.0).where(nn.v >= 2, E(np.ones(px)))).at_most(float(VAR_MAX))
    t6 = t6.where(nn.v >= 2, E(np.full(px, float(VAR_MAX))))
    v = FV.hv_of(variance).astype(np.float64).reshape(-1) if variance is not None else np.full(px, float(VAR_MAX))   # T7
    om = 1.0 - a
    vn = ((om * om) * vp + (a * a) * E(v)).at_least(0.0).at_most(float(VAR_MAX))
    below = float(m.measured_below)
    measured = nn.v < below
    var = vn.where(measured, t6)
    unsure |= live & ~measured & (np.abs(nn.v - 2.0) <= 1.1 * nn.e) & (nn.e > 0)
    unsure |= live & (np.abs(nn.v - below) <= 1.1 * nn.e) & (nn.e > 0) & (below <= nmax)
    np.seterr(**old)
    dead = ~live
    out = np.zeros((3, px, 4))
    err = np.zeros((3, px, 4))
    for j in range(3):
        out[0, :, j], err[0, :, j] = np.where(dead, hc[j], cn[j].v), np.where(dead, 0.0, cn[j].e)
        out[2, :, j] = np.where(dead, 0.0, Np[j])
    out[0, :, 3], err[0, :, 3] = np.where(dead, 0.0, nn.v), np.where(dead, 0.0, nn.e)
    out[1, :, 0], err[1, :, 0] = np.where(dead, 0.0, m1.v), np.where(dead, 0.0, m1.e)
    out[1, :, 1], err[1, :, 1] = np.where(dead, 0.0, m2.v), np.where(dead, 0.0, m2.e)
    out[1, :, 2], out[1, :, 3] = np.where(dead, 0.0, Zp), np.where(dead, 0.0, Cp)
    out[2, :, 3], err[2, :, 3] = np.where(dead, 0.0, vn.v), np.where(dead, 0.0, vn.e)
    return (out.reshape(3, h, w, 4), np.where(dead, 0.0, var.v).reshape(h, w), 1.1 * err.reshape(3, h, w, 4) + 1e-30,
            (1.1 * np.where(dead, 0.0, var.e) + 1e-30).reshape(h, w), unsure.reshape(h, w), searched.reshape(h, w))


same = F.same
