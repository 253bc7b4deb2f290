"""The guided filter restated in scalar C (tests/oracle_filter_hdr.c) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_filter_hdr.c as tests/oracle_hdr.py compiles its library: oracle/Makefile's flags (no contraction),
the same three other oracle sources. The library holds everything oracle_denoise_hdr's holds (the C file includes it), so
oracle_hdr.render / tonemap and oracle_denoise_hdr.denoise take it too. filter() is include/vrt.h vrt_filter_hdr points 1-5;
filter64() the same rule in float64 numpy with rel_bound() its error bound; PLANT names the checker's planted misreadings."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_denoise_hdr
import oracle_hdr

OPS = oracle_hdr.OPS
DEMODULATE = 1
MAX_LEVELS = 8
PLANT = {None: 0, "slope_max": 1, "no_alpha": 2, "dead_taps": 3, "no_step": 4}
B3 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
EPS = 2.0 ** -24            # half an ulp, relative: one float32 rounding
E_EXP = 1.2e-7              # relative, det_expf on [-87, 0] (tests/shader_ref64.py, measured by tests/test_path_reference64.py)


class Filter(C.Structure):
    """include/vrt.h vrt_filter"""
    _fields_ = [("levels", C.c_int32), ("flags", C.c_uint32), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float),
                ("sigma_depth", C.c_float)]


def make(levels, demodulate=True, sigma_normal=1.0, sigma_albedo=0.05, sigma_depth=2.0):
    return Filter(int(levels), DEMODULATE if demodulate else 0, sigma_normal, sigma_albedo, sigma_depth)


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_filter_hdr.so")
    srcs = [os.path.join(oracle_hdr.ROOT, "tests", "oracle_filter_hdr.c")] + [os.path.join(oracle_hdr.ORACLE, f) for f in
                                                                             ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *oracle_hdr.CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = _declare_base(C.CDLL(out))
    L.o_filter_hdr.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.POINTER(Filter), C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 3
    L.o_filter_hdr.restype = C.c_int
    L.o_filter_guide.argtypes = [C.c_float]
    L.o_filter_guide.restype = C.c_float
    return L


def _declare_base(L):
    """what oracle_denoise_hdr.build() declares of the sources this library shares with it"""
    L.o_denoise_hdr.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    L.o_denoise_hdr.restype = None
    L.o_render_hdr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_float, C.c_float,
                               C.c_void_p]
    L.o_render_hdr.restype = None
    L.o_render_lens.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_float,
                                C.c_float, C.c_void_p, C.c_void_p]
    L.o_render_lens.restype = None
    L.o_hdr_unorm8.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.o_hdr_unorm8.restype = None
    L.o_hdr_value.argtypes = [C.c_float]
    L.o_hdr_value.restype = C.c_float
    L.o_hdr_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.o_hdr_add.restype = None
    L.o_hdr_mean.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.o_hdr_mean.restype = None
    L.o_hdr_tonemap.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_void_p]
    L.o_hdr_tonemap.restype = None
    return L


def _planes(rgb, g):
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    n, a = np.ascontiguousarray(g["normal"], np.float32), np.ascontiguousarray(g["albedo"], np.float32)
    z, c = np.ascontiguousarray(g["depth"], np.float32), np.ascontiguousarray(g["coverage"], np.float32)
    assert rgb.shape == (h, w, 3) and n.shape == (h, w, 3) and a.shape == (h, w, 4) and z.shape == (h, w) and c.shape == (h, w)
    return rgb, n, a, z, c


def filter(L, rgb, guides, f, op="clamp", exposure=1.0, plant=None, levels_out=False):
    """rgb float32[H,W,3], guides {"normal", "albedo", "depth", "coverage"} as vrt_accum_guides returns them, f a Filter ->
    (filtered float32[H,W,3], tone-mapped rgba8[H,W,4]) and, with levels_out, u after every level float32[levels,H,W,3];
    op None: the NULL vrt_tonemap"""
    rgb, n, a, z, c = _planes(rgb, guides)
    h, w = rgb.shape[:2]
    out, out8 = np.zeros_like(rgb), np.zeros((h, w, 4), np.uint8)
    lv = np.zeros((max(f.levels, 1), h, w, 3), np.float32)
    if op is None:
        op, exposure = "clamp", 1.0
    r = L.o_filter_hdr(rgb.ctypes.data, n.ctypes.data, a.ctypes.data, z.ctypes.data, c.ctypes.data, w, h, C.byref(f), OPS[op],
                       float(np.float32(exposure)), PLANT[plant], out.ctypes.data, out8.ctypes.data, lv.ctypes.data)
    assert r == 0
    return (out, out8, lv[:f.levels]) if levels_out else (out, out8)


def g_of(v):
    """g(v) of point 1 in numpy: NaN -> 0, else into [-65504, 65504]"""
    v = np.asarray(v, np.float32)
    return np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(-65504), np.float32(65504))).astype(np.float32)


def h_of(v):
    """h(c) in numpy: NaN, -0 and everything negative -> +0, else at most 65504"""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.minimum(v, np.float32(65504)), np.float32(0)).astype(np.float32)


def _shift(a, dy, dx, fill):
    """a[y + dy, x + dx] where that is inside the image, `fill` elsewhere"""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if (dy < H and -dy < H) and (dx < W and -dx < W):
        out[yd, xd] = a[ys, xs]
    return out


def filter64(rgb, guides, f):
    """The five points in float64 numpy on the float32 inputs (kn, ka as the host computes them, in float32) -> float64[H,W,3]"""
    rgb, n, a, z, c = _planes(rgb, guides)
    N, A, Z, Cv = (g_of(v).astype(np.float64) for v in (n, a, z, c))
    live = Cv > 0
    demod = bool(f.flags & DEMODULATE)
    M = np.maximum(A[..., :3] + (1.0 - Cv)[..., None], float(np.float32(1.0) / np.float32(255.0))) if demod else np.ones_like(A[..., :3])
    hc = h_of(rgb).astype(np.float64)
    u = hc / M
    kn = float(np.float32(1.0) / (np.float32(f.sigma_normal) * np.float32(f.sigma_normal)))
    ka = float(np.float32(1.0) / (np.float32(f.sigma_albedo) * np.float32(f.sigma_albedo)))
    sd = float(np.float32(f.sigma_depth))

    def slope(dy, dx):
        best = np.full(Z.shape, np.inf)
        for sgn in (-1, 1):
            ok = _shift(live, sgn * dy, sgn * dx, False)
            d = np.abs(_shift(Z, sgn * dy, sgn * dx, 0.0) - Z)
            best = np.where(ok, np.minimum(best, d), best)
        return np.where(np.isinf(best), 0.0, best)

    gx, gy = slope(0, 1), slope(1, 0)
    old = np.seterr(all="ignore")   # pixels that are not live are computed along with the rest (a negative depth overflows there) and dropped
    for i in range(f.levels):
        s = 1 << i
        sumw = np.zeros(Z.shape)
        acc = np.zeros(u.shape)
        for oy in range(-2, 3):
            for ox in range(-2, 3):
                ok = _shift(live, s * oy, s * ox, False)
                dn2 = ((_shift(N, s * oy, s * ox, 0.0) - N) ** 2).sum(axis=2)
                da2 = ((_shift(A, s * oy, s * ox, 0.0) - A) ** 2).sum(axis=2)
                dzq = np.abs(_shift(Z, s * oy, s * ox, 0.0) - Z)
                den = sd * ((gx * (abs(ox) * s) + gy * (abs(oy) * s)) + Z / 256.0) + 2.0 ** -20
                e = (dn2 * kn + da2 * ka) + dzq / den
                w = np.where(ok & (e <= 87.0), B3[oy + 2] * B3[ox + 2] * np.exp(-np.minimum(e, 87.0)), 0.0)
                sumw += w
                acc += w[..., None] * _shift(u, s * oy, s * ox, 0.0)
        u = np.where(live[..., None], acc / np.where(live, sumw, 1.0)[..., None], 0.0)
    np.seterr(**old)
    return np.where(live[..., None], np.clip(u * M, 0.0, 65504.0), hc)


def rel_bound(levels):
    """The relative error of the checker's float32 result against filter64(), for inputs whose depths are not negative (every term
    of e and of den is then >= 0: no cancellation). First order in EPS = 2^-24, one EPS per float32 operation:
      e:   a difference EPS, its square 3, the sums +2 -> dn2, da2: 5; times kn / ka 6, their sum 7. den: a slope EPS, its product 2,
           the sum of two 3, plus the exact Z / 256 4, times sigma_depth 5, plus 2^-20 6; dzq / den: 1 + 6 + 1 = 8; e: 9 EPS.
      w:   exp(-e) has absolute sensitivity e <= 87 to e's relative error, and det_expf its own E_EXP; the B product is exact, the
           product with it one EPS:  eta = E_EXP + 87 * 9 EPS + EPS.   (Past 87 the weight is 0 or below 1.7e-38: nothing.)
      u':  the same w stands in numerator and denominator, every u is >= 0: the ratio moves by at most 2 eta; each product w * u one
           EPS, 25 sequential additions in each of the two sums and the division: 2 * 25 + 2 EPS.  R = 2 eta + 52 EPS per level,
           and the level's inputs carry the level before's relative error through unchanged (a weighted mean of values >= 0).
      ends: m is two operations, h(c) / m one more: 3 EPS in; u * m: 3 more out. h() does not stretch an error."""
    eta = E_EXP + 87 * 9 * EPS + EPS
    return 1.05 * (levels * (2 * eta + 52 * EPS) + 6 * EPS)


def same(got, want, what):
    """bit for bit on a float32 or uint8 image"""
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    gb, wb = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
    if not np.array_equal(gb, wb):
        bad = np.argwhere(gb != wb)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: differs at {len(bad)} entries; first at {i}: got {g[i]!r} want {w[i]!r}")
