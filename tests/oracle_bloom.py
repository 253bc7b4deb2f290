"""Bloom restated twice -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles tests/oracle_bloom.c (B0-B8 of include/vrt.h vrt_bloom_hdr in scalar C) as tests/oracle_meter.py compiles its
library; run() calls it, PLANT names its planted misreadings. The second restatement, py_run(), is float32 numpy on whole images, one
operation per expression, written from the header again: it gathers the taps of a level with index arrays where the C walks the
pixels. The two share no code. workspace_bytes() restates vrt_bloom_workspace_bytes."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_hdr

MAX_LEVELS = 8
KARIS = 1
PLANT = {None: 0, "far_near_swapped": 1, "tent_by_multiplying": 2, "karis_weight_at_level_2": 3, "threshold_against_y": 4,
         "inv_levels_left_out": 5}
OPS = oracle_hdr.OPS
KEYS = ("levels", "karis", "threshold", "knee", "intensity")
f32 = np.float32
F32_MAX = f32(3.402823466e38)


class Bloom(C.Structure):
    """include/vrt.h vrt_bloom"""
    _fields_ = [("levels", C.c_int32), ("flags", C.c_uint32), ("threshold", C.c_float), ("knee", C.c_float), ("intensity", C.c_float)]


class Record(C.Structure):
    """include/vrt.h vrt_exposure"""
    _fields_ = [("exposure", C.c_float), ("metered", C.c_float), ("window", C.c_uint32), ("frames", C.c_uint32)]


def make(levels=5, karis=True, threshold=1.0, knee=0.5, intensity=0.2):
    return Bloom(levels, KARIS if karis else 0, threshold, knee, intensity)


def keys(b):
    """a Bloom as the dict the package's `bloom` arguments take"""
    return {"levels": int(b.levels), "karis": bool(b.flags & KARIS), "threshold": float(b.threshold), "knee": float(b.knee),
            "intensity": float(b.intensity)}


def sizes(width, height, levels):
    """B0 -> [(w_l, h_l) for l = 0..levels]"""
    out = [(width, height)]
    for _ in range(levels):
        w, h = out[-1]
        out.append(((w + 1) >> 1, (h + 1) >> 1))
    return out


def workspace_bytes(width, height, levels):
    """vrt_bloom_workspace_bytes in Python's integers"""
    if width < 1 or height < 1 or width * height > 1 << 30 or not 1 <= levels <= MAX_LEVELS:
        return 0
    return sum((w * h * 16 + 255) // 256 * 256 for w, h in sizes(width, height, levels)[1:])


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_bloom.so")
    srcs = [os.path.join(oracle_hdr.ROOT, "tests", "oracle_bloom.c")] + [os.path.join(oracle_hdr.ORACLE, f) for f in
                                                                        ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *oracle_hdr.CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_bloom_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Bloom), C.c_int, C.c_float, C.POINTER(Record), C.c_int] + [C.c_void_p] * 4
    L.o_bloom_run.restype = C.c_int
    return L


def _record(state):
    return None if state is None else C.byref(Record(state["exposure"], state.get("metered", 0.0), state.get("window", 0), state.get("frames", 0)))


def run(L, rgb, b, op="clamp", exposure=1.0, state=None, plant=None, detail=False):
    """B0-B8: rgb float32[H,W,3], a Bloom, the tone map (op None: the NULL vrt_tonemap), the record as a dict (None: no record) ->
    (f float32[H,W,3], rgba8[H,W,4]); detail: also ([D_l float32[h_l,w_l,4] for l = 1..L], B float32[H,W,3])"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    assert rgb.shape == (h, w, 3)
    if op is None:
        op, exposure = "clamp", 1.0
    f = np.zeros((h, w, 3), np.float32)
    rgba = np.zeros((h, w, 4), np.uint8)
    sz = sizes(w, h, b.levels)[1:]
    levels = np.zeros(sum(lw * lh * 4 for lw, lh in sz), np.float32) if detail else None
    glow = np.zeros((h, w, 3), np.float32) if detail else None
    r = L.o_bloom_run(rgb.ctypes.data, w, h, C.byref(b), OPS[op], float(np.float32(exposure)), _record(state), PLANT[plant], f.ctypes.data,
                      rgba.ctypes.data, None if levels is None else levels.ctypes.data, None if glow is None else glow.ctypes.data)
    assert r == 0
    if not detail:
        return f, rgba
    out, at = [], 0
    for lw, lh in sz:
        out.append(levels[at:at + lw * lh * 4].reshape(lh, lw, 4))
        at += lw * lh * 4
    return f, rgba, out, glow


# ---- the numpy restatement ----

def _min(a, b):
    """min(a, b) = b < a ? b : a"""
    return np.where(b < a, b, a).astype(np.float32)


def _max(a, b):
    """max(a, b) = a < b ? b : a"""
    return np.where(a < b, b, a).astype(np.float32)


def _h(c):
    c = np.asarray(c, np.float32)
    return _min(_max(np.zeros_like(c), c), np.full_like(c, 65504.0))


def _lum(x):
    x = _h(x)
    return ((f32(0.2126) * x[..., 0] + f32(0.7152) * x[..., 1]).astype(np.float32) + f32(0.0722) * x[..., 2]).astype(np.float32)


def _tent(a0, a1, a2, a3):
    p0, p1, p2 = a0 + a1, a1 + a2, a2 + a3
    return (p0 + p1) + (p1 + p2)


def _taps(n_dst, n_src):
    """B4's four source indices per destination index -> int[4, n_dst]"""
    d = np.arange(n_dst)
    return np.stack([np.clip(2 * d + o, 0, n_src - 1) for o in (-1, 0, 1, 2)])


def _down(s):
    """B4 on float32[h, w, 4] -> float32[h', w', 4], before any division"""
    sh, sw = s.shape[:2]
    dh, dw = (sh + 1) >> 1, (sw + 1) >> 1
    cx, cy = _taps(dw, sw), _taps(dh, sh)
    rows = [_tent(*(s[cy[j]][:, cx[o]] for o in range(4))) for j in range(4)]
    return (_tent(*rows) * f32(0.015625)).astype(np.float32)


def _lerp(far, near):
    return (((far + near) + (near + near)) * f32(0.25)).astype(np.float32)


def _up(s, w, h):
    """B5: float32[h', w', C] -> float32[h, w, C]"""
    sh, sw = s.shape[:2]
    x, y = np.arange(w), np.arange(h)
    nx, ny = x >> 1, y >> 1
    fx = np.clip(nx + np.where(x & 1, 1, -1), 0, sw - 1)
    fy = np.clip(ny + np.where(y & 1, 1, -1), 0, sh - 1)
    t_far = _lerp(s[fy][:, fx], s[fy][:, nx])
    t_near = _lerp(s[ny][:, fx], s[ny][:, nx])
    return _lerp(t_far, t_near)


def py_run(rgb, b, op="clamp", exposure=1.0, state=None, detail=False):
    """B0-B8 in float32 numpy; the arguments and the results of run()"""
    rgb = np.asarray(rgb, np.float32)
    hh, ww = rgb.shape[:2]
    if op is None:
        op, exposure = "clamp", 1.0
    with np.errstate(all="ignore"):
        e = f32(exposure)
        if state is not None:
            e = _min(f32(e * f32(state["exposure"])), F32_MAX)[()]
        thr, knee, gain = f32(b.threshold), f32(b.knee), f32(b.intensity)
        # B2
        x = _h(rgb)
        y = _lum(rgb)
        ye = _min((y * e).astype(np.float32), np.full_like(y, F32_MAX))
        d = (ye - thr).astype(np.float32)
        soft = np.zeros_like(d)
        if knee > 0:
            s = _min(_max((d + knee).astype(np.float32), np.zeros_like(d)), np.full_like(d, f32(knee + knee)))
            soft = ((s * s).astype(np.float32) / f32(f32(4.0) * knee)).astype(np.float32)
        a = _max(_max(soft, d), np.zeros_like(d))
        g = _min((a / _max(ye, np.full_like(ye, f32(2.0 ** -16)))).astype(np.float32), np.ones_like(a))
        pix = np.ones((hh, ww, 4), np.float32)
        pix[..., :3] = x * g[..., None]
        # B3
        if b.flags & KARIS:
            wgt = (f32(1.0) / (f32(1.0) + _lum(pix[..., :3])).astype(np.float32)).astype(np.float32)
            pix[..., :3] = pix[..., :3] * wgt[..., None]
            pix[..., 3] = wgt
        # B4
        levels = []
        src = pix
        for l in range(1, b.levels + 1):
            v = _down(src)
            if l == 1 and b.flags & KARIS:
                v = np.concatenate([(v[..., :3] / v[..., 3:]).astype(np.float32), np.ones_like(v[..., 3:])], axis=2)
            levels.append(v)
            src = v
        # B6
        u = levels[-1]
        for l in range(b.levels - 1, 0, -1):
            dl = levels[l - 1]
            u = (dl + _up(u, dl.shape[1], dl.shape[0])).astype(np.float32)
        # B7, B8
        glow = (_up(u[..., :3], ww, hh) * f32(f32(1.0) / f32(b.levels))).astype(np.float32)
        f = _h((x + (gain * glow).astype(np.float32)).astype(np.float32))
        t = (e * f).astype(np.float32)
        if op == "reinhard":
            t = (t / (f32(1.0) + t).astype(np.float32)).astype(np.float32)
        c = np.where(t < f32(0.0), f32(0.0), t)
        c = np.where(f32(1.0) < c, f32(1.0), c)
        q = np.rint((c * f32(255.0)).astype(np.float32))
    rgba = np.full((hh, ww, 4), 255, np.uint8)
    rgba[..., :3] = np.where(np.isnan(t), 0, q).astype(np.uint8)
    return (f, rgba, levels, glow) if detail else (f, rgba)
