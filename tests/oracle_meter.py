"""Light metering restated twice -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles tests/oracle_meter.c (E1-E9 of include/vrt.h vrt_meter_hdr in scalar C) as tests/oracle_upsample.py compiles
its library; histogram(), resolve() and tonemap() call it, PLANT names its planted misreadings. The second restatement is Python:
E3-E6 in Python's big integers (py_bins, py_histogram, py_sums, py_metered), E1, E7, E8 and E9 in float32 numpy scalars, one
operation per expression (py_luminance, py_resolve, py_tonemap). The two share no code."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_hdr

BINS = 256
PLANT = {None: 0, "centre_left_out": 1, "black_in_sums": 2, "window_over_non_black": 3, "adapt_on_first_frame": 4,
         "tm_exposure_ignored": 5}
OPS = oracle_hdr.OPS
KEYS = ("key", "low_permille", "high_permille", "min_exposure", "max_exposure", "adapt", "x0", "y0", "x1", "y1")
F32_MAX = np.float32(3.402823466e38)


class Meter(C.Structure):
    """include/vrt.h vrt_meter"""
    _fields_ = [("key", C.c_float), ("low_permille", C.c_int32), ("high_permille", C.c_int32), ("min_exposure", C.c_float),
                ("max_exposure", C.c_float), ("adapt", C.c_float), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32)]


class Exposure(C.Structure):
    """include/vrt.h vrt_exposure"""
    _fields_ = [("exposure", C.c_float), ("metered", C.c_float), ("window", C.c_uint32), ("frames", C.c_uint32)]


def make(key=0.18, low=500, high=950, min_exposure=2.0 ** -10, max_exposure=2.0 ** 10, adapt=1.0, rect=(0, 0, 0, 0)):
    return Meter(key, low, high, min_exposure, max_exposure, adapt, *rect)


def keys(m):
    """a Meter as the dict the package's `meter` arguments take"""
    return {k: getattr(m, k) for k in KEYS}


def record(e):
    """an Exposure as the dict the package returns"""
    return {"exposure": float(e.exposure), "metered": float(e.metered), "window": int(e.window), "frames": int(e.frames)}


def from_record(d):
    return Exposure() if d is None else Exposure(d["exposure"], d["metered"], d["window"], d["frames"])


def bits(d):
    """a record's four words as integers: equality of these is equality bit for bit (-0.0 and NaN payloads included)"""
    f = np.array([d["exposure"], d["metered"]], np.float32).view(np.uint32)
    return (int(f[0]), int(f[1]), int(d["window"]), int(d["frames"]))


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_meter.so")
    srcs = [os.path.join(oracle_hdr.ROOT, "tests", "oracle_meter.c")] + [os.path.join(oracle_hdr.ORACLE, f) for f in
                                                                        ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *oracle_hdr.CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_meter_luminance.argtypes = [C.c_float] * 3
    L.o_meter_luminance.restype = C.c_float
    L.o_meter_bin.argtypes = [C.c_float]
    L.o_meter_bin.restype = C.c_int
    L.o_meter_histogram.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
    L.o_meter_histogram.restype = None
    L.o_meter_resolve.argtypes = [C.c_void_p, C.POINTER(Meter), C.POINTER(Exposure), C.c_int]
    L.o_meter_resolve.restype = C.c_uint64
    L.o_meter_tonemap.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.POINTER(Exposure), C.c_int, C.c_void_p]
    L.o_meter_tonemap.restype = None
    return L


def histogram(L, rgb, rect=(0, 0, 0, 0)):
    """rgb float32[H,W,3] -> uint32[BINS] of the rectangle (E1-E3)"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    assert rgb.shape == (h, w, 3)
    hist = np.zeros(BINS, np.uint32)
    L.o_meter_histogram(rgb.ctypes.data, w, h, *rect, hist.ctypes.data)
    return hist


def resolve(L, hist, m, state=None, plant=None):
    """E4-E8: hist, a Meter, the previous record as a dict (None: zeroed) -> the new record as a dict"""
    hist = np.ascontiguousarray(hist, np.uint32)
    assert hist.shape == (BINS,)
    e = from_record(state)
    L.o_meter_resolve(hist.ctypes.data, C.byref(m), C.byref(e), PLANT[plant])
    return record(e)


def meter(L, rgb, m, state=None, plant=None):
    """E1-E8 on an image -> (record, histogram)"""
    hist = histogram(L, rgb, (m.x0, m.y0, m.x1, m.y1))
    return resolve(L, hist, m, state, plant), hist


def tonemap(L, rgb, op="clamp", exposure=1.0, state=None, plant=None):
    """E9: rgb float32[..., 3] -> uint8[..., 4]; state None: no record; op None: the NULL vrt_tonemap"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    out = np.zeros(rgb.shape[:-1] + (4,), np.uint8)
    if op is None:
        op, exposure = "clamp", 1.0
    e = None if state is None else C.byref(from_record(state))
    L.o_meter_tonemap(rgb.ctypes.data, rgb.size // 3, OPS[op], float(np.float32(exposure)), e, PLANT[plant], out.ctypes.data)
    return out


# ---- the Python restatement ----

def _h(c):
    """h(c) on float32 arrays: min(max(0, c), 65504) in the store's conventions, NaN -> +0"""
    c = np.asarray(c, np.float32)
    z = np.where(np.float32(0.0) < c, c, np.float32(0.0))          # max(0, c) = 0 < c ? c : 0
    return np.where(np.float32(65504.0) < z, np.float32(65504.0), z).astype(np.float32)   # min(z, 65504) = 65504 < z ? 65504 : z


def py_luminance(rgb):
    """E1 on float32[..., 3], every operation a float32 numpy operation of its own"""
    rgb = np.asarray(rgb, np.float32)
    r, g, b = _h(rgb[..., 0]), _h(rgb[..., 1]), _h(rgb[..., 2])
    return ((np.float32(0.2126) * r + np.float32(0.7152) * g).astype(np.float32) + np.float32(0.0722) * b).astype(np.float32)


def py_bins(y):
    """E2 on float32 luminances -> Python-sized integers"""
    k = (np.ascontiguousarray(y, np.float32).view(np.uint32) >> 20).astype(np.int64) - 888
    return np.maximum(k, 0)


def py_histogram(rgb, rect=(0, 0, 0, 0)):
    """E1-E3 -> a list of BINS Python integers"""
    rgb = np.asarray(rgb, np.float32)
    x0, y0, x1, y1 = rect
    if not any(rect):
        y1, x1 = rgb.shape[:2]
    return np.bincount(py_bins(py_luminance(rgb[y0:y1, x0:x1])).ravel(), minlength=BINS).tolist()


def py_sums(hist, low, high):
    """E4, E5 in big integers -> (N, M, S)"""
    hist = [int(v) for v in hist]
    n = sum(hist)
    a, b = n * low // 1000, n * high // 1000
    cum = big_m = big_s = 0
    for k, c in enumerate(hist):
        lo, hi = max(cum, a), min(cum + c, b)
        cum += c
        if k >= 1 and hi > lo:
            big_m += hi - lo
            big_s += (hi - lo) * k
    return n, big_m, big_s


def py_metered(big_m, big_s):
    """E6 -> float32 (the +0.0 of M = 0 included)"""
    if big_m == 0:
        return np.float32(0.0)
    word = (888 << 20) + (big_s << 20) // big_m + (1 << 19)
    assert 0 < word < 1 << 31
    return np.array([word], np.uint32).view(np.float32)[0]


def _min(a, b):
    return b if b < a else a


def _max(a, b):
    return b if a < b else a


def py_resolve(hist, m, state=None):
    """E4-E8 -> the record as a dict"""
    f = np.float32
    prev_e, frames = (f(0.0), 0) if state is None else (f(state["exposure"]), int(state["frames"]))
    _, big_m, big_s = py_sums(hist, m.low_permille, m.high_permille)
    ym = py_metered(big_m, big_s)
    lo, hi = f(m.min_exposure), f(m.max_exposure)
    if big_m:
        target = _min(_max(f(m.key) / ym, lo), hi)
    else:
        target = prev_e if frames > 0 else _min(_max(f(1.0), lo), hi)
    e = target
    if not (f(m.adapt) == f(1.0) or frames == 0 or big_m == 0):
        d = f(target - prev_e)
        e = f(prev_e + f(f(m.adapt) * d))
    return {"exposure": float(e), "metered": float(ym), "window": big_m, "frames": min(frames + 1, 0xffffffff)}


def py_tonemap(rgb, op="clamp", exposure=1.0, state=None):
    """E9 in float32 numpy -> uint8[..., 4]"""
    f = np.float32
    rgb = np.asarray(rgb, np.float32)
    e = f(exposure)
    if state is not None:
        with np.errstate(over="ignore"):
            e = _min(f(e * f(state["exposure"])), F32_MAX)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        y = (e * rgb).astype(np.float32)
        if op == "reinhard":
            y = (y / (f(1.0) + y).astype(np.float32)).astype(np.float32)
        # unorm8: clamp to [0, 1] in the store's conventions, scale, round to nearest even; NaN stores 0
        c = np.where(y < f(0.0), f(0.0), y)
        c = np.where(f(1.0) < c, f(1.0), c)
        q = np.rint((c * f(255.0)).astype(np.float32))
    out = np.full(rgb.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = np.where(np.isnan(y), 0, q).astype(np.uint8)
    return out
