"""The oracle's float colour at any sample of the progressive accumulation and the HDR accumulation's arithmetic
(tests/oracle_hdr.c) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_hdr.c with oracle/Makefile's flags together with the other three oracle sources into a shared
library in tmp_dir. render() is one sample's float colour; Accum restates an HDR accumulation (plain, or adaptive with
oracle_adaptive's rule on the bytes); tonemap() and unorm8() the resolve's byte side."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_adaptive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
CFLAGS = ["-O3", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]   # oracle/Makefile
OPS = {"clamp": 0, "reinhard": 1}


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_hdr.so")
    srcs = [os.path.join(ROOT, "tests", "oracle_hdr.c")] + [os.path.join(ORACLE, f) for f in
                                                            ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
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
    L.o_hdr_sum_repeat.argtypes = [C.c_float, C.c_uint32]
    L.o_hdr_sum_repeat.restype = C.c_double
    L.o_hdr_product.argtypes = [C.c_float, C.c_uint32]
    L.o_hdr_product.restype = C.c_double
    L.o_hdr_mean.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.o_hdr_mean.restype = None
    L.o_hdr_tonemap.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_void_p]
    L.o_hdr_tonemap.restype = None
    return L


def render(L, scene, width, height, mode, sample, jitter=False, aperture=0.0, focus=1.0):
    """-> float32[H,W,3]: the colour pathTrace returns for sample `sample` (corner: no jitter, aperture 0)"""
    rgb = np.zeros((height, width, 3), np.float32)
    L.o_render_hdr(C.addressof(scene), width, height, 0, height, mode, int(sample) & 0xFFFFFFFF, 1 if jitter else 0,
                   float(aperture), float(focus), rgb.ctypes.data)
    return rgb


def render_bytes(L, scene, width, height, mode, sample, jitter=False, aperture=0.0, focus=1.0):
    """-> (rgba8[H,W,4], id_dist[H,W,2]) of the same sample: tests/oracle_lens.c's o_render_lens"""
    rgba = np.zeros((height, width, 4), np.uint8)
    idd = np.zeros((height, width, 2), np.int32)
    L.o_render_lens(C.addressof(scene), width, height, 0, height, mode, int(sample) & 0xFFFFFFFF, 1 if jitter else 0,
                    float(aperture), float(focus), rgba.ctypes.data, idd.ctypes.data)
    return rgba, idd


def unorm8(L, v):
    """the unorm8 store of every float of v -> uint8, same shape"""
    v = np.ascontiguousarray(v, np.float32)
    out = np.zeros(v.shape, np.uint8)
    L.o_hdr_unorm8(v.ctypes.data, v.size, out.ctypes.data)
    return out


def rgba_of(L, rgb):
    """float32[H,W,3] -> the rgba8[H,W,4] a sample of that colour stores"""
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = unorm8(L, rgb)
    return out


def value(L, c):
    return np.float32(L.o_hdr_value(C.c_float(float(c)) if not isinstance(c, np.float32) else C.c_float(c.item())))


def tonemap(L, mean, op="clamp", exposure=1.0):
    """float32[H,W,3] -> rgba8[H,W,4]"""
    mean = np.ascontiguousarray(mean, np.float32)
    out = np.zeros(mean.shape[:2] + (4,), np.uint8)
    L.o_hdr_tonemap(mean.ctypes.data, mean.shape[0] * mean.shape[1], OPS[op], float(np.float32(exposure)), out.ctypes.data)
    return out


class Accum:
    """An HDR accumulation restated: float64 sums in sample order, the integer sums beside them; rule = (min, max, tolerance)
    makes it adaptive -- the rule on the bytes (oracle_adaptive), the float sums following the same pixels."""

    def __init__(self, L, height, width, rule=None):
        self.L, self.rule = L, rule
        self.hsum = np.zeros((height, width, 3), np.float64)
        self.st = oracle_adaptive.State(height, width, np.int64)
        self.n = 0

    def add(self, rgb):
        """one sample (plain) or one round (adaptive): rgb float32[H,W,3]"""
        rgb = np.ascontiguousarray(rgb, np.float32)
        rgba = rgba_of(self.L, rgb)
        rule = self.rule or (self.n + 1, self.n + 1, 0)   # plain: every pixel takes every sample
        act = self.st.active(rule)
        take = np.ascontiguousarray(np.repeat(act[..., None], 3, axis=2), np.uint8)
        self.L.o_hdr_add(self.hsum.ctypes.data, rgb.ctypes.data, take.ctypes.data, rgb.size)
        self.st.add_round(rgba, rule)
        self.n += 1

    def counts(self):
        return self.st.counts()

    def mean(self):
        counts = np.ascontiguousarray(np.maximum(self.counts(), 1), np.uint32)
        out = np.zeros(self.hsum.shape, np.float32)
        self.L.o_hdr_mean(self.hsum.ctypes.data, counts.ctypes.data, counts.size, out.ctypes.data)
        return out

    def resolve_bytes(self):
        return self.st.resolve()
