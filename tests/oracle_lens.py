"""The oracle at any thin-lens sample of the progressive accumulation (tests/oracle_lens.c) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_lens.c with oracle/Makefile's flags together with the other three oracle sources into a shared
library in tmp_dir; render() runs it on an oracle_py scene, point() and uv() return the lens sequence, ray() one sample's ray."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
CFLAGS = ["-O3", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]   # oracle/Makefile
F = C.POINTER(C.c_float)


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_lens.so")
    srcs = [os.path.join(ROOT, "tests", "oracle_lens.c")] + [os.path.join(ORACLE, f) for f in
                                                             ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_render_lens.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_float,
                                C.c_float, C.c_void_p, C.c_void_p]
    L.o_render_lens.restype = None
    L.o_lens_uv.argtypes = [C.c_uint32, F, F]
    L.o_lens_uv.restype = None
    L.o_lens_point.argtypes = [C.c_uint32, F, F]
    L.o_lens_point.restype = None
    L.o_lens_ray.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_float, C.c_float, F, F]
    L.o_lens_ray.restype = C.c_int
    return L


def uv(L, k):
    """-> (lu, lv) of sample k as float32"""
    a, b = C.c_float(), C.c_float()
    L.o_lens_uv(int(k) & 0xFFFFFFFF, C.byref(a), C.byref(b))
    return np.float32(a.value), np.float32(b.value)


def point(L, k):
    """-> (lx, ly) of sample k on the unit disc, float32"""
    a, b = C.c_float(), C.c_float()
    L.o_lens_point(int(k) & 0xFFFFFFFF, C.byref(a), C.byref(b))
    return np.float32(a.value), np.float32(b.value)


def ray(L, scene, width, height, px, py, sample, aperture, focus, jitter=False):
    """-> (moved, origin float32[3], direction float32[3]) of pixel (px, py) at sample `sample`"""
    o = (C.c_float * 3)()
    d = (C.c_float * 3)()
    moved = L.o_lens_ray(C.addressof(scene), width, height, px, py, int(sample) & 0xFFFFFFFF, 1 if jitter else 0,
                         float(aperture), float(focus), o, d)
    return bool(moved), np.array(o[:], np.float32), np.array(d[:], np.float32)


def render(L, scene, width, height, mode, sample, aperture, focus, jitter=False, row0=0, row1=None):
    """-> (rgba8[H,W,4], id_dist[H,W,2]) of lens sample `sample` (rows outside [row0, row1) stay zero)"""
    row1 = height if row1 is None else row1
    rgba = np.zeros((height, width, 4), np.uint8)
    idd = np.zeros((height, width, 2), np.int32)
    L.o_render_lens(C.addressof(scene), width, height, row0, row1, mode, int(sample) & 0xFFFFFFFF, 1 if jitter else 0,
                    float(aperture), float(focus), rgba.ctypes.data, idd.ctypes.data)
    return rgba, idd
