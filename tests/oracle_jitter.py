"""The oracle at any jittered sample of the progressive accumulation (tests/oracle_jitter.c) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_jitter.c with oracle/Makefile's flags together with the other three oracle sources into a
shared library in tmp_dir; render() runs it on an oracle_py scene, offsets() returns the sequence's (jx, jy)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
CFLAGS = ["-O3", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]   # oracle/Makefile


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_jitter.so")
    srcs = [os.path.join(ROOT, "tests", "oracle_jitter.c")] + [os.path.join(ORACLE, f) for f in
                                                               ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_render_jittered.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p,
                                    C.c_void_p]
    L.o_render_jittered.restype = None
    L.o_jitter_offsets.argtypes = [C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.o_jitter_offsets.restype = None
    return L


def offsets(L, k):
    """-> (jx, jy) of sample k as float32"""
    jx, jy = C.c_float(), C.c_float()
    L.o_jitter_offsets(int(k) & 0xFFFFFFFF, C.byref(jx), C.byref(jy))
    return np.float32(jx.value), np.float32(jy.value)


def render(L, scene, width, height, mode, sample, jitter=True, row0=0, row1=None):
    """-> (rgba8[H,W,4], id_dist[H,W,2]) of sample `sample` (rows outside [row0, row1) stay zero)"""
    row1 = height if row1 is None else row1
    rgba = np.zeros((height, width, 4), np.uint8)
    idd = np.zeros((height, width, 2), np.int32)
    L.o_render_jittered(C.addressof(scene), width, height, row0, row1, mode, int(sample) & 0xFFFFFFFF, 1 if jitter else 0,
                        rgba.ctypes.data, idd.ctypes.data)
    return rgba, idd
