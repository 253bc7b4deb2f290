"""The oracle at any initRNG sample index (tests/oracle_samples.c) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_samples.c with oracle/Makefile's flags together with the other three oracle sources into a
shared library in tmp_dir; render_sample() runs it on an oracle_py scene."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
CFLAGS = ["-O3", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]   # oracle/Makefile


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_samples.so")
    srcs = [os.path.join(ROOT, "tests", "oracle_samples.c")] + [os.path.join(ORACLE, f) for f in
                                                                ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_render_sample.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.o_render_sample.restype = None
    return L


def render_sample(L, scene, width, height, mode, sample, row0=0, row1=None):
    """-> (rgba8[H,W,4], id_dist[H,W,2]) of sample `sample` (rows outside [row0, row1) stay zero)"""
    row1 = height if row1 is None else row1
    rgba = np.zeros((height, width, 4), np.uint8)
    idd = np.zeros((height, width, 2), np.int32)
    s = int(sample)
    s = s - (1 << 32) if s >= 1 << 31 else s   # the C int of the same bits
    L.o_render_sample(C.addressof(scene), width, height, row0, row1, mode, s, rgba.ctypes.data, idd.ctypes.data)
    return rgba, idd
