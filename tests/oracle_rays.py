"""The oracle's pathTrace for ray batches (tests/oracle_rays.c) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_rays.c with oracle/Makefile's flags together with the other three oracle sources into a shared
library in tmp_dir; shade() traces a batch at one sample, mean() gives the exact mean of a sample range by the accumulation's
resolve rule, frame_rays() the rays o_render traces for a frame."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
CFLAGS = ["-O3", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]   # oracle/Makefile


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_rays.so")
    srcs = [os.path.join(ROOT, "tests", "oracle_rays.c")] + [os.path.join(ORACLE, f) for f in
                                                             ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_shade_rays.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                               C.c_void_p]
    L.o_shade_rays.restype = None
    L.o_frame_rays.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.o_frame_rays.restype = None
    return L


def _rays(origins, dirs):
    d = np.ascontiguousarray(dirs, np.float32)
    o = np.ascontiguousarray(origins, np.float32)
    assert d.ndim == 2 and d.shape[1] == 3
    if o.shape == (3,):
        return o, 0, d
    assert o.shape == d.shape
    return o, 3, d


def shade(L, scene, origins, dirs, mode, width=None, sample=0):
    """-> (rgba8[n,4], id_dist[n,2]) of the batch at sample `sample`; origins (n, 3) or (3,) shared"""
    o, stride, d = _rays(origins, dirs)
    n = d.shape[0]
    rgba = np.zeros((n, 4), np.uint8)
    idd = np.zeros((n, 2), np.int32)
    s = int(sample) & 0xFFFFFFFF
    s = s - (1 << 32) if s >= 1 << 31 else s   # the C int of the same bits
    L.o_shade_rays(C.addressof(scene), n, o.ctypes.data, stride, d.ctypes.data, int(n if width is None else width), int(mode), s,
                   rgba.ctypes.data, idd.ctypes.data)
    return rgba, idd


def mean(L, scene, origins, dirs, mode, width=None, first_sample=0, n_samples=1):
    """The exact mean of samples first_sample .. first_sample + n_samples - 1 (indices modulo 2^32): per channel the integer sum
    of the samples' bytes, resolved as (sum + n / 2) / n, alpha 255 -> (rgba8[n,4], id_dist[n,2] of the first sample)"""
    total = None
    idd0 = None
    for k in range(n_samples):
        rgba, idd = shade(L, scene, origins, dirs, mode, width, (first_sample + k) & 0xFFFFFFFF)
        total = rgba.astype(np.uint64) if total is None else total + rgba
        idd0 = idd if idd0 is None else idd0
    out = ((total + n_samples // 2) // n_samples).astype(np.uint8)
    out[:, 3] = 255
    return out, idd0


def frame_rays(L, scene, width, height):
    """-> (origins float32[W*H,3], dirs float32[W*H,3]): what o_render hands path_trace per pixel, row-major"""
    o = np.zeros((width * height, 3), np.float32)
    d = np.zeros((width * height, 3), np.float32)
    L.o_frame_rays(C.addressof(scene), width, height, o.ctypes.data, d.ctypes.data)
    return o, d
