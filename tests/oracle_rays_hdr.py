"""The oracle's float colour for ray batches and the arithmetic of vrt_shade_rays_hdr (tests/oracle_rays_hdr.c, which includes
tests/oracle_hdr.c unchanged) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_rays_hdr.c with oracle/Makefile's flags together with the other three oracle sources into a
shared library in tmp_dir, with oracle_hdr's prototypes on it, so that oracle_hdr.unorm8 / tonemap work on it as they do on
oracle_hdr's own library. shade() is one sample's float colour per ray; Batch restates a call (or a chain of calls through
d_sums): float64 sums in sample order, the mean over n_prior + n_samples, the tone-mapped bytes."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_hdr

ROOT = oracle_hdr.ROOT
ORACLE = oracle_hdr.ORACLE
CFLAGS = oracle_hdr.CFLAGS


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_rays_hdr.so")
    srcs = [os.path.join(ROOT, "tests", "oracle_rays_hdr.c")] + [os.path.join(ORACLE, f) for f in
                                                                 ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_shade_rays_hdr.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p]
    L.o_shade_rays_hdr.restype = None
    L.o_hdr_sum_repeat.argtypes = [C.c_float, C.c_uint32]
    L.o_hdr_sum_repeat.restype = C.c_double
    L.o_hdr_unorm8.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.o_hdr_unorm8.restype = None
    L.o_hdr_value.argtypes = [C.c_float]
    L.o_hdr_value.restype = C.c_float
    L.o_hdr_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.o_hdr_add.restype = None
    L.o_hdr_product.argtypes = [C.c_float, C.c_uint32]
    L.o_hdr_product.restype = C.c_double
    L.o_hdr_mean.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.o_hdr_mean.restype = None
    L.o_hdr_tonemap.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_void_p]
    L.o_hdr_tonemap.restype = None
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
    """-> (rgb float32[n,3], id_dist[n,2]): what pathTrace returns for the batch at sample `sample`; origins (n, 3) or (3,) shared"""
    o, stride, d = _rays(origins, dirs)
    n = d.shape[0]
    rgb = np.zeros((n, 3), np.float32)
    idd = np.zeros((n, 2), np.int32)
    s = int(sample) & 0xFFFFFFFF
    s = s - (1 << 32) if s >= 1 << 31 else s   # the C int of the same bits
    L.o_shade_rays_hdr(C.addressof(scene), n, o.ctypes.data, stride, d.ctypes.data, int(n if width is None else width), int(mode), s,
                       rgb.ctypes.data, idd.ctypes.data)
    return rgb, idd


def tonemap(L, mean, op="clamp", exposure=1.0):
    """float32[n,3] -> rgba8[n,4] (oracle_hdr.tonemap on a one-row image)"""
    return oracle_hdr.tonemap(L, np.ascontiguousarray(mean, np.float32)[None], op, exposure)[0]


class Batch:
    """vrt_shade_rays_hdr restated: sums (float64[n,3], +0.0 or the caller's) take each call's samples, the mean divides by all"""

    def __init__(self, L, scene, origins, dirs, mode, width=None, sums=None):
        self.L, self.scene, self.o, self.d, self.mode, self.width = L, scene, origins, dirs, mode, width
        n = np.asarray(dirs).shape[0]
        self.sums = np.zeros((n, 3), np.float64) if sums is None else np.array(sums, np.float64)
        self.n = 0
        self.id_dist = None

    def add(self, first_sample, n_samples):
        L = self.L
        if self.mode == 2:
            for k in range(n_samples):
                rgb, idd = shade(L, self.scene, self.o, self.d, 2, self.width, (first_sample + k) & 0xFFFFFFFF)
                L.o_hdr_add(self.sums.ctypes.data, rgb.ctypes.data, None, rgb.size)
                self.id_dist = idd if self.id_dist is None else self.id_dist
        else:   # one multiply and one add
            rgb, self.id_dist = shade(L, self.scene, self.o, self.d, self.mode, self.width, first_sample)
            prod = np.array([L.o_hdr_product(C.c_float(v.item()), n_samples) for v in rgb.ravel()], np.float64).reshape(rgb.shape)
            self.sums = self.sums + prod
        self.n += n_samples
        return self

    def mean(self):
        counts = np.full(self.sums.shape[0], self.n, np.uint32)
        out = np.zeros(self.sums.shape, np.float32)
        self.L.o_hdr_mean(self.sums.ctypes.data, counts.ctypes.data, counts.size, out.ctypes.data)
        return out
