"""The guide planes on the oracle's own march (tests/oracle_guides.c) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_guides.c with oracle/Makefile's flags together with the other three oracle sources into a shared
library in tmp_dir. sample() is one sample's guide of every pixel, rays() that of a caller's rays; State restates the sums and the
resolve of include/vrt.h vrt_accum_guides; planes() runs a whole accumulation's guides; ray_planes() the planes of a batch."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
CFLAGS = ["-O3", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]   # oracle/Makefile
PLANT = {None: 0, "normal_sign": 1, "depth_from_eye": 2}
KEYS = ("normal", "albedo", "depth", "coverage")


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_guides.so")
    srcs = [os.path.join(ROOT, "tests", "oracle_guides.c")] + [os.path.join(ORACLE, f) for f in
                                                               ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_guide_sample.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 5
    L.o_guide_sample.restype = None
    L.o_guide_rays.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 5
    L.o_guide_rays.restype = None
    L.o_guide_add.argtypes = [C.c_size_t] + [C.c_void_p] * 8
    L.o_guide_add.restype = None
    L.o_guide_resolve.argtypes = [C.c_size_t, C.c_uint32] + [C.c_void_p] * 8
    L.o_guide_resolve.restype = None
    return L


class Guide:
    """one sample's guide: normal int8[..., 3], albedo uint8[..., 4], depth float32[...], hit uint8[...], cell int32[..., 3]"""

    def __init__(self, shape):
        self.normal = np.zeros(shape + (3,), np.int8)
        self.albedo = np.zeros(shape + (4,), np.uint8)
        self.depth = np.zeros(shape, np.float32)
        self.hit = np.zeros(shape, np.uint8)
        self.cell = np.zeros(shape + (3,), np.int32)

    def _ptrs(self):
        return [a.ctypes.data for a in (self.normal, self.albedo, self.depth, self.hit, self.cell)]


def sample(L, scene, width, height, k, jitter=False, aperture=0.0, focus=1.0, plant=None):
    g = Guide((height, width))
    L.o_guide_sample(C.addressof(scene), width, height, int(k) & 0xFFFFFFFF, 1 if jitter else 0, float(aperture), float(focus),
                     PLANT[plant], *g._ptrs())
    return g


def rays(L, scene, origins, dirs):
    """origins float32 (n, 3) or (3,) shared, dirs float32 (n, 3) as given"""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    o = np.ascontiguousarray(origins, np.float32)
    stride = 0 if o.ndim == 1 else 3
    g = Guide((d.shape[0],))
    L.o_guide_rays(C.addressof(scene), d.shape[0], o.ctypes.data, stride, d.ctypes.data, *g._ptrs())
    return g


class State:
    """the 40 bytes per pixel: uint32[4], int32[3], uint32, double"""

    def __init__(self, L, shape):
        self.L, self.shape, self.n = L, tuple(shape), 0
        self.asum = np.zeros(self.shape + (4,), np.uint32)
        self.nsum = np.zeros(self.shape + (3,), np.int32)
        self.hits = np.zeros(self.shape, np.uint32)
        self.dsum = np.zeros(self.shape, np.float64)

    def add(self, g):
        self.L.o_guide_add(self.hits.size, g.normal.ctypes.data, g.albedo.ctypes.data, g.depth.ctypes.data, g.hit.ctypes.data,
                           self.asum.ctypes.data, self.nsum.ctypes.data, self.hits.ctypes.data, self.dsum.ctypes.data)
        self.n += 1

    def resolve(self):
        out = {"normal": np.zeros(self.shape + (3,), np.float32), "albedo": np.zeros(self.shape + (4,), np.float32),
               "depth": np.zeros(self.shape, np.float32), "coverage": np.zeros(self.shape, np.float32)}
        self.L.o_guide_resolve(self.hits.size, self.n, self.asum.ctypes.data, self.nsum.ctypes.data, self.hits.ctypes.data,
                               self.dsum.ctypes.data, out["normal"].ctypes.data, out["albedo"].ctypes.data, out["depth"].ctypes.data,
                               out["coverage"].ctypes.data)
        return out


def planes(L, scene, width, height, first, n, jitter=False, aperture=0.0, focus=1.0, plant=None, state=None):
    """the planes after samples first .. first + n - 1 (added to `state` when one is given) -> (dict, State)"""
    st = state or State(L, (height, width))
    for k in range(first, first + n):
        st.add(sample(L, scene, width, height, k, jitter, aperture, focus, plant))
    return st.resolve(), st


def ray_planes(L, scene, origins, dirs):
    """vrt_guide_rays' outputs: the planes of n = 1 and the hit bytes"""
    g = rays(L, scene, origins, dirs)
    st = State(L, g.hit.shape)
    st.add(g)
    out = st.resolve()
    return {"normal": out["normal"], "albedo": out["albedo"], "depth": out["depth"], "hit": g.hit != 0}


def same(got, want, what, keys=KEYS):
    """bit for bit on every plane"""
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        gb, wb = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        if not np.array_equal(gb, wb):
            bad = np.argwhere(gb != wb)
            i = tuple(bad[0])
            raise AssertionError(f"{what}: {k} differs at {len(bad)} entries; first at {i}: got {g[i]!r} want {w[i]!r}")
