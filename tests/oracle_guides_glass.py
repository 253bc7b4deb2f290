"""Guides past glass on the oracle's own march (tests/oracle_guides_glass.c) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_guides_glass.c (which includes oracle_guides.c) with oracle/Makefile's flags together with the other
three oracle sources into a shared library in tmp_dir; the library holds oracle_guides.c's entry points too, so tests/oracle_guides.py's
functions run on it. sample() is one sample's past-glass guide of every pixel, rays() that of a caller's rays, both with the surface
count S and the final surface's voxel ID; planes() and ray_planes() are oracle_guides.py's over them."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_guides as G

ROOT, ORACLE, KEYS, same = G.ROOT, G.ORACLE, G.KEYS, G.same
PLANT = {None: 0, "ratio_inverted": 1, "depth_straight": 2, "alpha_of_final": 3, "nudge_outwards": 4}


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_guides_glass.so")
    srcs = [os.path.join(ROOT, "tests", "oracle_guides_glass.c")] + [os.path.join(ORACLE, f) for f in
                                                                     ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *G.CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_guide_sample.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 5
    L.o_guide_sample.restype = None
    L.o_guide_rays.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 5
    L.o_guide_rays.restype = None
    L.o_guide_add.argtypes = [C.c_size_t] + [C.c_void_p] * 8
    L.o_guide_add.restype = None
    L.o_guide_resolve.argtypes = [C.c_size_t, C.c_uint32] + [C.c_void_p] * 8
    L.o_guide_resolve.restype = None
    L.o_glass_sample.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 7
    L.o_glass_sample.restype = None
    L.o_glass_rays.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7
    L.o_glass_rays.restype = None
    return L


class Guide(G.Guide):
    """oracle_guides.Guide and, per sample, surfaces int32[...] (S) and vid int32[...] (the final surface's voxel ID)"""

    def __init__(self, shape):
        super().__init__(shape)
        self.surfaces = np.zeros(shape, np.int32)
        self.vid = np.zeros(shape, np.int32)

    def _ptrs(self):
        return super()._ptrs() + [self.surfaces.ctypes.data, self.vid.ctypes.data]


def sample(L, scene, width, height, k, jitter=False, aperture=0.0, focus=1.0, plant=None):
    g = Guide((height, width))
    L.o_glass_sample(C.addressof(scene), width, height, int(k) & 0xFFFFFFFF, 1 if jitter else 0, float(aperture), float(focus),
                     PLANT[plant], *g._ptrs())
    return g


def rays(L, scene, origins, dirs, plant=None):
    """origins float32 (n, 3) or (3,) shared, dirs float32 (n, 3) as given"""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    o = np.ascontiguousarray(origins, np.float32)
    stride = 0 if o.ndim == 1 else 3
    g = Guide((d.shape[0],))
    L.o_glass_rays(C.addressof(scene), d.shape[0], o.ctypes.data, stride, d.ctypes.data, PLANT[plant], *g._ptrs())
    return g


def planes(L, scene, width, height, first, n, jitter=False, aperture=0.0, focus=1.0, plant=None, state=None):
    """the past-glass planes after samples first .. first + n - 1 (added to `state` when one is given) -> (dict, State)"""
    st = state or G.State(L, (height, width))
    for k in range(first, first + n):
        st.add(sample(L, scene, width, height, k, jitter, aperture, focus, plant))
    return st.resolve(), st


def ray_planes(L, scene, origins, dirs):
    """vrt_guide_rays' outputs with the setting on: the planes of n = 1 and the hit bytes"""
    g = rays(L, scene, origins, dirs)
    st = G.State(L, g.hit.shape)
    st.add(g)
    out = st.resolve()
    return {"normal": out["normal"], "albedo": out["albedo"], "depth": out["depth"], "hit": g.hit != 0}
