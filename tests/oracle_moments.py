"""The luminance moments of an HDR accumulation (tests/oracle_moments.c: M1-M3 of include/vrt.h vrt_accum_keep_moments) -- TEST
INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_moments.c (which includes oracle_hdr.c) with the oracle's flags and declares oracle_hdr's functions
and its own, so every oracle_hdr helper works on the library. Accum is oracle_hdr.Accum with the two float64 sums beside the colour
sums -- the same pixels take the same samples -- and variance() the M3 plane; plant names one deliberate misreading of the rule."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_hdr

PLANT = {None: 0, "divisor_n": 1, "square_in_double": 2, "y_of_bytes": 3}
VAR_UNKNOWN = np.float32(65504.0) * np.float32(65504.0)


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_moments.so")
    srcs = [os.path.join(oracle_hdr.ROOT, "tests", "oracle_moments.c")] + [os.path.join(oracle_hdr.ORACLE, f) for f in
                                                                          ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *oracle_hdr.CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    # oracle_hdr.build()'s declarations
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
    L.o_hdr_mean.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.o_hdr_mean.restype = None
    L.o_hdr_tonemap.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_void_p]
    L.o_hdr_tonemap.restype = None
    # ... and this file's
    L.o_mom_luminance.argtypes = [C.c_void_p, C.c_int]
    L.o_mom_luminance.restype = C.c_float
    L.o_mom_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.o_mom_add.restype = None
    L.o_mom_sum_repeat.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.o_mom_sum_repeat.restype = None
    L.o_mom_add_product.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.o_mom_add_product.restype = None
    L.o_mom_variance.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.o_mom_variance.restype = None
    return L


def luminance(L, rgb, plant=None):
    """M1's y of every pixel of rgb float32[..., 3] -> float32[...]"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    flat = rgb.reshape(-1, 3)
    out = np.array([L.o_mom_luminance(flat[i:i + 1].ctypes.data, PLANT[plant]) for i in range(flat.shape[0])], np.float32)
    return out.reshape(rgb.shape[:-1])


def sum_repeat(L, c, k):
    """k sequential adds of the colour c to +0.0 -> float64[2]"""
    c = np.ascontiguousarray(c, np.float32)
    s = np.zeros(2, np.float64)
    L.o_mom_sum_repeat(c.ctypes.data, int(k), s.ctypes.data)
    return s


def add_product(L, c, k, s=None):
    """s + ((double)y * k, (double)q * k), s float64[2] (None: zeros) -> float64[2]"""
    c = np.ascontiguousarray(c, np.float32)
    s = np.zeros(2, np.float64) if s is None else np.array(s, np.float64)
    L.o_mom_add_product(c.ctypes.data, int(k), s.ctypes.data)
    return s


def variance_of(L, msum, counts, plant=None):
    """M3: msum float64[H,W,2], counts [H,W] -> float32[H,W]"""
    msum = np.ascontiguousarray(msum, np.float64)
    counts = np.ascontiguousarray(counts, np.uint32)
    out = np.zeros(counts.shape, np.float32)
    L.o_mom_variance(msum.ctypes.data, counts.ctypes.data, counts.size, PLANT[plant], out.ctypes.data)
    return out


class Accum(oracle_hdr.Accum):
    """oracle_hdr.Accum with S1 and S2 per pixel: each sample the pixel takes adds to them where it adds to the colour sums"""

    def __init__(self, L, height, width, rule=None, plant=None):
        super().__init__(L, height, width, rule)
        self.msum = np.zeros((height, width, 2), np.float64)
        self.plant = plant

    def add(self, rgb):
        rgb = np.ascontiguousarray(rgb, np.float32)
        rule = self.rule or (self.n + 1, self.n + 1, 0)
        take = np.ascontiguousarray(self.st.active(rule), np.uint8)   # the pixels the colour sums are about to add for
        self.L.o_mom_add(self.msum.ctypes.data, rgb.ctypes.data, take.ctypes.data, take.size, PLANT[self.plant])
        super().add(rgb)

    def variance(self, plant=None):
        return variance_of(self.L, self.msum, self.counts(), plant)


def resolve_filtered_var(LV, acc, guides, f, op="clamp", exposure=1.0):
    """What vrt_accum_resolve_hdr_filtered_var is specified to return for the accumulation `acc` (an Accum; LV: oracle_filter_var's
    library): the variance-guided filter on its mean and guide planes, fed the M3 plane once the accumulation holds two samples,
    the spatial estimate (no plane) with one -> (rgb, rgba8, variance)"""
    import oracle_filter_var as FV
    return FV.filter(LV, acc.mean(), guides, f, acc.variance() if acc.n >= 2 else None, op, exposure)
