"""pathTrace with a path depth and a sun disc (tests/oracle_sun.c; include/vrt.h vrt_set_sun_disc) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_sun.c with oracle/Makefile's flags together with the other three oracle sources into a shared
library in tmp_dir, the way oracle_path_depth.py builds its own. shade() traces a batch at one sample, one depth and one radius
-> bytes, (voxel ID, dist), the unclamped float colour and, on request, the vertex log; mean() is the exact mean of a sample
range by the accumulation's resolve rule; restate() sums a log's contributions in float64 by the rule's formulas (the DIRECT
term with the logged lit and ndotl', which the sun disc changes and nothing else). The HDR arithmetic (float64 sums, mean, tone
maps) is tests/oracle_hdr.c's, through oracle_hdr / oracle_rays_hdr on the floats shade() returns."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_path_depth as opd

ROOT = opd.ROOT
ORACLE = opd.ORACLE
CFLAGS = opd.CFLAGS   # oracle/Makefile
MAX_DEPTH = opd.MAX_DEPTH

SKY0, SKY, GLASS, EMIT0, EMIT, DIRECT, AMBIENT = range(7)   # o_sun_vertex.kind, as oracle_path_depth's
VERTEX = np.dtype(opd.VERTEX.descr + [("u1", np.float32), ("u2", np.float32), ("dx", np.float32), ("dy", np.float32),
                                      ("lp", np.float32, 3), ("rx", np.float32), ("ry", np.float32), ("normal", np.float32, 3),
                                      ("shadow_steps", np.int32)])
assert VERTEX.itemsize == 56 + 52


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_sun.so")
    srcs = [os.path.join(ROOT, "tests", "oracle_sun.c")] + [os.path.join(ORACLE, f) for f in
                                                            ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_shade_rays_sun.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.o_shade_rays_sun.restype = C.c_size_t
    L.o_sun_disc_map.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.o_sun_disc_map.restype = None
    L.o_sun_basis.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
    L.o_sun_basis.restype = None
    for name in ("o_det_sinf", "o_det_cosf"):   # the probes of the conventions' sin / cos
        getattr(L, name).argtypes = [C.c_float]
        getattr(L, name).restype = C.c_float
    return L


def basis(L, light_dir, tan_radius):
    """-> (tan_radius, ll, Ln[3], T[3], B[3]) as the checker makes them (float32)"""
    ld = np.ascontiguousarray(light_dir, np.float32)
    out = np.zeros(11, np.float32)
    L.o_sun_basis(ld.ctypes.data, float(tan_radius), out.ctypes.data)
    return out[0], out[1], out[2:5].copy(), out[5:8].copy(), out[8:11].copy()


def shade(L, scene, origins, dirs, depth, tan_radius, width=None, sample=0, log=False):
    """-> (rgba8[n,4], id_dist[n,2], rgb float32[n,3]) of the batch at sample `sample`, path depth `depth` and sun disc
    `tan_radius`, in VRT_MODE_FULL; with log=True also the vertex log (a VERTEX array, in the order the contributions were
    added). origins (n, 3) or (3,) shared"""
    assert 1 <= depth <= MAX_DEPTH and 0.0 <= tan_radius <= 1.0
    o, stride, d = opd._rays(origins, dirs)
    n = d.shape[0]
    rgba = np.zeros((n, 4), np.uint8)
    idd = np.zeros((n, 2), np.int32)
    rgb = np.zeros((n, 3), np.float32)
    s = int(sample) & 0xFFFFFFFF
    s = s - (1 << 32) if s >= 1 << 31 else s   # the C int of the same bits
    w = int(n if width is None else width)
    if log:   # once to count the records, once to take them
        dummy = np.zeros(1, VERTEX)
        cap = L.o_shade_rays_sun(C.addressof(scene), n, o.ctypes.data, stride, d.ctypes.data, w, int(depth), float(tan_radius), s, None,
                                 None, None, dummy.ctypes.data, 0)
    vlog = np.zeros(max(cap, 1) if log else 1, VERTEX)
    got = L.o_shade_rays_sun(C.addressof(scene), n, o.ctypes.data, stride, d.ctypes.data, w, int(depth), float(tan_radius), s,
                             rgba.ctypes.data, idd.ctypes.data, rgb.ctypes.data, vlog.ctypes.data if log else None, cap if log else 0)
    if log:
        assert got == cap, "vertex log cut"
        return rgba, idd, rgb, vlog[:got]
    return rgba, idd, rgb


def mean(L, scene, origins, dirs, depth, tan_radius, width=None, first_sample=0, n_samples=1):
    """The exact mean of samples first_sample .. first_sample + n_samples - 1 (indices modulo 2^32): per channel the integer sum
    of the samples' bytes, resolved as (sum + n / 2) / n, alpha 255 -> (rgba8[n,4], id_dist[n,2] of the first sample)"""
    total = None
    idd0 = None
    for k in range(n_samples):
        rgba, idd, _ = shade(L, scene, origins, dirs, depth, tan_radius, width, (first_sample + k) & 0xFFFFFFFF)
        total = rgba.astype(np.uint64) if total is None else total + rgba
        idd0 = idd if idd0 is None else idd0
    out = ((total + n_samples // 2) // n_samples).astype(np.uint8)
    out[:, 3] = 255
    return out, idd0


def restate(vlog, n_rays, global_light):
    """float64[n_rays, 3]: the logged contributions summed by the rule's formulas; the record's first fields are
    oracle_path_depth's, and a DIRECT record's lit and ndotl are the sun disc's lit and ndotl'"""
    return opd.restate(vlog, n_rays, global_light)
