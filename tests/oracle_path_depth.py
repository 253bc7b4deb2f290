"""pathTrace with a path depth (tests/oracle_path_depth.c; include/vrt.h vrt_set_path_depth) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_path_depth.c with oracle/Makefile's flags together with the other three oracle sources into a
shared library in tmp_dir. shade() traces a batch at one sample and one depth -> bytes, (voxel ID, dist), the unclamped float
colour and, on request, the vertex log; mean() is the exact mean of a sample range by the accumulation's resolve rule;
restate() sums a log's contributions in float64 by the rule's formulas. The HDR arithmetic (float64 sums, mean, tone maps) is
tests/oracle_hdr.c's, through oracle_hdr / oracle_rays_hdr on the floats shade() returns."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
CFLAGS = ["-O3", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]   # oracle/Makefile
MAX_DEPTH = 8

SKY0, SKY, GLASS, EMIT0, EMIT, DIRECT, AMBIENT = range(7)   # o_pd_vertex.kind
VERTEX = np.dtype([("ray", np.uint32), ("kind", np.int32), ("depth", np.int32), ("chain", np.int32), ("lit", np.int32),
                   ("ndotl", np.float32), ("sc", np.float32, 3), ("tc", np.float32, 3), ("weight", np.float32),
                   ("extra", np.float32)])
assert VERTEX.itemsize == 56


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_path_depth.so")
    srcs = [os.path.join(ROOT, "tests", "oracle_path_depth.c")] + [os.path.join(ORACLE, f) for f in
                                                                   ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_shade_rays_depth.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.o_shade_rays_depth.restype = C.c_size_t
    return L


def _rays(origins, dirs):
    d = np.ascontiguousarray(dirs, np.float32)
    o = np.ascontiguousarray(origins, np.float32)
    assert d.ndim == 2 and d.shape[1] == 3
    if o.shape == (3,):
        return o, 0, d
    assert o.shape == d.shape
    return o, 3, d


def shade(L, scene, origins, dirs, depth, width=None, sample=0, log=False):
    """-> (rgba8[n,4], id_dist[n,2], rgb float32[n,3]) of the batch at sample `sample` and path depth `depth`, in VRT_MODE_FULL;
    with log=True also the vertex log (a VERTEX array, in the order the contributions were added). origins (n, 3) or (3,) shared"""
    assert 1 <= depth <= MAX_DEPTH
    o, stride, d = _rays(origins, dirs)
    n = d.shape[0]
    rgba = np.zeros((n, 4), np.uint8)
    idd = np.zeros((n, 2), np.int32)
    rgb = np.zeros((n, 3), np.float32)
    s = int(sample) & 0xFFFFFFFF
    s = s - (1 << 32) if s >= 1 << 31 else s   # the C int of the same bits
    if log:   # once to count the records, once to take them
        dummy = np.zeros(1, VERTEX)
        cap = L.o_shade_rays_depth(C.addressof(scene), n, o.ctypes.data, stride, d.ctypes.data, int(n if width is None else width),
                                   int(depth), s, None, None, None, dummy.ctypes.data, 0)
    vlog = np.zeros(max(cap, 1) if log else 1, VERTEX)
    got = L.o_shade_rays_depth(C.addressof(scene), n, o.ctypes.data, stride, d.ctypes.data, int(n if width is None else width), int(depth),
                               s, rgba.ctypes.data, idd.ctypes.data, rgb.ctypes.data, vlog.ctypes.data if log else None, cap if log else 0)
    if log:
        assert got == cap, "vertex log cut"
        return rgba, idd, rgb, vlog[:got]
    return rgba, idd, rgb


def mean(L, scene, origins, dirs, depth, width=None, first_sample=0, n_samples=1):
    """The exact mean of samples first_sample .. first_sample + n_samples - 1 (indices modulo 2^32): per channel the integer sum
    of the samples' bytes, resolved as (sum + n / 2) / n, alpha 255 -> (rgba8[n,4], id_dist[n,2] of the first sample)"""
    total = None
    idd0 = None
    for k in range(n_samples):
        rgba, idd, _ = shade(L, scene, origins, dirs, depth, width, (first_sample + k) & 0xFFFFFFFF)
        total = rgba.astype(np.uint64) if total is None else total + rgba
        idd0 = idd if idd0 is None else idd0
    out = ((total + n_samples // 2) // n_samples).astype(np.uint8)
    out[:, 3] = 255
    return out, idd0


def restate(vlog, n_rays, global_light):
    """float64[n_rays, 3]: the logged contributions summed by the rule's formulas (include/vrt.h), every factor a float32 the
    checker logged, every operation in float64"""
    PI = np.float64(np.float32(3.14159265359))
    sky = np.array([0.5, 0.7, 1.0], np.float64)
    sun = 3.0
    gl = np.asarray(global_light, np.float32)[:3].astype(np.float64)
    k = vlog["kind"]
    sc = vlog["sc"].astype(np.float64)
    tc = vlog["tc"].astype(np.float64)
    w = vlog["weight"].astype(np.float64)[:, None]
    ndotl = vlog["ndotl"].astype(np.float64)[:, None]
    lit = vlog["lit"].astype(np.float64)[:, None]
    extra = vlog["extra"].astype(np.float64)[:, None]
    term = np.zeros((len(vlog), 3), np.float64)
    term = np.where((k == SKY0)[:, None], gl * sky * tc * w, term)
    term = np.where((k == SKY)[:, None], tc * sky * sun * w / PI, term)
    term = np.where((k == GLASS)[:, None], tc * (sc * (gl * ndotl)) * w, term)
    term = np.where((k == EMIT0)[:, None], tc * sc * extra * w, term)
    term = np.where((k == EMIT)[:, None], tc * sc * extra * w / PI, term)
    term = np.where((k == DIRECT)[:, None], gl * lit * ndotl * sc * tc * w / PI, term)
    term = np.where((k == AMBIENT)[:, None], extra * sc * tc * w / PI, term)
    out = np.zeros((n_rays, 3), np.float64)
    np.add.at(out, vlog["ray"], term)
    return out
