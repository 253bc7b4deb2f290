"""The one checker of the five path rules -- path depth, sun disc, emitter sampling, importance and MIS (tests/oracle_paths.c;
include/vrt.h) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_paths.c with oracle/Makefile's flags together with the other three oracle sources into one shared
library, once per process. shade() traces a batch at one sample, depth, radius, emitter list, weights, mode, MIS flag and planted flaw
-> bytes, (voxel ID, dist), the unclamped float colour and, on request, the vertex log; mean() is the exact mean of a sample range by
the accumulation's resolve rule. oracle_path_depth, oracle_sun, oracle_emit, oracle_emit_power and oracle_emit_mis each fix the
arguments their rule does not have and cut the log to their own VERTEX, a prefix of this one (prefix(), cut())."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
CFLAGS = ["-O3", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]   # oracle/Makefile
MAX_DEPTH = 8
UNIFORM, POWER = 0, 1
FLAW_NONE, FLAW_POWER_SIX_FACES, FLAW_POWER_NO_P, FLAW_MIS_BOUNCE_FULL, FLAW_MIS_BOUNCE_NONE = range(5)   # oracle_paths.c O_FLAW_*

SKY0, SKY, GLASS, EMIT0, EMIT, DIRECT, AMBIENT = range(7)   # o_path_vertex.kind
_F, _I = np.float32, np.int32
VERTEX = np.dtype([("ray", np.uint32), ("kind", _I), ("depth", _I), ("chain", _I), ("lit", _I), ("ndotl", _F), ("sc", _F, 3),
                   ("tc", _F, 3), ("weight", _F), ("extra", _F),                                                      # the loop
                   ("u1", _F), ("u2", _F), ("dx", _F), ("dy", _F), ("lp", _F, 3), ("rx", _F), ("ry", _F), ("normal", _F, 3),
                   ("shadow_steps", _I),                                                                              # sun disc
                   ("u0", _F), ("uf", _F), ("ua", _F), ("ub", _F), ("j", _I), ("f", _I), ("q", _F, 3), ("cs", _F), ("cl", _F),
                   ("r2", _F), ("conn_hit", _I), ("in_box", _I), ("conn_steps", _I), ("g", _F), ("E", _F, 3),         # sampling
                   ("t", _I), ("ticks", _I), ("m", _I), ("x", _F, 3),                                                 # importance
                   ("has_mis", _I), ("mx", _F, 3), ("mdir", _F, 3), ("mcs", _F), ("mpoint", _F, 3), ("maxis", _I), ("mcell", _I, 3),
                   ("mrgb", _I), ("millum", _I), ("mm", _I), ("mw", _I), ("pl", _F), ("pb", _F), ("wt", _F)])         # MIS
assert VERTEX.itemsize == 296
# the fields past a prefix that describe the loop itself and not a later rule: filled whether that rule is on or off
_LOOP_FIELDS = ("lp", "rx", "ry", "normal", "shadow_steps", "x")
_lib = None


def build(tmp_dir):
    global _lib
    if _lib is None:
        out = os.path.join(str(tmp_dir), "liboracle_paths.so")
        srcs = [os.path.join(ROOT, "tests", "oracle_paths.c")] + [os.path.join(ORACLE, f) for f in
                                                                  ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
        subprocess.run(["gcc", *CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
        L = C.CDLL(out)
        L.o_shade_rays_paths.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                         C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_size_t]
        L.o_shade_rays_paths.restype = C.c_size_t
        L.o_emit_thresholds.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.o_emit_thresholds.restype = None
        L.o_sun_disc_map.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.o_sun_disc_map.restype = None
        L.o_sun_basis.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
        L.o_sun_basis.restype = None
        for name in ("o_det_sinf", "o_det_cosf"):   # the probes of the conventions' sin / cos
            getattr(L, name).argtypes = [C.c_float]
            getattr(L, name).restype = C.c_float
        _lib = L
    return _lib


def prefix(last):
    """the record of the rules up to the one that added the field `last`: VERTEX's fields up to and including it"""
    return np.dtype(VERTEX.descr[:VERTEX.names.index(last) + 1])


def cut(result, vertex):
    """shade()'s result with its log, if it has one, restricted to the fields of `vertex` (a prefix()); what the rules past that prefix
    draw and compute must be zero in it"""
    if len(result) == 3:
        return result
    vlog = result[3]
    for name in VERTEX.names[len(vertex.names):]:
        assert name in _LOOP_FIELDS or not np.any(vlog[name]), f"{name}: a rule that is off left its mark in the log"
    out = np.zeros(len(vlog), vertex)
    for name in vertex.names:
        out[name] = vlog[name]
    return (*result[:3], out)


def _rays(origins, dirs):
    d = np.ascontiguousarray(dirs, np.float32)
    o = np.ascontiguousarray(origins, np.float32)
    assert d.ndim == 2 and d.shape[1] == 3
    if o.shape == (3,):
        return o, 0, d
    assert o.shape == d.shape
    return o, 3, d


def _list(emitters):
    e = np.zeros((0, 4), np.int32) if emitters is None else np.ascontiguousarray(emitters, np.int32).reshape(-1, 4)
    return e, (e.ctypes.data if len(e) else None)


def shade(L, scene, origins, dirs, depth=1, tan_radius=0.0, emitters=None, weights=None, mode=UNIFORM, mis=0, width=None, sample=0,
          log=False, flaw=FLAW_NONE):
    """-> (rgba8[n,4], id_dist[n,2], rgb float32[n,3]) of the batch at sample `sample`, path depth `depth`, sun disc `tan_radius`, the
    emitter list `emitters` (int32[N, 4]; None or N == 0: sampling off) with its weights (uint64[N]), the mode and the MIS flag, in
    VRT_MODE_FULL; with log=True also the vertex log (a VERTEX array, in the order the contributions were added). origins (n, 3) or
    (3,) shared"""
    assert 1 <= depth <= MAX_DEPTH and 0.0 <= tan_radius <= 1.0 and mode in (UNIFORM, POWER) and mis in (0, 1) and flaw in range(5)
    o, stride, d = _rays(origins, dirs)
    e, ep = _list(emitters)
    wt = np.zeros(0, np.uint64) if weights is None else np.ascontiguousarray(weights, np.uint64)
    assert len(wt) == len(e) or (mode == UNIFORM and len(wt) == 0)
    wp = wt.ctypes.data if len(wt) else None
    n = d.shape[0]
    rgba = np.zeros((n, 4), np.uint8)
    idd = np.zeros((n, 2), np.int32)
    rgb = np.zeros((n, 3), np.float32)
    s = int(sample) & 0xFFFFFFFF
    s = s - (1 << 32) if s >= 1 << 31 else s   # the C int of the same bits
    w = int(n if width is None else width)
    head = (C.addressof(scene), n, o.ctypes.data, stride, d.ctypes.data, w, int(depth), float(tan_radius), ep, wp, len(e), int(mode), int(mis),
            int(flaw), s)
    if log:   # once to count the records, once to take them
        dummy = np.zeros(1, VERTEX)
        cap = L.o_shade_rays_paths(*head, None, None, None, dummy.ctypes.data, 0)
    vlog = np.zeros(max(cap, 1) if log else 1, VERTEX)
    got = L.o_shade_rays_paths(*head, rgba.ctypes.data, idd.ctypes.data, rgb.ctypes.data, vlog.ctypes.data if log else None, cap if log else 0)
    if log:
        assert got == cap, "vertex log cut"
        return rgba, idd, rgb, vlog[:got]
    return rgba, idd, rgb


def mean(L, scene, origins, dirs, depth=1, tan_radius=0.0, emitters=None, width=None, first_sample=0, n_samples=1):
    """The exact mean of samples first_sample .. first_sample + n_samples - 1 (indices modulo 2^32): per channel the integer sum
    of the samples' bytes, resolved as (sum + n / 2) / n, alpha 255 -> (rgba8[n,4], id_dist[n,2] of the first sample)"""
    total = None
    idd0 = None
    for k in range(n_samples):
        rgba, idd, _ = shade(L, scene, origins, dirs, depth, tan_radius, emitters, width=width, sample=(first_sample + k) & 0xFFFFFFFF)
        total = rgba.astype(np.uint64) if total is None else total + rgba
        idd0 = idd if idd0 is None else idd0
    out = ((total + n_samples // 2) // n_samples).astype(np.uint8)
    out[:, 3] = 255
    return out, idd0
