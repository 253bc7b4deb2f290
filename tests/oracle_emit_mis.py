"""pathTrace with emitter sampling, either mode of vrt_set_emitter_importance and the balance heuristic of vrt_set_emitter_mis
(tests/oracle_emit_mis.c; include/vrt.h) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_emit_mis.c the way oracle_emit_power.py builds its own. shade() traces a batch at one sample, depth,
radius, emitter list, weights, mode and MIS flag (debug plants a misreading of the rule) -> bytes, (voxel ID, dist), the unclamped
float colour and, on request, the vertex log. density() and weights_of() restate the header's emit_mis_density and the two weights in
numpy float32, one rounding per operation; inv_power() restates the launch's 1 / Wtot. The checker computes its thresholds and its
inv_power from the weights itself."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_emit as oe
import oracle_emit_power as oep
import oracle_path_depth as opd

ROOT = oe.ROOT
UNIFORM, POWER = oep.UNIFORM, oep.POWER
SKY0, SKY, GLASS, EMIT0, EMIT, DIRECT, AMBIENT = range(7)
VERTEX = np.dtype(oep.VERTEX.descr + [("has_mis", np.int32), ("mx", np.float32, 3), ("mdir", np.float32, 3), ("mcs", np.float32),
                                      ("mpoint", np.float32, 3), ("maxis", np.int32), ("mcell", np.int32, 3), ("mrgb", np.int32),
                                      ("millum", np.int32), ("mm", np.int32), ("mw", np.int32), ("pl", np.float32),
                                      ("pb", np.float32), ("wt", np.float32)])
assert VERTEX.itemsize == oep.VERTEX.itemsize + 88
PI = np.float32(3.14159265359)


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_emit_mis.so")
    srcs = [os.path.join(ROOT, "tests", "oracle_emit_mis.c")] + [os.path.join(oe.ORACLE, f) for f in
                                                                 ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *oe.CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_shade_rays_emitm.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_size_t]
    L.o_shade_rays_emitm.restype = C.c_size_t
    return L


def shade(L, scene, origins, dirs, depth, tan_radius, emitters, weights, mode, mis, width=None, sample=0, log=False, debug=0):
    """-> (rgba8[n,4], id_dist[n,2], rgb float32[n,3]) of the batch at sample `sample`, path depth `depth`, sun disc `tan_radius`, the
    emitter list `emitters` (int32[N, 4]; None or N == 0: sampling off) with its weights (uint64[N]), the mode and the MIS flag; with
    log=True also the vertex log (a VERTEX array). origins (n, 3) or (3,) shared"""
    assert 1 <= depth <= oe.MAX_DEPTH and 0.0 <= tan_radius <= 1.0 and mode in (UNIFORM, POWER) and mis in (0, 1) and debug in (0, 1, 2)
    o, stride, d = opd._rays(origins, dirs)
    e, ep = oe._list(emitters)
    wt = np.zeros(0, np.uint64) if weights is None else np.ascontiguousarray(weights, np.uint64)
    assert len(wt) == len(e) or (mode == UNIFORM and len(wt) == 0)
    wp = wt.ctypes.data if len(wt) else None
    n = d.shape[0]
    rgba = np.zeros((n, 4), np.uint8)
    idd = np.zeros((n, 2), np.int32)
    rgb = np.zeros((n, 3), np.float32)
    s = int(sample) & 0xFFFFFFFF
    s = s - (1 << 32) if s >= 1 << 31 else s
    w = int(n if width is None else width)
    head = (C.addressof(scene), n, o.ctypes.data, stride, d.ctypes.data, w, int(depth), float(tan_radius), ep, wp, len(e), int(mode), int(mis),
            int(debug), s)
    if log:
        dummy = np.zeros(1, VERTEX)
        cap = L.o_shade_rays_emitm(*head, None, None, None, dummy.ctypes.data, 0)
    vlog = np.zeros(max(cap, 1) if log else 1, VERTEX)
    got = L.o_shade_rays_emitm(*head, rgba.ctypes.data, idd.ctypes.data, rgb.ctypes.data, vlog.ctypes.data if log else None, cap if log else 0)
    if log:
        assert got == cap, "vertex log cut"
        return rgba, idd, rgb, vlog[:got]
    return rgba, idd, rgb


def inv_power(wts):
    """inv_power of the header, "Per launch", of the integer weights -> float32"""
    total = sum(int(w) for w in wts)
    return np.float32(1.0 / float(total)) if total > 0 else np.float32(0.0)


def density(x, dirs, cs, point, axis, cell, w, inv_pow):
    """emit_mis_density of the header in numpy float32, every operation rounded on its own -> (pl, pb, m). x, dirs, point (n, 3)
    float32; cs (n,) float32; axis (n,) int, -1 for a hit without a normal (cl = 0); cell (n, 3) int; w (n,) int; inv_pow a float32
    or (n,) float32"""
    f = np.float32
    x, dirs, point = (np.asarray(a, f).reshape(-1, 3) for a in (x, dirs, point))
    cs = np.asarray(cs, f).reshape(-1)
    axis = np.asarray(axis, np.int64).reshape(-1)
    cellf = np.asarray(cell, np.int64).reshape(-1, 3).astype(f)
    wf = np.asarray(w, np.int64).reshape(-1).astype(f)
    ip = np.broadcast_to(np.asarray(inv_pow, f), cs.shape)
    v = point - x
    r2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    cl = np.where(axis >= 0, np.abs(dirs[np.arange(len(axis)), np.clip(axis, 0, 2)]), f(0.0)).astype(f)
    m = ((x < cellf) | (x > cellf + f(1.0))).sum(axis=1)
    ok = (m > 0) & (cl > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        pl = np.where(ok, ((wf * ip) * r2) / (m.astype(f) * cl), f(0.0)).astype(f)
    pb = (np.where(cs > 0, cs, f(0.0)).astype(f) / PI).astype(f)
    assert r2.dtype == f and pl.dtype == f and pb.dtype == f
    return pl, pb, m


def weights_of(pl, pb):
    """the balance heuristic's two weights of the header in float32 -> (wn, wb): wn = pl / (pl + pb), 0 where nothing is added; wb =
    pb / (pl + pb), 1 where !(pl > 0)"""
    f = np.float32
    pl, pb = np.asarray(pl, f), np.asarray(pb, f)
    pos = pl > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        s = pl + pb
        wn = np.where(pos, pl / s, f(0.0)).astype(f)
        wb = np.where(pos, pb / s, f(1.0)).astype(f)
    return wn, wb
