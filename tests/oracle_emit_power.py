"""pathTrace with emitter sampling in either mode of vrt_set_emitter_importance (tests/oracle_emit_power.c; include/vrt.h) -- TEST
INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_emit_power.c the way oracle_emit.py builds its own. shade() traces a batch at one sample, depth, radius,
emitter list, weights and mode (0 uniform, 1 power; debug plants a misreading of the rule) -> bytes, (voxel ID, dist), the unclamped
float colour and, on request, the vertex log. walk() is oracle_emit.walk() that also hands out each entry's record words; weights()
and thresholds() restate the header's integers in Python's big integers. The checker computes its thresholds from the weights
itself."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_emit as oe
import oracle_path_depth as opd

ROOT = oe.ROOT
UNIFORM, POWER = 0, 1
TICKS = 1 << 24
SKY0, SKY, GLASS, EMIT0, EMIT, DIRECT, AMBIENT = range(7)
VERTEX = np.dtype(oe.VERTEX.descr + [("t", np.int32), ("ticks", np.int32), ("m", np.int32), ("x", np.float32, 3)])
assert VERTEX.itemsize == oe.VERTEX.itemsize + 24


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_emit_power.so")
    srcs = [os.path.join(ROOT, "tests", "oracle_emit_power.c")] + [os.path.join(oe.ORACLE, f) for f in
                                                                   ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *oe.CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_shade_rays_emitp.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.o_shade_rays_emitp.restype = C.c_size_t
    L.o_emit_thresholds.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.o_emit_thresholds.restype = None
    return L


def shade(L, scene, origins, dirs, depth, tan_radius, emitters, weights, mode, width=None, sample=0, log=False, debug=0):
    """-> (rgba8[n,4], id_dist[n,2], rgb float32[n,3]) of the batch at sample `sample`, path depth `depth`, sun disc `tan_radius`, the
    emitter list `emitters` (int32[N, 4]; None or N == 0: sampling off) with its weights (uint64[N]) and the mode; with log=True also
    the vertex log (a VERTEX array). origins (n, 3) or (3,) shared"""
    assert 1 <= depth <= oe.MAX_DEPTH and 0.0 <= tan_radius <= 1.0 and mode in (UNIFORM, POWER) and debug in (0, 1, 2)
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
    head = (C.addressof(scene), n, o.ctypes.data, stride, d.ctypes.data, w, int(depth), float(tan_radius), ep, wp, len(e), int(mode), int(debug), s)
    if log:
        dummy = np.zeros(1, VERTEX)
        cap = L.o_shade_rays_emitp(*head, None, None, None, dummy.ctypes.data, 0)
    vlog = np.zeros(max(cap, 1) if log else 1, VERTEX)
    got = L.o_shade_rays_emitp(*head, rgba.ctypes.data, idd.ctypes.data, rgb.ctypes.data, vlog.ctypes.data if log else None, cap if log else 0)
    if log:
        assert got == cap, "vertex log cut"
        return rgba, idd, rgb, vlog[:got]
    return rgba, idd, rgb


def checker_thresholds(L, weights):
    """the checker's own table of the weights -> uint32[N]"""
    wt = np.ascontiguousarray(weights, np.uint64)
    out = np.zeros(len(wt), np.uint32)
    if len(wt):
        L.o_emit_thresholds(wt.ctypes.data, len(wt), out.ctypes.data)
    return out


def walk(records, world_min=(-1023, -1023, -1023), world_max=(1024, 1024, 1024)):
    """oracle_emit.walk() with the record words of every entry -> (int32[N, 4], uint32[N, 2]); a unit cell of a leaf whose box is
    no cube takes that leaf's words"""
    rec = np.asarray(records, np.uint32).reshape(-1, 2)
    found = []

    def visit(i, mn, mx):
        w0, first = int(rec[i, 0]), int(rec[i, 1])
        slot = 0
        for ci in range(8):
            if not (w0 >> ci) & 1:
                continue
            idx = first + slot
            slot += 1
            cmn, cmx = list(mn), list(mx)
            for k in range(3):
                mid = mn[k] + ((mx[k] - mn[k]) >> 1)
                if (ci >> (2 - k)) & 1:
                    cmn[k] = mid
                else:
                    cmx[k] = mid
            if not (w0 >> (8 + ci)) & 1:
                visit(idx, cmn, cmx)
                continue
            l0, l1 = int(rec[idx, 0]), int(rec[idx, 1])
            if (l0 >> 24) == 0 or ((l1 >> 8) & 0xFF) == 0:
                continue
            size = [cmx[k] - cmn[k] for k in range(3)]
            if min(size) <= 0:
                continue
            if size[0] == size[1] == size[2]:
                found.append((cmn[0], cmn[1], cmn[2], size[0], l0, l1))
            else:
                found.extend((x, y, z, 1, l0, l1) for x in range(cmn[0], cmx[0]) for y in range(cmn[1], cmx[1]) for z in range(cmn[2], cmx[2]))

    if len(rec):
        visit(0, list(world_min), list(world_max))
    found.sort(key=lambda f: f[:3])
    lst = np.array([f[:4] for f in found], np.int64).astype(np.int32).reshape(-1, 4)
    words = np.array([f[4:] for f in found], np.uint64).astype(np.uint32).reshape(-1, 2)
    return lst, words


def weights(lst, words):
    """W_j = size^2 * illum * (R + G + B) in Python integers -> a list of int"""
    out = []
    for (_, _, _, size), (w0, w1) in zip(np.asarray(lst).tolist(), np.asarray(words).tolist()):
        out.append(size * size * ((w1 >> 8) & 0xFF) * ((w0 & 0xFF) + ((w0 >> 8) & 0xFF) + ((w0 >> 16) & 0xFF)))
    return out


def thresholds(wts):
    """T_j of the header in Python integers -> a list of int"""
    n = len(wts)
    total = sum(wts)
    out, c = [], 0
    for j, w in enumerate(wts):
        c += w
        out.append((j + 1) + c * (TICKS - n) // total if total > 0 else (j + 1) * TICKS // n)
    return out


def restate(vlog, n_rays, global_light):
    return oe.restate(vlog, n_rays, global_light)
