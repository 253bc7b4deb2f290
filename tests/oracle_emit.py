"""pathTrace with a path depth, a sun disc and emitter sampling (tests/oracle_emit.c; include/vrt.h vrt_set_emitter_sampling) -- TEST
INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_emit.c with oracle/Makefile's flags together with the other three oracle sources into a shared library
in tmp_dir, the way oracle_sun.py builds its own. shade() traces a batch at one sample, one depth, one radius and one emitter list
(None or empty: sampling off) -> bytes, (voxel ID, dist), the unclamped float colour and, on request, the vertex log; mean() is the
exact mean of a sample range by the accumulation's resolve rule; restate() sums a log's contributions in float64 by the rule's
formulas, the connection's E * g among them; walk() is the emitter list of a record array by a Python walk of its own. The HDR
arithmetic is tests/oracle_hdr.c's, through oracle_hdr / oracle_rays_hdr on the floats shade() returns."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_path_depth as opd
import oracle_sun as osun

ROOT = opd.ROOT
ORACLE = opd.ORACLE
CFLAGS = opd.CFLAGS   # oracle/Makefile
MAX_DEPTH = opd.MAX_DEPTH

SKY0, SKY, GLASS, EMIT0, EMIT, DIRECT, AMBIENT = range(7)   # o_emit_vertex.kind, as oracle_path_depth's
VERTEX = np.dtype(osun.VERTEX.descr + [("u0", np.float32), ("uf", np.float32), ("ua", np.float32), ("ub", np.float32), ("j", np.int32),
                                       ("f", np.int32), ("q", np.float32, 3), ("cs", np.float32), ("cl", np.float32), ("r2", np.float32),
                                       ("conn_hit", np.int32), ("in_box", np.int32), ("conn_steps", np.int32), ("g", np.float32),
                                       ("E", np.float32, 3)])
assert VERTEX.itemsize == 108 + 76


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_emit.so")
    srcs = [os.path.join(ROOT, "tests", "oracle_emit.c")] + [os.path.join(ORACLE, f) for f in
                                                             ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_shade_rays_emit.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.o_shade_rays_emit.restype = C.c_size_t
    return L


def _list(emitters):
    e = np.zeros((0, 4), np.int32) if emitters is None else np.ascontiguousarray(emitters, np.int32).reshape(-1, 4)
    return e, (e.ctypes.data if len(e) else None)


def shade(L, scene, origins, dirs, depth, tan_radius, emitters, width=None, sample=0, log=False):
    """-> (rgba8[n,4], id_dist[n,2], rgb float32[n,3]) of the batch at sample `sample`, path depth `depth`, sun disc `tan_radius` and
    the emitter list `emitters` (int32[N, 4]; None or N == 0: sampling off), in VRT_MODE_FULL; with log=True also the vertex log (a
    VERTEX array, in the order the contributions were added). origins (n, 3) or (3,) shared"""
    assert 1 <= depth <= MAX_DEPTH and 0.0 <= tan_radius <= 1.0
    o, stride, d = opd._rays(origins, dirs)
    e, ep = _list(emitters)
    n = d.shape[0]
    rgba = np.zeros((n, 4), np.uint8)
    idd = np.zeros((n, 2), np.int32)
    rgb = np.zeros((n, 3), np.float32)
    s = int(sample) & 0xFFFFFFFF
    s = s - (1 << 32) if s >= 1 << 31 else s   # the C int of the same bits
    w = int(n if width is None else width)
    if log:   # once to count the records, once to take them
        dummy = np.zeros(1, VERTEX)
        cap = L.o_shade_rays_emit(C.addressof(scene), n, o.ctypes.data, stride, d.ctypes.data, w, int(depth), float(tan_radius), ep, len(e), s,
                                  None, None, None, dummy.ctypes.data, 0)
    vlog = np.zeros(max(cap, 1) if log else 1, VERTEX)
    got = L.o_shade_rays_emit(C.addressof(scene), n, o.ctypes.data, stride, d.ctypes.data, w, int(depth), float(tan_radius), ep, len(e), s,
                              rgba.ctypes.data, idd.ctypes.data, rgb.ctypes.data, vlog.ctypes.data if log else None, cap if log else 0)
    if log:
        assert got == cap, "vertex log cut"
        return rgba, idd, rgb, vlog[:got]
    return rgba, idd, rgb


def mean(L, scene, origins, dirs, depth, tan_radius, emitters, width=None, first_sample=0, n_samples=1):
    """The exact mean of samples first_sample .. first_sample + n_samples - 1 (indices modulo 2^32): per channel the integer sum
    of the samples' bytes, resolved as (sum + n / 2) / n, alpha 255 -> (rgba8[n,4], id_dist[n,2] of the first sample)"""
    total = None
    idd0 = None
    for k in range(n_samples):
        rgba, idd, _ = shade(L, scene, origins, dirs, depth, tan_radius, emitters, width, (first_sample + k) & 0xFFFFFFFF)
        total = rgba.astype(np.uint64) if total is None else total + rgba
        idd0 = idd if idd0 is None else idd0
    out = ((total + n_samples // 2) // n_samples).astype(np.uint8)
    out[:, 3] = 255
    return out, idd0


def restate(vlog, n_rays, global_light):
    """float64[n_rays, 3]: the logged contributions summed by the rule's formulas: oracle_path_depth's, and E * g of every DIRECT
    record (zero where the connection added nothing)"""
    out = opd.restate(vlog, n_rays, global_light)
    nee = vlog["E"].astype(np.float64) * vlog["g"].astype(np.float64)[:, None]
    np.add.at(out, vlog["ray"], nee)
    return out


def walk(records, world_min=(-1023, -1023, -1023), world_max=(1024, 1024, 1024)):
    """The emitter list of a record array (uint32[n, 2], csrc/vrt_layout.h) by a recursive Python walk: every leaf with alpha byte > 0
    and illumination byte > 0 as (lo.x, lo.y, lo.z, size) under the bounds split as the shader splits them (mid = min + (max - min)
    / 2; child bit 2 - k the upper half of axis k), sorted by (lo.x, lo.y, lo.z); a leaf whose box is no cube as its unit cells
    -> int32[N, 4]"""
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
                found.append((cmn[0], cmn[1], cmn[2], size[0]))
            else:
                found.extend((x, y, z, 1) for x in range(cmn[0], cmx[0]) for y in range(cmn[1], cmx[1]) for z in range(cmn[2], cmx[2]))

    if len(rec):
        visit(0, list(world_min), list(world_max))
    return np.array(sorted(found), np.int32).reshape(-1, 4)
