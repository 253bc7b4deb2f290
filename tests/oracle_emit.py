"""pathTrace with a path depth, a sun disc and emitter sampling (tests/oracle_paths.c; include/vrt.h vrt_set_emitter_sampling) -- TEST
INFRASTRUCTURE ONLY.

shade() and mean() are oracle_paths' at the uniform mode: a batch at one sample, one depth, one radius and one emitter list (None or
empty: sampling off) -> bytes, (voxel ID, dist), the unclamped float colour and, on request, the vertex log cut to this rule's
VERTEX. restate() sums a log's contributions in float64 by the rule's formulas, the connection's E * g among them; walk() is the
emitter list of a record array by a Python walk of its own. The HDR arithmetic is tests/oracle_hdr.c's, through oracle_hdr /
oracle_rays_hdr on the floats shade() returns."""
import numpy as np

import oracle_path_depth as opd
import oracle_paths as core

MAX_DEPTH = core.MAX_DEPTH
SKY0, SKY, GLASS, EMIT0, EMIT, DIRECT, AMBIENT = range(7)   # o_path_vertex.kind
VERTEX = core.prefix("E")
assert VERTEX.itemsize == 108 + 76
build = core.build


def shade(L, scene, origins, dirs, depth, tan_radius, emitters, width=None, sample=0, log=False):
    """oracle_paths.shade() of the depth, the radius and the list, at VRT_EMIT_UNIFORM; the log as a VERTEX array"""
    return core.cut(core.shade(L, scene, origins, dirs, depth, tan_radius, emitters, width=width, sample=sample, log=log), VERTEX)


def mean(L, scene, origins, dirs, depth, tan_radius, emitters, width=None, first_sample=0, n_samples=1):
    return core.mean(L, scene, origins, dirs, depth, tan_radius, emitters, width=width, first_sample=first_sample, n_samples=n_samples)


def restate(vlog, n_rays, global_light):
    """float64[n_rays, 3]: the logged contributions summed by the rule's formulas: oracle_path_depth's, and E * g of every DIRECT
    record (zero where the connection added nothing)"""
    out = opd.restate(vlog, n_rays, global_light)
    nee = vlog["E"].astype(np.float64) * vlog["g"].astype(np.float64)[:, None]
    np.add.at(out, vlog["ray"], nee)
    return out


def leaves(records, world_min=(-1023, -1023, -1023), world_max=(1024, 1024, 1024)):
    """The emissive leaves of a record array (uint32[n, 2], csrc/vrt_layout.h) by a recursive Python walk: every leaf with alpha byte
    > 0 and illumination byte > 0 as (lo.x, lo.y, lo.z, size, word 0, word 1) under the bounds split as the shader splits them (mid
    = min + (max - min) / 2; child bit 2 - k the upper half of axis k), sorted by (lo.x, lo.y, lo.z); a leaf whose box is no cube as
    its unit cells, each with that leaf's words -> a list of tuples"""
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
    return found


def walk(records, world_min=(-1023, -1023, -1023), world_max=(1024, 1024, 1024)):
    """The emitter list of a record array: leaves() as (lo.x, lo.y, lo.z, size) -> int32[N, 4]"""
    return np.array([f[:4] for f in leaves(records, world_min, world_max)], np.int32).reshape(-1, 4)
