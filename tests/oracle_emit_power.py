"""pathTrace with emitter sampling in either mode of vrt_set_emitter_importance (tests/oracle_paths.c; include/vrt.h) -- TEST
INFRASTRUCTURE ONLY.

shade() is oracle_paths' without MIS: a batch at one sample, depth, radius, emitter list, weights and mode (0 uniform, 1 power; debug
plants a misreading of the rule) -> bytes, (voxel ID, dist), the unclamped float colour and, on request, the vertex log cut to this
rule's VERTEX. walk() is oracle_emit.walk() that also hands out each entry's record words; weights() and thresholds() restate the
header's integers in Python's big integers. The checker computes its thresholds from the weights itself."""
import numpy as np

import oracle_emit as oe
import oracle_paths as core

UNIFORM, POWER = core.UNIFORM, core.POWER
TICKS = 1 << 24
SKY0, SKY, GLASS, EMIT0, EMIT, DIRECT, AMBIENT = range(7)   # o_path_vertex.kind
VERTEX = core.prefix("x")
assert VERTEX.itemsize == oe.VERTEX.itemsize + 24
FLAWS = {0: core.FLAW_NONE, 1: core.FLAW_POWER_SIX_FACES, 2: core.FLAW_POWER_NO_P}   # debug: 1 puts 6 in m's place in g, 2 leaves p out
build = core.build
restate = oe.restate


def shade(L, scene, origins, dirs, depth, tan_radius, emitters, weights, mode, width=None, sample=0, log=False, debug=0):
    """oracle_paths.shade() of the depth, the radius, the list, its weights and the mode; the log as a VERTEX array"""
    return core.cut(core.shade(L, scene, origins, dirs, depth, tan_radius, emitters, weights, mode, width=width, sample=sample, log=log,
                               flaw=FLAWS[debug]), VERTEX)


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
    found = oe.leaves(records, world_min, world_max)
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
