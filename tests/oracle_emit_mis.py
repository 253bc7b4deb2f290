"""pathTrace with emitter sampling, either mode of vrt_set_emitter_importance and the balance heuristic of vrt_set_emitter_mis
(tests/oracle_paths.c; include/vrt.h) -- TEST INFRASTRUCTURE ONLY.

shade() is oracle_paths' with every rule: a batch at one sample, depth, radius, emitter list, weights, mode and MIS flag (debug plants
a misreading of the rule) -> bytes, (voxel ID, dist), the unclamped float colour and, on request, the vertex log, whose VERTEX is the
whole record. density() and weights_of() restate the header's emit_mis_density and the two weights in numpy float32, one rounding per
operation; inv_power() restates the launch's 1 / Wtot. The checker computes its thresholds and its inv_power from the weights itself."""
import numpy as np

import oracle_emit_power as oep
import oracle_paths as core

UNIFORM, POWER = core.UNIFORM, core.POWER
SKY0, SKY, GLASS, EMIT0, EMIT, DIRECT, AMBIENT = range(7)   # o_path_vertex.kind
VERTEX = core.prefix("wt")
assert VERTEX == core.VERTEX and VERTEX.itemsize == oep.VERTEX.itemsize + 88
PI = np.float32(3.14159265359)
FLAWS = {0: core.FLAW_NONE, 1: core.FLAW_MIS_BOUNCE_FULL, 2: core.FLAW_MIS_BOUNCE_NONE}   # debug: the bounce keeps weight 1, adds nothing
build = core.build


def shade(L, scene, origins, dirs, depth, tan_radius, emitters, weights, mode, mis, width=None, sample=0, log=False, debug=0):
    """oracle_paths.shade() of the depth, the radius, the list, its weights, the mode and the MIS flag; the log as a VERTEX array"""
    return core.cut(core.shade(L, scene, origins, dirs, depth, tan_radius, emitters, weights, mode, mis, width=width, sample=sample, log=log,
                               flaw=FLAWS[debug]), VERTEX)


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
