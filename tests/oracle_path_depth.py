"""pathTrace with a path depth (tests/oracle_paths.c; include/vrt.h vrt_set_path_depth) -- TEST INFRASTRUCTURE ONLY.

shade() and mean() are oracle_paths' at radius 0 and without a list: a batch at one sample and one depth -> bytes, (voxel ID, dist),
the unclamped float colour and, on request, the vertex log cut to this rule's VERTEX. restate() sums a log's contributions in float64
by the rule's formulas. The HDR arithmetic (float64 sums, mean, tone maps) is tests/oracle_hdr.c's, through oracle_hdr /
oracle_rays_hdr on the floats shade() returns."""
import numpy as np

import oracle_paths as core

MAX_DEPTH = core.MAX_DEPTH
SKY0, SKY, GLASS, EMIT0, EMIT, DIRECT, AMBIENT = range(7)   # o_path_vertex.kind
VERTEX = core.prefix("extra")
assert VERTEX.itemsize == 56
build = core.build


def shade(L, scene, origins, dirs, depth, width=None, sample=0, log=False):
    """oracle_paths.shade() of the depth alone; the log as a VERTEX array"""
    return core.cut(core.shade(L, scene, origins, dirs, depth, width=width, sample=sample, log=log), VERTEX)


def mean(L, scene, origins, dirs, depth, width=None, first_sample=0, n_samples=1):
    return core.mean(L, scene, origins, dirs, depth, width=width, first_sample=first_sample, n_samples=n_samples)


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
