"""pathTrace with a path depth and a sun disc (tests/oracle_paths.c; include/vrt.h vrt_set_sun_disc) -- TEST INFRASTRUCTURE ONLY.

shade() and mean() are oracle_paths' without a list: a batch at one sample, one depth and one radius -> bytes, (voxel ID, dist), the
unclamped float colour and, on request, the vertex log cut to this rule's VERTEX. basis() is the disc's basis as the checker makes
it; restate() sums a log's contributions in float64 by the rule's formulas (the DIRECT term with the logged lit and ndotl', which
the sun disc changes and nothing else). The HDR arithmetic (float64 sums, mean, tone maps) is tests/oracle_hdr.c's, through
oracle_hdr / oracle_rays_hdr on the floats shade() returns."""
import numpy as np

import oracle_path_depth as opd
import oracle_paths as core

MAX_DEPTH = core.MAX_DEPTH
SKY0, SKY, GLASS, EMIT0, EMIT, DIRECT, AMBIENT = range(7)   # o_path_vertex.kind
VERTEX = core.prefix("shadow_steps")
assert VERTEX.itemsize == 56 + 52
build = core.build


def basis(L, light_dir, tan_radius):
    """-> (tan_radius, ll, Ln[3], T[3], B[3]) as the checker makes them (float32)"""
    ld = np.ascontiguousarray(light_dir, np.float32)
    out = np.zeros(11, np.float32)
    L.o_sun_basis(ld.ctypes.data, float(tan_radius), out.ctypes.data)
    return out[0], out[1], out[2:5].copy(), out[5:8].copy(), out[8:11].copy()


def shade(L, scene, origins, dirs, depth, tan_radius, width=None, sample=0, log=False):
    """oracle_paths.shade() of the depth and the radius; the log as a VERTEX array"""
    return core.cut(core.shade(L, scene, origins, dirs, depth, tan_radius, width=width, sample=sample, log=log), VERTEX)


def mean(L, scene, origins, dirs, depth, tan_radius, width=None, first_sample=0, n_samples=1):
    return core.mean(L, scene, origins, dirs, depth, tan_radius, width=width, first_sample=first_sample, n_samples=n_samples)


def restate(vlog, n_rays, global_light):
    """float64[n_rays, 3]: the logged contributions summed by the rule's formulas; the record's first fields are
    oracle_path_depth's, and a DIRECT record's lit and ndotl are the sun disc's lit and ndotl'"""
    return opd.restate(vlog, n_rays, global_light)
