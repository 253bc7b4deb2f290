"""The inputs of tests/test_gpu_filter_seams.py and the condition under which a comparison at a tile seam means something -- TEST
INFRASTRUCTURE ONLY.

Two inputs per frame: tests/test_filter_hdr.py's random_case (NaN, Inf, dead pixels, negative depths) and smooth_case (one normal,
one albedo, a planar depth, every pixel live, random colours: every tap carries weight).

The sensitivity condition. At the widest lattice step s the tiles of a class meet every kLat * s pixels (128 in x, 32 in y with the
32 x 8 tile at step 4). The levels before it reach 2 * (1 + 2 + ... + s / 2) = 2 (s - 1) pixels, so a change of input column
seam - 2 (s - 1) - 1 (121) has not crossed the seam when the step-s level starts; that level's taps, 2 s pixels long, carry it to the
columns seam .. seam + 2 s - 1. Those taps are read from the halo the workgroup beyond the seam stages. If the checker's output there
does not depend on the column, a halo staged wrongly would compare equal; far_side_changes() counts the pixels where it does. The same
from the other side (column seam + 2 (s - 1), observed in seam - 2 s .. seam - 1) and in y."""
import numpy as np

import filter_geometry as FG
import oracle_filter_hdr as F
import oracle_filter_var as FV
from test_filter_hdr import random_case
from test_filter_var import random_variance

SENSITIVITY_LEVELS = 3          # steps 1, 2, 4
SWEPT = dict(sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=1.0)              # tests/test_gpu_filter_hdr.py's
SWEPT_VAR = dict(SWEPT, sigma_lum=2.0)                                          # tests/test_gpu_filter_var.py's
RANDOM_SHARE = 8                # random case: at least one eighth of the observed pixels change; smooth case: all of them


def smooth_case(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    g = {"normal": np.broadcast_to(np.array([0.6, 0.8, 0.0], np.float32), (h, w, 3)).copy(),
         "albedo": np.broadcast_to(np.array([0.5, 0.25, 0.75, 1.0], np.float32), (h, w, 4)).copy(),
         "depth": (40.0 + 0.5 * xx + 0.25 * yy).astype(np.float32), "coverage": np.ones((h, w), np.float32)}
    return (rng.random((h, w, 3)) * 4.0).astype(np.float32), g


def make(kind, w, h):
    """-> (rgb, guides, variance plane); the seed is the frame's longer side"""
    rng = np.random.default_rng(max(w, h))
    if kind == "random":
        rgb, g = random_case(rng, h, w, negative_depth=True)
        return rgb, g, random_variance(rng, h, w)
    rgb, g = smooth_case(rng, h, w)
    return rgb, g, (rng.random((h, w)) ** 2 * 4.0 + 0.01).astype(np.float32)


def probes(k, w, h):
    """the perturbations a frame has room for -> [(axis, perturbed line, first observed line, one past the last)]; axis 1 is x"""
    s = k["kLatticeMaxStep"]
    assert FG.lattice_steps(k)[-1] == s and SENSITIVITY_LEVELS == len(FG.lattice_steps(k))
    before = 2 * (s - 1)
    out = []
    for axis, n, tile in ((1, w, k["kLatX"]), (0, h, k["kLatY"])):
        seam = tile * s
        if n <= seam:
            continue
        out.append((axis, seam - before - 1, seam, min(seam + 2 * s, n)))        # across the seam into the halo of the tile beyond
        if seam + before < n:
            out.append((axis, seam + before, seam - 2 * s, seam))              # and back into the halo of the tile before
    return out


def far_side_changes(run, rgb, axis, line, lo, hi):
    """run(rgb, levels) -> the checker's float image. Doubles the colours of one input line and adds 1 -> (pixels of the observed
    lines lo .. hi - 1 whose output changes, pixels observed, the same count with the widest step left out: must be 0, only that
    step's taps carry the change across)"""
    moved = np.array(rgb, copy=True)
    sel = [slice(None)] * 3
    sel[axis] = line
    with np.errstate(invalid="ignore", over="ignore"):
        moved[tuple(sel)] = moved[tuple(sel)] * np.float32(2.0) + np.float32(1.0)
    obs = [slice(None)] * 2
    obs[axis] = slice(lo, hi)
    counts = []
    for levels in (SENSITIVITY_LEVELS, SENSITIVITY_LEVELS - 1):
        diff = (run(moved, levels).view(np.uint32) != run(rgb, levels).view(np.uint32)).any(axis=2)
        counts.append(int(diff[tuple(obs)].sum()))
    return counts[0], int(diff[tuple(obs)].size), counts[1]


def assert_sensitive(L, K, kind, w, h, rgb, g, var):
    """the condition above on the two checkers (L: oracle_filter_var.build()'s library, K: filter_geometry.constants())"""
    runs = {"guide-only": (lambda c, n: F.filter(L, c, g, F.make(n, True, **SWEPT))[0], True),
            "variance plane": (lambda c, n: FV.filter(L, c, g, FV.make(n, True, **SWEPT_VAR), var)[0], True),
            # the 7 x 7 estimate reads 3 pixels further than the levels: the change is across before step 4, and further with it
            "spatial variance": (lambda c, n: FV.filter(L, c, g, FV.make(n, True, **SWEPT_VAR), None)[0], False)}
    lines = probes(K, w, h)
    assert lines, f"{w} x {h}: no seam at step {K['kLatticeMaxStep']}"
    for axis, line, lo, hi in lines:
        for name, (run, only_last_step) in runs.items():
            changed, observed, without = far_side_changes(run, rgb, axis, line, lo, hi)
            what = f"{w} x {h} {kind} {name}: {'column' if axis else 'row'} {line} -> {lo}..{hi - 1}: {changed} of {observed}, {without} without the last step"
            assert observed > 0, what
            if kind == "smooth":
                assert changed == observed, what
            else:
                assert changed * RANDOM_SHARE >= observed, what
            assert without == 0 or not only_last_step, what
