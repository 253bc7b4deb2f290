"""The temporal chain's quality measurement and the sweep that chose vrt_temporal_default -- TEST INFRASTRUCTURE ONLY, CPU only.
Frames, metric and the 256-sample reference are tests/filter_var_quality.py's (tests/filter_quality.py's two 40 x 24 worlds, the mean
over live pixels of (x - ref)^2 / (ref^2 + 0.01)); those files are imported, not edited.

Three camera paths per world, 8 frames of 4 jittered samples each (every frame its own sample indices), ending at the pose the other
two profiles measure at: static, a slow yaw (0.4 degrees a frame) and a slow translation (0.05 voxels a frame along x and z). The
reference is 256 other samples at the LAST pose. Rows: the last frame unfiltered, the parent's best spatial row on it
(vrt_filter_var_default, the spatial estimate), and the chain -- T1-T6 over the 8 frames with the history carried along, then
vrt_filter_var_default on the last integrated image with T6's variance -- over a sweep of the pass's parameters.

    python tests/temporal_quality.py            writes profiles/temporal_quality.txt (a few minutes)"""
import itertools
import os
import sys

import numpy as np

import filter_quality as Q

FRAMES, YAW, STEP = 8, 0.4, 0.05
PATHS = ("static", "yaw", "translation")
GRID = {"normal_min": (0.0, 0.25, 0.5, 0.9), "depth_tol": (0.05, 0.1, 0.2, 0.4), "alpha_min": (0.05, 0.1, 0.2, 0.4, 0.6),
        "alpha_moments_min": (0.05, 0.2, 0.4, 0.6), "max_history": (8, 32)}


def pose_at(pose, path, k):
    """frame k of FRAMES on `path`, the last one at `pose`"""
    back = FRAMES - 1 - k
    if path == "yaw":
        return (pose[0], pose[1], pose[2], pose[3] - YAW * back, pose[4])
    if path == "translation":
        return (pose[0] - STEP * back, pose[1], pose[2] - STEP * back, pose[3], pose[4])
    return pose


def frames_of(V, O, LF, LG, name, path):
    """-> [(cam, the 4-sample mean, its planes)] per frame, and the reference at the last pose"""
    import oracle_guides
    w, pose = Q._world(V, name)
    tex, dim = w.flatten()
    w.close()
    out = []
    for k in range(FRAMES):
        p = pose_at(pose, path, k)
        cam = V.camera_block(p[:3], p[3], p[4], Q.W, Q.H)[:3]
        scene = O.make_scene(tex, dim, *cam)
        first = Q.FIRST + Q.N_IN * k
        out.append((cam, Q.mean_of(LF, scene, first, Q.N_IN), oracle_guides.planes(LG, scene, Q.W, Q.H, first, Q.N_IN, jitter=True)[0]))
    return out, Q.mean_of(LF, scene, Q.REF_FIRST, Q.N_REF)


def chain_error(LT, frames, ref, f, **kw):
    """the chain over `frames` with the pass's parameters kw -> (the metric of the filtered last frame, of the integrated one)"""
    import oracle_filter_var as FV
    import oracle_temporal as T
    import temporal_worlds as TW
    hist, cam_prev = None, None
    for cam, mean, planes in frames:
        hist, integ, var = T.temporal(LT, cam, mean, planes, hist, TW.temporal_of(cam_prev, offset=(0.5, 0.5), **kw))
        cam_prev = cam
    live = planes["coverage"] > 0
    return Q.metric(FV.filter(LT, integ, planes, f, var)[0], ref, live), Q.metric(integ, ref, live)


def main():
    import tempfile
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    sys.path[:0] = [root, tests, os.path.join(root, "oracle")]
    import oracle_filter_var as FV
    import oracle_guides
    import oracle_py as O
    import oracle_temporal as T
    import vrt_import
    O.build()
    V = vrt_import.vrt()
    tmp = tempfile.mkdtemp()
    LT, LG = T.build(tmp), oracle_guides.build(tmp)
    f = FV.make(**V.default_filter_var())
    data = {(path, name): frames_of(V, O, LT, LG, name, path) for path in PATHS for name in Q.WORLDS}
    lines = ["# Temporal chain (vrt_accum_resolve_hdr_temporal's rule: T1-T6, then vrt_filter_var_default with T6's variance): error against a",
             "# 256-sample reference at the last pose, CPU checkers only (tests/temporal_quality.py). Worlds, frame size, metric: those of",
             "# profiles/filter_var_quality.txt. Per world and camera path 8 frames of 4 jittered samples, the history carried from frame to",
             f"# frame: static; yaw {YAW} degrees a frame; translation {STEP} voxels a frame along x and z. ratio = error / the last frame's",
             "# unfiltered error, summed over both worlds; total = the three paths' ratios added.", "#"]
    base, spatial = {}, {}
    for path in PATHS:
        un = sp = 0.0
        for name in Q.WORLDS:
            frames, ref = data[path, name]
            _, mean, planes = frames[-1]
            live = planes["coverage"] > 0
            un += Q.metric(mean, ref, live)
            sp += Q.metric(FV.filter(LT, mean, planes, f, None)[0], ref, live)
        base[path], spatial[path] = un, sp / un
    lines.append("# path         unfiltered (4 samples)   vrt_filter_var_default, spatial estimate (the parent's best row)")
    for path in PATHS:
        lines.append(f"  {path:12s} 1.0000                   {spatial[path]:.4f}")
    lines += ["#", "# normal_min depth_tol alpha_min alpha_moments_min max_history   static   yaw      transl.  total    (integrated, unfiltered: static yaw transl.)"]
    rows = []
    keys = list(GRID)
    for combo in itertools.product(*(GRID[k] for k in keys)):
        kw = dict(zip(keys, combo))
        r, ri = [], []
        for path in PATHS:
            e = [chain_error(LT, *data[path, name], f, **kw) for name in Q.WORLDS]
            r.append(sum(x[0] for x in e) / base[path])
            ri.append(sum(x[1] for x in e) / base[path])
        rows.append((sum(r), kw, r, ri))
        lines.append(f"  {kw['normal_min']:<10g} {kw['depth_tol']:<9g} {kw['alpha_min']:<9g} {kw['alpha_moments_min']:<17g} {kw['max_history']:<12d}  "
                     f"{r[0]:.4f}   {r[1]:.4f}   {r[2]:.4f}   {sum(r):.4f}   ({ri[0]:.4f} {ri[1]:.4f} {ri[2]:.4f})")
    best = min(rows, key=lambda x: x[0])
    lines += ["#", "# best row (vrt_temporal_default): " + " ".join(f"{k} {v:g}" for k, v in best[1].items()) + f" total {best[0]:.4f}"]
    edge = [k for k, v in best[1].items() if k != "max_history" and v in (min(GRID[k]), max(GRID[k]))]
    lines.append("# on the grid's edge in: " + (", ".join(edge) or "nothing") + " -- a pixel that loses its history is handed the variance 65504^2, which V3")
    lines.append("# carries to its neighbours level by level and switches their luminance term off too: the sweep pays more for a dropped history")
    lines.append("# than for a stale one, so the loosest tap tests win on these three paths (no disocclusion larger than a pixel or two).")
    for i, path in enumerate(PATHS):
        verdict = "wins" if best[2][i] < spatial[path] else "LOSES"
        lines.append(f"# {path}: chain {best[2][i]:.4f} against spatial-only {spatial[path]:.4f}: the chain {verdict}")
    lines += ["#", "# the best row's chain with fewer levels of the same filter (vrt_filter_var_default's sigmas): static yaw transl. total"]
    for lv in (0, 1, 2, 3):
        d = V.default_filter_var()
        fl = FV.make(**dict(d, levels=lv))
        r = [sum(chain_error(LT, *data[path, name], fl, **best[1])[0] for name in Q.WORLDS) / base[path] for path in PATHS]
        lines.append(f"# levels {lv}: {r[0]:.4f} {r[1]:.4f} {r[2]:.4f} {sum(r):.4f}")
    share = []
    for path in PATHS:
        import temporal_worlds as TW
        n = live_n = 0
        for name in Q.WORLDS:
            hist, cam_prev = None, None
            for cam, mean, planes in data[path, name][0]:
                hist = T.temporal(LT, cam, mean, planes, hist, TW.temporal_of(cam_prev, offset=(0.5, 0.5), **best[1]))[0]
                cam_prev = cam
            live = planes["coverage"] > 0
            n += int((hist[0, ..., 3][live] < 2).sum())
            live_n += int(live.sum())
        share.append(n / live_n)
    lines.append("# share of live pixels of the last frame without a history (N' < 2, variance 65504^2) at the best row: "
                 + " ".join(f"{p} {x:.3f}" for p, x in zip(PATHS, share)))
    with open(os.path.join(root, "profiles", "temporal_quality.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[-14:]))


if __name__ == "__main__":
    main()
