"""The quality of the temporal chain with measured variances and the 3 x 3 search, and the sweep that chose vrt_temporal_mom_default
-- TEST INFRASTRUCTURE ONLY, CPU only. Worlds, metric, the 256-sample reference and the three camera paths are
tests/temporal_quality.py's (imported, not edited); one faster path is added, a yaw of 2 degrees a frame, where disocclusion at the
room's edges is common. Every frame's variance plane is the checker's M3 plane of that frame's own 4 samples
(tests/oracle_moments.c), what vrt_accum_resolve_hdr_temporal_mom hands the pass on an accumulation that keeps moments.

Rows: the last frame unfiltered; the parent's spatial-only row; the parent's chain (T1-T6) at vrt_temporal_default; the new chain over
measured_below in {1, 2, 4, 32769} x search in {0, 1} at the parent's default tap tests and at SVGF-like ones (normal_min 0.9,
depth_tol 0.05), where the parent's chain loses to the spatial filter; and the share of live pixels that drop their history per
frame on each path. The best row of a set of tap tests is the one with the least error summed over all four paths.

    python tests/temporal_mom_quality.py            writes profiles/temporal_mom_quality.txt (a few minutes)"""
import os
import sys

import numpy as np

import filter_quality as Q
import temporal_quality as TQ

FAST_YAW = 2.0
PATHS = TQ.PATHS + ("fast yaw",)
BELOW = (1, 2, 4, 32769)
TIGHT = dict(normal_min=0.9, depth_tol=0.05)


def pose_at(pose, path, k):
    if path == "fast yaw":
        return (pose[0], pose[1], pose[2], pose[3] - FAST_YAW * (TQ.FRAMES - 1 - k), pose[4])
    return TQ.pose_at(pose, path, k)


def frames_of(V, O, LM, LG, name, path):
    """-> [(cam, the 4-sample mean, its planes, its M3 plane)] per frame, and the reference at the last pose"""
    import oracle_guides
    import oracle_hdr
    import oracle_moments as OM
    w, pose = Q._world(V, name)
    tex, dim = w.flatten()
    w.close()
    out = []
    for k in range(TQ.FRAMES):
        p = pose_at(pose, path, k)
        cam = V.camera_block(p[:3], p[3], p[4], Q.W, Q.H)[:3]
        scene = O.make_scene(tex, dim, *cam)
        first = Q.FIRST + Q.N_IN * k
        acc = OM.Accum(LM, Q.H, Q.W)
        for s in range(first, first + Q.N_IN):
            acc.add(oracle_hdr.render(LM, scene, Q.W, Q.H, Q.MODE_FULL, s, jitter=True))
        out.append((cam, acc.mean(), oracle_guides.planes(LG, scene, Q.W, Q.H, first, Q.N_IN, jitter=True)[0], acc.variance()))
    return out, Q.mean_of(LM, scene, Q.REF_FIRST, Q.N_REF)


def chain_error(LT, frames, ref, f, below, search, **kw):
    """the new chain over `frames` -> (the metric of the filtered last frame, of the integrated one, the share of live pixels that
    dropped their history per frame after the first)"""
    import oracle_filter_var as FV
    import oracle_temporal_mom as M
    import temporal_worlds as TW
    hist, cam_prev, dropped, live_n = None, None, 0, 0
    for cam, mean, planes, mvar in frames:
        hist, integ, var = M.temporal(LT, cam, mean, planes, mvar, hist, M.make(TW.temporal_of(cam_prev, offset=(0.5, 0.5), **kw), below, search))
        live = planes["coverage"] > 0
        if cam_prev is not None:
            dropped += int((hist[0, ..., 3][live] < 2).sum())
            live_n += int(live.sum())
        cam_prev = cam
    return Q.metric(FV.filter(LT, integ, planes, f, var)[0], ref, live), Q.metric(integ, ref, live), dropped / live_n


def main():
    import tempfile
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    sys.path[:0] = [root, tests, os.path.join(root, "oracle")]
    import oracle_filter_var as FV
    import oracle_guides
    import oracle_moments as OM
    import oracle_py as O
    import oracle_temporal_mom as M
    import vrt_import
    O.build()
    V = vrt_import.vrt()
    tmp = tempfile.mkdtemp()
    LT, LG, LM = M.build(tmp), oracle_guides.build(tmp), OM.build(tmp)
    f = FV.make(**V.default_filter_var())
    base_kw = {k: v for k, v in V.default_temporal().items() if k not in ("offset_x", "offset_y")}
    data = {(path, name): frames_of(V, O, LM, LG, name, path) for path in PATHS for name in Q.WORLDS}
    lines = ["# Temporal chain with measured variances and the 3 x 3 search (vrt_accum_resolve_hdr_temporal_mom's rule: T1-T5, T3s, T7, T6m,",
             "# then vrt_filter_var_default with the pass's variance): error against a 256-sample reference at the last pose, CPU checkers only",
             "# (tests/temporal_mom_quality.py). Worlds, frame size, metric, reference and the first three paths: profiles/temporal_quality.txt's;",
             f"# fast yaw: {FAST_YAW} degrees a frame. Per world and path 8 frames of 4 jittered samples, each frame's variance plane the M3 plane of",
             "# its own 4 samples. ratio = error / the last frame's unfiltered error, summed over both worlds; total = the first three paths'",
             "# ratios added (the parent's total), total4 = all four. dropped = share of live pixels with N' < 2 per frame after the first.", "#"]
    un, spatial = {}, {}
    for path in PATHS:
        u = s = 0.0
        for name in Q.WORLDS:
            frames, ref = data[path, name]
            _, mean, planes, _ = frames[-1]
            live = planes["coverage"] > 0
            u += Q.metric(mean, ref, live)
            s += Q.metric(FV.filter(LT, mean, planes, f, None)[0], ref, live)
        un[path], spatial[path] = u, s / u
    head = "  " + " ".join(f"{p:>11s}" for p in PATHS)
    lines += ["# row" + " " * 60 + head + "    total   total4   (dropped:" + head + ")"]

    def row(label, r, d=None):
        t = f"  {label:62s}" + " ".join(f"{x:11.4f}" for x in r) + f"   {sum(r[:3]):.4f}   {sum(r):.4f}"
        if d is not None:
            t += "   (         " + " ".join(f"{x:11.3f}" for x in d) + ")"
        lines.append(t)

    row("unfiltered (4 samples)", [1.0] * len(PATHS))
    row("vrt_filter_var_default, spatial estimate (the parent's row)", [spatial[p] for p in PATHS])

    def run(below, search, **kw):
        r, d = [], []
        for path in PATHS:
            e = [chain_error(LT, *data[path, name], f, below, search, **kw) for name in Q.WORLDS]
            r.append(sum(x[0] for x in e) / un[path])
            d.append(float(np.mean([x[2] for x in e])))
        return r, d

    parent = []
    for path in PATHS:                                      # the parent's chain, by the parent's checker
        e = 0.0
        for name in Q.WORLDS:
            frames, ref = data[path, name]
            e += TQ.chain_error(LT, [(c, m, p) for c, m, p, _ in frames], ref, f, **base_kw)[0]
        parent.append(e / un[path])
    row("parent's chain (T1-T6) at vrt_temporal_default", parent)
    best = {}
    for label, tests_kw in (("vrt_temporal_default's tap tests", {}), ("normal_min 0.9, depth_tol 0.05", TIGHT)):
        lines.append(f"# the new chain at {label}:")
        rows = []
        for search in (0, 1):
            for below in BELOW:
                r, d = run(below, search, **dict(base_kw, **tests_kw))
                rows.append((sum(r), below, search, r))
                row(f"measured_below {below:<6d} search {search}", r, d)
        best[label] = min(rows, key=lambda x: (x[0], x[1], x[2]))
    lines.append("#")
    for label, b in best.items():
        lines.append(f"# best row at {label} (by total4, this sweep's four paths): measured_below {b[1]} search {b[2]} total {sum(b[3][:3]):.4f} total4 {b[0]:.4f}")
    b = best["vrt_temporal_default's tap tests"]
    lines.append(f"# against the parent's chain {sum(parent[:3]):.4f} / {sum(parent):.4f} ({' '.join('%.4f' % x for x in parent)}): "
                 + " ".join(f"{p} {x:.4f}" for p, x in zip(PATHS, b[3])))
    improved = b[0] < sum(parent)
    lines.append("# vrt_temporal_mom_default: " + (f"measured_below {b[1]}, search {b[2]} (that row)" if improved else
                                                   "measured_below 1, search 0, the identity values: no row improves on the parent's chain"))
    t = best["normal_min 0.9, depth_tol 0.05"]
    for i, path in enumerate(PATHS):
        lines.append(f"# tight tests, {path}: best row {t[3][i]:.4f} against spatial-only {spatial[path]:.4f}: the chain "
                     + ("wins" if t[3][i] < spatial[path] else "LOSES"))
    with open(os.path.join(root, "profiles", "temporal_mom_quality.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
