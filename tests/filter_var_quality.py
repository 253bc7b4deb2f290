"""The variance-guided filter's quality measurement (tests/test_filter_var.py) and the sweep that chose vrt_filter_var_default -- TEST
INFRASTRUCTURE ONLY, CPU only. Everything is tests/filter_quality.py's: the same two 40 x 24 worlds, the same 4-sample input, the
same 256-sample reference, the same metric; that file is imported, not edited.

Two variance sources per row: "spatial" is the filter's own estimate (no plane); "true" is the variance of the mean computed in numpy
from the four samples themselves -- Y (V1) of each sample's h(c), the unbiased sample variance over the four, divided by 4 -- passed
as the caller's plane. An optional third frame, the room at 80 x 48, shows what a larger frame does to the level count.

    python tests/filter_var_quality.py            writes profiles/filter_var_quality.txt (a few minutes)"""
import os
import sys

import numpy as np

import filter_quality as Q

SIGMA_LUM = (1.0, 2.0, 4.0, 8.0, 16.0, 1e6)
# the best row of profiles/filter_quality.txt per level count -- (sigma_normal, sigma_albedo, sigma_depth), demodulation on in all --
PARENT_BEST = {1: (0.5, 0.05, 2.0), 2: (0.5, 0.05, 0.5), 3: (0.25, 0.05, 0.25), 4: (0.25, 0.05, 0.25), 5: (0.25, 0.05, 0.25)}
# ... and the neighbours swept with them: the parent's defaults and each best row's neighbours in the parent's own grid
GUIDE_SIGMAS = ((1.0, 0.05, 2.0), (0.5, 0.05, 2.0), (0.5, 0.05, 0.5), (0.25, 0.05, 0.25), (0.5, 0.05, 1.0), (0.25, 0.05, 0.5),
                (0.5, 0.1, 0.5), (0.25, 0.1, 0.25), (1.0, 0.05, 0.5), (1.0, 0.1, 2.0))
SOURCES = ("spatial", "true")


def true_variance(V, O, LF, name, size=(Q.W, Q.H)):
    """the variance of the luminance of the 4-sample mean, from the four samples: float32[H,W]"""
    import oracle_filter_hdr as F
    import oracle_hdr
    w, pose = Q._world(V, name)
    tex, dim = w.flatten()
    w.close()
    scene = O.make_scene(tex, dim, *V.camera_block(pose[:3], pose[3], pose[4], size[0], size[1])[:3])
    y = []
    for k in range(Q.FIRST, Q.FIRST + Q.N_IN):
        c = F.h_of(oracle_hdr.render(LF, scene, size[0], size[1], Q.MODE_FULL, k, jitter=True)).astype(np.float64)
        y.append(0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2])
    return (np.var(np.stack(y), axis=0, ddof=1) / Q.N_IN).astype(np.float32)


def inputs(V, O, LF, LG, name):
    """filter_quality.inputs() and "variance": the true variance of the mean"""
    d = Q.inputs(V, O, LF, LG, name)
    d["variance"] = true_variance(V, O, LF, name)
    return d


def inputs_at(V, O, LF, LG, name, size):
    """the same at another frame size: filter_quality's constants are module globals its functions read"""
    old = (Q.W, Q.H)
    Q.W, Q.H = size
    try:
        d = Q.inputs(V, O, LF, LG, name)
        d["variance"] = true_variance(V, O, LF, name, size)
    finally:
        Q.W, Q.H = old
    return d


def error(LV, d, f, source):
    """the metric of the variance-guided filter with f on d, its variance from `source`"""
    import oracle_filter_var as FV
    out = FV.filter(LV, d["noisy"], d["guides"], f, d["variance"] if source == "true" else None)[0]
    return Q.metric(out, d["ref"], d["guides"]["coverage"] > 0)


def error_guide_only(LV, d, f):
    import oracle_filter_hdr as F
    return Q.metric(F.filter(LV, d["noisy"], d["guides"], f)[0], d["ref"], d["guides"]["coverage"] > 0)


def unfiltered(data):
    return sum(Q.metric(d["noisy"], d["ref"], d["guides"]["coverage"] > 0) for d in data.values())


def sweep(LV, data, levels=(1, 2, 3, 4, 5), sigmas=GUIDE_SIGMAS, sigma_lum=SIGMA_LUM, sources=SOURCES):
    """-> rows (ratio to the unfiltered error summed over data's worlds, levels, source, (sn, sa, sd), sigma_lum, per-world errors)"""
    import oracle_filter_var as FV
    base = unfiltered(data)
    rows = []
    for lv in levels:
        for src in sources:
            for sg in sigmas:
                for sl in sigma_lum:
                    e = [error(LV, d, FV.make(lv, True, *sg, sl), src) for d in data.values()]
                    rows.append((sum(e) / base, lv, src, sg, sl, e))
    return rows


def parent_best(LV, data, levels):
    """the guide-only filter at the parent's best row of that level count, the same ratio"""
    import oracle_filter_hdr as F
    return sum(error_guide_only(LV, d, F.make(levels, True, *PARENT_BEST[levels])) for d in data.values()) / unfiltered(data)


def best(rows, levels=None, source=None):
    return min(r for r in rows if (levels is None or r[1] == levels) and (source is None or r[2] == source))


def main():
    import tempfile
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    sys.path[:0] = [root, tests, os.path.join(root, "oracle")]
    import oracle_filter_var as FV
    import oracle_guides
    import oracle_py as O
    import vrt_import
    O.build()
    V = vrt_import.vrt()
    tmp = tempfile.mkdtemp()
    LV, LG = FV.build(tmp), oracle_guides.build(tmp)
    data = {n: inputs(V, O, LV, LG, n) for n in Q.WORLDS}
    lines = ["# Variance-guided filter (vrt_filter_hdr_var): error against a 256-sample reference, CPU checkers only",
             "# (tests/filter_var_quality.py). Frames, input, reference and metric are those of profiles/filter_quality.txt: 40 x 24, the mean",
             "# of 4 samples against the mean of 256 others, mean over live pixels of (x - ref)^2 / (ref^2 + 0.01); ratio = filtered /",
             "# unfiltered, summed over both worlds. source: spatial = the filter's own 7 x 7 estimate; true = var(Y) / 4 of the four",
             "# samples passed as the caller's plane. sigma_lum 1e+06 switches the luminance term off (the guide-only weights).",
             "# Demodulation on in every row.", "#",
             "# levels source  sigma_normal sigma_albedo sigma_depth sigma_lum   room     lamp     ratio"]
    rows = sweep(LV, data)
    for ratio, lv, src, sg, sl, e in rows:
        lines.append(f"  {lv}      {src:7s} {sg[0]:<12g} {sg[1]:<12g} {sg[2]:<11g} {sl:<10g}  {e[0]:.5f}  {e[1]:.5f}  {ratio:.4f}")
    lines += ["#", "# best row per level count: the parent's guide-only best row (recomputed here), then per source"]
    for lv in (1, 2, 3, 4, 5):
        t = f"# levels {lv}: guide-only {parent_best(LV, data, lv):.4f}"
        for src in SOURCES:
            b = best(rows, lv, src)
            t += f" | {src} {b[0]:.4f} at sigmas {b[3][0]:g} / {b[3][1]:g} / {b[3][2]:g} sigma_lum {b[4]:g}"
        lines.append(t)
    b = best(rows, source="spatial")
    lines.append(f"# best with the spatial estimate (vrt_filter_var_default): levels {b[1]} sigma_normal {b[3][0]:g} sigma_albedo {b[3][1]:g} "
                 f"sigma_depth {b[3][2]:g} sigma_lum {b[4]:g} ratio {b[0]:.4f}")
    b = best(rows, source="true")
    lines.append(f"# best with the true variance: levels {b[1]} sigma_normal {b[3][0]:g} sigma_albedo {b[3][1]:g} sigma_depth {b[3][2]:g} "
                 f"sigma_lum {b[4]:g} ratio {b[0]:.4f}")
    if "--no-large" not in sys.argv:
        big = {"room": inputs_at(V, O, LV, LG, "room", (80, 48))}
        lines += ["#", "# the room at 80 x 48 (one frame; ratio to its own unfiltered error), the best row per level count and source over the same grid"]
        rows = sweep(LV, big)
        for lv in (1, 2, 3, 4, 5):
            t = f"# 80x48 levels {lv}: guide-only {parent_best(LV, big, lv):.4f}"
            for src in SOURCES:
                b = best(rows, lv, src)
                t += f" | {src} {b[0]:.4f} at sigmas {b[3][0]:g} / {b[3][1]:g} / {b[3][2]:g} sigma_lum {b[4]:g}"
            lines.append(t)
    with open(os.path.join(root, "profiles", "filter_var_quality.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[-14:]))


if __name__ == "__main__":
    main()
