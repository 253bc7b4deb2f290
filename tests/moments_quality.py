"""What the measured variance of an accumulation that keeps moments (vrt_accum_keep_moments, M1-M3) buys the variance-guided filter
-- TEST INFRASTRUCTURE ONLY, CPU only. Everything is tests/filter_quality.py's and tests/filter_var_quality.py's: the same two 40 x 24
worlds, the same 4-sample input, the same 256-sample reference, the same metric, the same grid of filters; those files are imported,
not edited.

Three variance sources per row: "moments" is the checker's M3 plane of the four input samples (tests/oracle_moments.c), what
vrt_accum_resolve_hdr_filtered_var hands the filter on such an accumulation; "spatial" the filter's own estimate (no plane); "true"
numpy's float64 variance of the mean from the same four samples (filter_var_quality.true_variance).

    python tests/moments_quality.py            writes profiles/moments_quality.txt (a few minutes): the best rows; --rows: all 900 too"""
import os
import sys

import numpy as np

import filter_quality as Q
import filter_var_quality as QV

SOURCES = ("moments", "spatial", "true")


def moments_variance(V, O, LM, name):
    """M3's plane of the 4-sample input: float32[H,W]"""
    import oracle_hdr
    import oracle_moments as OM
    w, pose = Q._world(V, name)
    tex, dim = w.flatten()
    w.close()
    scene = O.make_scene(tex, dim, *V.camera_block(pose[:3], pose[3], pose[4], Q.W, Q.H)[:3])
    acc = OM.Accum(LM, Q.H, Q.W)
    for k in range(Q.FIRST, Q.FIRST + Q.N_IN):
        acc.add(oracle_hdr.render(LM, scene, Q.W, Q.H, Q.MODE_FULL, k, jitter=True))
    return acc.variance(), acc.mean()


def sweep(LV, data):
    """filter_var_quality.sweep() over the three sources -> its rows, the source named"""
    rows = QV.sweep(LV, data, sources=("spatial", "true"))
    as_plane = {n: dict(d, variance=d["moments"]) for n, d in data.items()}
    rows += [(r[0], r[1], "moments") + r[3:] for r in QV.sweep(LV, as_plane, sources=("true",))]
    return rows


def main():
    import tempfile
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    sys.path[:0] = [root, tests, os.path.join(root, "oracle")]
    import oracle_filter_var as FV
    import oracle_guides
    import oracle_moments as OM
    import oracle_py as O
    import vrt_import
    O.build()
    V = vrt_import.vrt()
    tmp = tempfile.mkdtemp()
    LV, LG, LM = FV.build(tmp), oracle_guides.build(tmp), OM.build(tmp)
    data = {n: QV.inputs(V, O, LV, LG, n) for n in Q.WORLDS}
    lines = ["# Variance-guided filter fed the measured variance of an accumulation that keeps moments (vrt_accum_keep_moments, M3's plane):",
             "# error against a 256-sample reference, CPU checkers only (tests/moments_quality.py). Frames, input, reference, metric and grid are",
             "# those of profiles/filter_var_quality.txt: 40 x 24, the mean of 4 samples against the mean of 256 others, mean over live pixels of",
             "# (x - ref)^2 / (ref^2 + 0.01); ratio = filtered / unfiltered, summed over both worlds. source: moments = M3's plane of the four",
             "# samples (float64 sums of the float32 y and y * y, the mean squared in float32); spatial = the filter's own 7 x 7 estimate; true =",
             "# numpy's float64 var(Y) / 4 of the same four samples. Demodulation on in every row.", "#"]
    for n in Q.WORLDS:
        data[n]["moments"], mean = moments_variance(V, O, LM, n)
        assert np.array_equal(mean.view(np.uint32), data[n]["noisy"].view(np.uint32))     # the same four samples
        m, t = data[n]["moments"].astype(np.float64), data[n]["variance"].astype(np.float64)
        zero_m, zero_t = int((m == 0).sum()), int((t == 0).sum())
        both = (m > 0) & (t > 0)
        rel = np.abs(m[both] - t[both]) / t[both]
        lines.append(f"# {n}: M3 against numpy on {Q.W * Q.H} pixels: exactly 0 in {zero_m} (numpy: {zero_t}); where both are > 0 ({int(both.sum())} pixels) "
                     f"relative difference max {rel.max():.3g}, median {np.median(rel):.3g}; largest absolute difference {np.abs(m - t).max():.3g}"
                     f" at a variance of {t.flat[np.abs(m - t).argmax()]:.3g}")
    rows = sweep(LV, data)
    if "--rows" in sys.argv:
        lines += ["#", "# levels source  sigma_normal sigma_albedo sigma_depth sigma_lum   room     lamp     ratio"]
        for ratio, lv, src, sg, sl, e in rows:
            lines.append(f"  {lv}      {src:7s} {sg[0]:<12g} {sg[1]:<12g} {sg[2]:<11g} {sl:<10g}  {e[0]:.5f}  {e[1]:.5f}  {ratio:.4f}")
    else:
        lines += ["#", f"# The {len(rows)} rows of the sweep (5 level counts x 3 sources x 10 guide-sigma triples x 6 sigma_lum) are not listed: --rows writes them."]
    lines += ["# best row per level count and source"]
    for lv in (1, 2, 3, 4, 5):
        t = f"# levels {lv}:"
        for src in SOURCES:
            b = QV.best(rows, lv, src)
            t += f" | {src} {b[0]:.4f} at sigmas {b[3][0]:g} / {b[3][1]:g} / {b[3][2]:g} sigma_lum {b[4]:g}"
        lines.append(t)
    for src in SOURCES:
        b = QV.best(rows, source=src)
        lines.append(f"# best with source {src}: levels {b[1]} sigma_normal {b[3][0]:g} sigma_albedo {b[3][1]:g} sigma_depth {b[3][2]:g} "
                     f"sigma_lum {b[4]:g} ratio {b[0]:.4f}")
    gap = max(abs(QV.best(rows, lv, "moments")[0] - QV.best(rows, lv, "true")[0]) for lv in (1, 2, 3, 4, 5))
    worst = max(abs(a[0] - b[0]) for a in rows if a[2] == "moments" for b in rows if b[2] == "true" and b[1] == a[1] and b[3:5] == a[3:5])
    lines.append(f"# largest gap between the moments and the true column: {gap:.2g} over the best rows, {worst:.2g} over all {len(rows) // 3} rows")
    with open(os.path.join(root, "profiles", "moments_quality.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[-11:]))


if __name__ == "__main__":
    main()
