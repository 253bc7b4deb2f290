"""The guided filter's quality measurement (tests/test_filter_hdr.py) and the sweep that chose vrt_filter_default -- TEST
INFRASTRUCTURE ONLY, CPU only: everything here is the checkers' (oracle_hdr samples, oracle_guides planes, oracle_filter_hdr,
oracle_denoise_hdr), nothing is the product's but the world builders and the camera block.

Two 40 x 24 jittered frames of VRT_MODE_FULL: the reference's room from inside (guide_worlds.py) and the emitter-MIS lamp room
from inside (emit_mis_worlds.py). The input is the mean of 4 samples; the reference the mean of N_REF = 256 OTHER sample indices
-- never the filter's own output -- whose own noise variance is 4 / 256 = 1 / 64 of the input's. The metric is the mean over live
pixels of (x - ref)^2 / (ref^2 + 0.01).

    python tests/filter_quality.py            writes profiles/filter_quality.txt (the sweep over levels and sigmas, well under a minute)"""
import os
import sys

import numpy as np

W, H = 40, 24
FIRST, N_IN = 5, 4
REF_FIRST, N_REF = 1000, 256
MODE_FULL = 2
WORLDS = ("room", "lamp")


def _world(V, name):
    import emit_mis_worlds
    import guide_worlds
    if name == "room":
        return guide_worlds.world(V, "room"), guide_worlds.FRAMES["room"][0]
    return emit_mis_worlds.room(V), emit_mis_worlds.INSIDE_POSE


def mean_of(LF, scene, first, n):
    """the float mean of jittered samples first .. first + n - 1, as an HDR accumulation resolves it"""
    import oracle_hdr
    acc = oracle_hdr.Accum(LF, H, W)
    for k in range(first, first + n):
        acc.add(oracle_hdr.render(LF, scene, W, H, MODE_FULL, k, jitter=True))
    return acc.mean()


def inputs(V, O, LF, LG, name):
    """-> {"noisy": the 4-sample mean, "ref": the 256-sample mean, "guides": the 4 samples' planes, "id_dist": the corner frame's}"""
    import oracle_guides
    import oracle_hdr
    w, pose = _world(V, name)
    tex, dim = w.flatten()
    w.close()
    cam = V.camera_block(pose[:3], pose[3], pose[4], W, H)[:3]
    scene = O.make_scene(tex, dim, *cam)
    return {"noisy": mean_of(LF, scene, FIRST, N_IN), "ref": mean_of(LF, scene, REF_FIRST, N_REF),
            "guides": oracle_guides.planes(LG, scene, W, H, FIRST, N_IN, jitter=True)[0],
            "id_dist": oracle_hdr.render_bytes(LF, scene, W, H, MODE_FULL, FIRST)[1]}


def metric(x, ref, live):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float((((x - ref) ** 2) / (ref ** 2 + 0.01))[live].mean())


def errors(LF, d, f):
    """-> (unfiltered, ID-aware blur, guided filter with f): the metric of each against the reference"""
    import oracle_denoise_hdr
    import oracle_filter_hdr as F
    live = d["guides"]["coverage"] > 0
    return (metric(d["noisy"], d["ref"], live), metric(oracle_denoise_hdr.denoise(LF, d["noisy"], d["id_dist"])[0], d["ref"], live),
            metric(F.filter(LF, d["noisy"], d["guides"], f)[0], d["ref"], live))


def main():
    import tempfile
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    sys.path[:0] = [root, tests, os.path.join(root, "oracle")]
    import oracle_filter_hdr as F
    import oracle_guides
    import oracle_py as O
    import vrt_import
    O.build()
    V = vrt_import.vrt()
    tmp = tempfile.mkdtemp()
    LF, LG = F.build(tmp), oracle_guides.build(tmp)
    data = {n: inputs(V, O, LF, LG, n) for n in WORLDS}
    lines = ["# Guided filter (vrt_filter_hdr): error against a 256-sample reference, CPU checkers only (tests/filter_quality.py).",
             f"# {W} x {H} jittered frames of VRT_MODE_FULL, input = mean of samples {FIRST}..{FIRST + N_IN - 1}, reference = mean of samples",
             f"# {REF_FIRST}..{REF_FIRST + N_REF - 1}. Metric: mean over live pixels of (x - ref)^2 / (ref^2 + 0.01); lower is better.",
             "# 'blur' is the ID-aware blur (vrt_denoise_hdr) on the same input. ratio = filtered / unfiltered, summed over both worlds.",
             "#", "# world  unfiltered  blur"]
    base = {n: errors(LF, data[n], F.make(0))[:2] for n in WORLDS}
    for n in WORLDS:
        lines.append(f"# {n:5s}  {base[n][0]:.5f}  {base[n][1]:.5f}")
    lines += ["#", "# levels demod sigma_normal sigma_albedo sigma_depth   room     lamp     ratio"]
    rows = []
    for levels in (1, 2, 3, 4, 5):
        for demod in (False, True):
            for sn in (0.25, 0.5, 1.0):
                for sa in (0.05, 0.1, 0.25, 0.5):
                    for sd in (0.25, 0.5, 1.0, 2.0, 4.0):
                        f = F.make(levels, demod, sn, sa, sd)
                        e = [metric(F.filter(LF, data[n]["noisy"], data[n]["guides"], f)[0], data[n]["ref"], data[n]["guides"]["coverage"] > 0)
                             for n in WORLDS]
                        rows.append((sum(e) / sum(base[n][0] for n in WORLDS), levels, demod, sn, sa, sd, e))
    for ratio, levels, demod, sn, sa, sd, e in rows:
        lines.append(f"  {levels}      {int(demod)}     {sn:<12g} {sa:<12g} {sd:<12g} {e[0]:.5f}  {e[1]:.5f}  {ratio:.4f}")
    best = min(rows)
    lines.append(f"# best: levels {best[1]} demodulate {int(best[2])} sigma_normal {best[3]:g} sigma_albedo {best[4]:g} sigma_depth {best[5]:g}"
                 f" ratio {best[0]:.4f}")
    with open(os.path.join(root, "profiles", "filter_quality.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(lines[-1])


if __name__ == "__main__":
    main()
