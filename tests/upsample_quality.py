"""Guided upsampling's quality measurement and the sweep that chose vrt_upsample_default -- TEST INFRASTRUCTURE ONLY, CPU only:
everything here is the checkers' (oracle_hdr samples, oracle_guides planes, oracle_upsample, oracle_filter_var), nothing is the
product's but the world builders and the camera block.

Two 80 x 48 HIGH frames of VRT_MODE_FULL, tests/filter_quality.py's worlds: the reference's room from inside and the emitter lamp
room from inside. The reference is the mean of N_REF = 256 jittered high-resolution samples of OTHER sample indices; the metric
profiles/filter_quality.txt's, the mean over live high pixels of (x - ref)^2 / (ref^2 + 0.01). Compared at EQUAL shaded-sample cost:
the high-resolution mean of n = 4 jittered samples against the low-resolution mean of r^2 n jittered samples at 80 / r x 48 / r,
upsampled with the low frame's own planes and the high frame's one-corner-sample planes (vrt_guide_frame's), for r = 2 and 4; the
same with the unresolved pixels replaced by the high-resolution n-sample mean's (the caller's repair: those pixels re-shaded at the
same cost per pixel); the unresolved share; and both sides after vrt_filter_var_default (the high mean with its own planes, the
upsampled image with the corner planes, both with the filter's spatial variance estimate).

    python tests/upsample_quality.py            writes profiles/upsample_quality.txt (the sweep over the flag, sigmas and min_weight)"""
import os
import sys

import numpy as np

W, H = 80, 48
FIRST, N_IN = 5, 4
REF_FIRST, N_REF = 1000, 256
FACTORS = (2, 4)
MODE_FULL = 2
WORLDS = ("room", "lamp")


def mean_of(L, scene, w, h, first, n):
    import oracle_hdr
    acc = oracle_hdr.Accum(L, h, w)
    for k in range(first, first + n):
        acc.add(oracle_hdr.render(L, scene, w, h, MODE_FULL, k, jitter=True))
    return acc.mean()


def inputs(V, O, L, LG, name):
    """-> {"ref", "high": the n-sample high mean, "high_guides": its planes, "corner": the high corner planes, r: (low mean, low planes)}"""
    import oracle_guides
    from filter_quality import _world
    w, pose = _world(V, name)
    tex, dim = w.flatten()
    w.close()

    def scene(width, height):
        return O.make_scene(tex, dim, *V.camera_block(pose[:3], pose[3], pose[4], width, height)[:3])

    hi = scene(W, H)
    d = {"ref": mean_of(L, hi, W, H, REF_FIRST, N_REF), "high": mean_of(L, hi, W, H, FIRST, N_IN),
         "high_guides": oracle_guides.planes(LG, hi, W, H, FIRST, N_IN, jitter=True)[0], "corner": oracle_guides.planes(LG, hi, W, H, 0, 1)[0]}
    for r in FACTORS:
        lo = scene(W // r, H // r)
        d[r] = (mean_of(L, lo, W // r, H // r, FIRST, r * r * N_IN), oracle_guides.planes(LG, lo, W // r, H // r, FIRST, r * r * N_IN, jitter=True)[0])
    return d


def metric(x, ref, live):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float((((x - ref) ** 2) / (ref ** 2 + 0.01))[live].mean())


def upsampled(L, d, r, **kw):
    """-> (image, repaired image, unresolved share among live high pixels)"""
    import oracle_upsample as U
    out, _, mask = U.upsample(L, d[r][0], d[r][1], d["corner"], U.make(r, offset_lo=(0.5, 0.5), **kw))
    live = d["corner"]["coverage"] > 0
    return out, np.where((mask != 0)[..., None], d["high"], out), float((mask != 0)[live].mean())


def main():
    import tempfile
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    sys.path[:0] = [root, tests, os.path.join(root, "oracle")]
    import oracle_filter_var as FV
    import oracle_guides
    import oracle_py as O
    import oracle_upsample as U
    import vrt_import
    O.build()
    V = vrt_import.vrt()
    tmp = tempfile.mkdtemp()
    L, LV, LG = U.build(tmp), FV.build(tmp), oracle_guides.build(tmp)
    data = {n: inputs(V, O, L, LG, n) for n in WORLDS}
    live = {n: data[n]["corner"]["coverage"] > 0 for n in WORLDS}
    fv = FV.make(**V.default_filter_var())
    base = {n: metric(data[n]["high"], data[n]["ref"], live[n]) for n in WORLDS}
    base_f = {n: metric(FV.filter(LV, data[n]["high"], data[n]["high_guides"], fv)[0], data[n]["ref"], live[n]) for n in WORLDS}
    lines = ["# Guided upsampling (vrt_upsample_hdr): error against a 256-sample high-resolution reference at equal shaded-sample cost, CPU",
             f"# checkers only (tests/upsample_quality.py). {W} x {H} high frames of VRT_MODE_FULL; 'high' = the mean of the {N_IN} jittered high-resolution",
             f"# samples {FIRST}..{FIRST + N_IN - 1}; 'r' = the mean of r^2 * {N_IN} jittered samples at {W} / r x {H} / r upsampled with its own planes and the",
             f"# high frame's one-corner-sample planes; reference = the mean of the high-resolution samples {REF_FIRST}..{REF_FIRST + N_REF - 1}. Metric: mean over",
             "# live high pixels of (x - ref)^2 / (ref^2 + 0.01); lower is better. 'rep' = unresolved pixels replaced by the high mean's (the",
             "# caller's repair at the same cost per pixel); 'unres' = the unresolved share of live high pixels; '+f' = after",
             "# vrt_filter_var_default (the high mean with its own planes, the upsampled image with the corner planes, spatial variance).",
             "# ratio = upsampled / high, summed over both worlds and both factors, unrepaired and unfiltered: what the sweep ranks by.",
             "#", "# world  high      high+f"]
    for n in WORLDS:
        lines.append(f"# {n:5s}  {base[n]:.5f}  {base_f[n]:.5f}")
    lines += ["#", "# demod sigma_normal sigma_albedo sigma_depth min_weight | per world and factor: error, repaired, unresolved share | ratio",
              "#                                                       | room r2                 room r4                 lamp r2                 lamp r4"]
    rows = []
    for demod in (True, False):
        for sn in (0.5, 1.0, 2.0):
            for sa in (0.05, 0.1, 0.25, 0.5):
                for sd in (0.5, 1.0, 2.0, 4.0, 8.0):
                    for mw in (0.0, 0.05, 0.25):
                        cells, total = [], 0.0
                        for n in WORLDS:
                            for r in FACTORS:
                                out, rep, share = upsampled(L, data[n], r, demodulate=demod, sigma_normal=sn, sigma_albedo=sa, sigma_depth=sd,
                                                            min_weight=mw)
                                e = metric(out, data[n]["ref"], live[n])
                                cells.append((e, metric(rep, data[n]["ref"], live[n]), share))
                                total += e
                        rows.append((total / (len(FACTORS) * sum(base.values())), demod, sn, sa, sd, mw, cells))
    for ratio, demod, sn, sa, sd, mw, cells in rows:
        lines.append(f"  {int(demod)}     {sn:<12g} {sa:<12g} {sd:<11g} {mw:<10g} | " + "  ".join(f"{e:.5f} {p:.5f} {s:.4f}" for e, p, s in cells)
                     + f" | {ratio:.4f}")
    best = min(rows, key=lambda row: row[0])
    kw = dict(demodulate=best[1], sigma_normal=best[2], sigma_albedo=best[3], sigma_depth=best[4], min_weight=best[5])
    lines.append(f"# best: demodulate {int(best[1])} sigma_normal {best[2]:g} sigma_albedo {best[3]:g} sigma_depth {best[4]:g} min_weight {best[5]:g}"
                 f" ratio {best[0]:.4f}")
    lines += ["#", "# The best row per world and factor, beside the high-resolution mean at the same cost (x: upsampling loses):",
              "# world r   high     upsampled  repaired   unres    | high+f   upsampled+f  repaired+f"]
    for n in WORLDS:
        for r in FACTORS:
            out, rep, share = upsampled(L, data[n], r, **kw)
            e, p = metric(out, data[n]["ref"], live[n]), metric(rep, data[n]["ref"], live[n])
            ef, pf = (metric(FV.filter(LV, img, data[n]["corner"], fv)[0], data[n]["ref"], live[n]) for img in (out, rep))
            lines.append(f"# {n:5s} {r}   {base[n]:.5f}  {e:.5f}{'x' if e > base[n] else ' '}   {p:.5f}{'x' if p > base[n] else ' '}   {share:.4f}   | "
                         f"{base_f[n]:.5f}  {ef:.5f}{'x' if ef > base_f[n] else ' '}     {pf:.5f}{'x' if pf > base_f[n] else ' '}")
    with open(os.path.join(root, "profiles", "upsample_quality.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[-10:]))


if __name__ == "__main__":
    main()
