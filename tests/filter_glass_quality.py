"""What guides past glass (vrt_set_guide_glass) do for the two guided filters at their defaults -- TEST INFRASTRUCTURE ONLY, CPU only:
everything here is the checkers' (oracle_hdr samples, oracle_guides and oracle_guides_glass planes, oracle_filter_hdr,
oracle_filter_var), nothing is the product's but the world builders, the camera block and the default sigmas.

Two 40 x 24 jittered frames of VRT_MODE_FULL (tests/guide_worlds.py): the lamp room through its pane and the reference's room from
inside. Input, reference and metric are those of tests/filter_quality.py: the mean of 4 samples against the mean of 256 OTHER sample
indices, the mean of (x - ref)^2 / (ref^2 + 0.01) -- over all live pixels, and over the pixels whose first hit is translucent (the
corner ray's surface alpha below 255). vrt_filter_default and vrt_filter_var_default (spatial variance estimate), each with the
first-hit planes and with the past-glass planes of the same four samples.

    python tests/filter_glass_quality.py      writes profiles/filter_glass_quality.txt (about a minute)"""
import os
import sys

import numpy as np

import filter_quality as Q

WORLDS = ("lamp", "room")


def main():
    import tempfile
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    sys.path[:0] = [root, tests, os.path.join(root, "oracle")]
    import guide_worlds as GW
    import oracle_filter_hdr as F
    import oracle_filter_var as FV
    import oracle_guides as G
    import oracle_guides_glass as GG
    import oracle_py as O
    import vrt_import
    O.build()
    V = vrt_import.vrt()
    tmp = tempfile.mkdtemp()
    LV, LG = FV.build(tmp), GG.build(tmp)
    f, fv = F.make(**V.default_filter()), FV.make(**V.default_filter_var())
    lines = ["# Guides past glass (vrt_set_guide_glass) under the guided filters at their defaults: error against a 256-sample reference,",
             "# CPU checkers only (tests/filter_glass_quality.py). 40 x 24 jittered frames of VRT_MODE_FULL (tests/guide_worlds.py: the lamp",
             f"# room through its pane, the room from inside), input = mean of samples {Q.FIRST}..{Q.FIRST + Q.N_IN - 1}, reference = mean of samples",
             f"# {Q.REF_FIRST}..{Q.REF_FIRST + Q.N_REF - 1}. Metric: mean of (x - ref)^2 / (ref^2 + 0.01), lower is better; 'all': over the live pixels of",
             "# either set of planes (coverage > 0 with the first-hit planes: sky seen through glass is live there and not past glass, where",
             "# the filter passes it through); 'glass': over the pixels whose corner ray's first hit is translucent. ratio = filtered /",
             "# unfiltered over the same pixels. filter: vrt_filter_default; filter_var: vrt_filter_var_default with its spatial estimate.",
             "#", "# world  pixels all/glass  filter      planes      all      ratio   glass    ratio"]
    for name in WORLDS:
        w = GW.world(V, name)
        tex, dim = w.flatten()
        w.close()
        scene = O.make_scene(tex, dim, *GW.camera(V, name, (Q.W, Q.H)))
        noisy, ref = Q.mean_of(LV, scene, Q.FIRST, Q.N_IN), Q.mean_of(LV, scene, Q.REF_FIRST, Q.N_REF)
        planes = {"first-hit": G.planes(LG, scene, Q.W, Q.H, Q.FIRST, Q.N_IN, jitter=True)[0],
                  "past-glass": GG.planes(LG, scene, Q.W, Q.H, Q.FIRST, Q.N_IN, jitter=True)[0]}
        corner = G.sample(LG, scene, Q.W, Q.H, 0)
        live = planes["first-hit"]["coverage"] > 0
        glass = live & (corner.hit != 0) & (corner.albedo[..., 3] < 255)
        base = (Q.metric(noisy, ref, live), Q.metric(noisy, ref, glass))
        lines.append(f"  {name:5s}  {int(live.sum()):4d}/{int(glass.sum()):<4d}        unfiltered  -           {base[0]:.5f}  1.0000  {base[1]:.5f}  1.0000")
        for fname, run in (("filter", lambda p: F.filter(LV, noisy, p, f)[0]), ("filter_var", lambda p: FV.filter(LV, noisy, p, fv)[0])):
            for pname, p in planes.items():
                out = run(p)
                e = (Q.metric(out, ref, live), Q.metric(out, ref, glass))
                lines.append(f"  {name:5s}  {int(live.sum()):4d}/{int(glass.sum()):<4d}        {fname:10s}  {pname:10s}  {e[0]:.5f}  {e[0] / base[0]:.4f}  {e[1]:.5f}  {e[1] / base[1]:.4f}")
    with open(os.path.join(root, "profiles", "filter_glass_quality.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[8:]))


if __name__ == "__main__":
    main()
