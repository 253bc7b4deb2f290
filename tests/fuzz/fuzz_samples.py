"""Parity fuzz of the sample stack over SYNTHETIC worlds (not part of the test suite; the suite's bounded version is
tests/test_gpu_sample_sweep.py): the worlds of tests/sample_sweep_worlds.py -- its six families in turn, under this run's seed, at
any index -- each at a DRAWN setting (path depth, sun radius, emitter rule, ray source, variant) instead of a scheduled one, through
every route test_gpu_sample_sweep.run_case compares with the checkers: accumulations plain, adaptive, HDR and with moments, the
primary modes, the guide planes plain and past glass, and the world's ray batch through shade_rays, shade_rays_hdr and guide_rays.
One MISMATCH line per failing (world, setting, route), with the arguments that replay it; exit status 1 on any mismatch. One
process, one context.
usage: tests/fuzz/fuzz_samples.py [n_worlds] [seed]
       tests/fuzz/fuzz_samples.py --case FAMILY INDEX [SEED D RADIUS RULE SOURCE VARIANT]   (FAMILY INDEX alone: the suite's case)"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_py as O  # noqa: E402
import vrt_import  # noqa: E402
import sample_sweep_worlds as sw  # noqa: E402
import test_gpu_sample_sweep as sweep  # noqa: E402

V = vrt_import.vrt()


def replay_args(case):
    s = case.setting
    return f"--case {case.family} {case.index} {case.seed} {s['D']} {s['radius']} {s['rule']} {s['source']} {s['variant']}"


def run(ctx, libs, case, counts):
    def report(route, check):
        counts["routes"] += 1
        try:
            check()
        except AssertionError as e:
            counts["bad"] += 1
            print("MISMATCH", replay_args(case), "|", f"{case.W} x {case.H}", "route:", route, "|", str(e).splitlines()[0][:300], flush=True)
    try:
        sweep.run_case(ctx, V, O, libs, case, report)
    finally:
        sweep.reset(ctx)


def main(argv):
    O.build()
    libs = sweep.build_libs(tempfile.mkdtemp(prefix="fuzz_samples_"))
    ctx = V.Context(0)
    counts = {"routes": 0, "bad": 0}
    t0 = time.time()
    if argv[:1] == ["--case"]:
        family, index = argv[1], int(argv[2])
        kw = {}
        if len(argv) > 3:
            kw = {"seed": int(argv[3]), "setting": {"D": int(argv[4]), "radius": float(argv[5]), "rule": argv[6], "source": argv[7],
                                                    "variant": int(argv[8])}}
        case = sw.case(V, O, family, index, **kw)
        print(case.name(), "pose", case.pose, "lens", case.lens, "uniforms", case.uniforms, flush=True)
        run(ctx, libs, case, counts)
        case.close()
        print("sample fuzz case done:", counts["routes"], "routes,", counts["bad"], "mismatches")
    else:
        n = int(argv[0]) if argv else 50
        seed = int(argv[1]) if len(argv) > 1 else 1
        skipped = 0
        for number in range(n):
            family, index = sw.FAMILIES[number % len(sw.FAMILIES)], number // len(sw.FAMILIES)
            rng = np.random.default_rng([seed, 99, number])
            idx = [int(rng.integers(0, len(axis))) for axis in sw.AXES]
            if sw.sampling_off(family, index):
                idx[2] = 0
            try:
                case = sw.case(V, O, family, index, setting=sw.setting_of(idx), seed=seed)
            except AssertionError as e:   # the generator found no pose in its nine draws, or no room for a cube: not a parity matter
                skipped += 1
                print("SKIPPED", family, index, "seed", seed, "|", str(e)[:200], flush=True)
                continue
            run(ctx, libs, case, counts)
            case.close()
            if number % 10 == 9:
                print(number + 1, "worlds,", counts["routes"], "routes,", counts["bad"], "mismatches, %.0f s" % (time.time() - t0), flush=True)
        print("sample fuzz done:", n, "worlds,", skipped, "skipped,", counts["routes"], "routes,", counts["bad"], "mismatches, seed", seed)
    ctx.close()
    sys.exit(1 if counts["bad"] else 0)


main(sys.argv[1:])
