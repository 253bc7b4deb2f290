"""Parity fuzz of edit sessions (not part of the test suite; the suite's bounded version is tests/test_gpu_edit_sessions.py): the
worlds of tests/sample_sweep_worlds.py -- its six families in turn, under this run's seed, at any index -- each taken through a
session of a DRAWN plan (edit_sessions.draw_plan: two to five groups out of the vocabulary of tests/edit_sessions.py) on ONE context
per session, patched from the first upload to the last checkpoint, and at every checkpoint through every route
test_gpu_edit_sessions.run_session compares with the checkers. One MISMATCH line per failing (session, checkpoint, route), with the
arguments that replay it; exit status 1 on any mismatch.
usage: tests/fuzz/fuzz_edits.py [n_sessions] [seed]
       tests/fuzz/fuzz_edits.py --case FAMILY INDEX [SEED]   (FAMILY INDEX alone: the suite's session; with SEED: the fuzzer's)"""
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
import edit_sessions as es  # noqa: E402
import test_gpu_edit_sessions as sessions  # noqa: E402
import test_gpu_sample_sweep as sweep  # noqa: E402

V = vrt_import.vrt()


def run(libs, family, index, seed, counts):
    """seed None: the suite's session (family, index); else a drawn plan under that seed"""
    plan = None if seed is None else es.draw_plan(np.random.default_rng([seed, 98, es.FAMILIES.index(family), index]), family, index)
    replay = f"--case {family} {index}" + ("" if seed is None else f" {seed}")

    def report(route, check):
        counts["routes"] += 1
        try:
            check()
        except AssertionError as e:
            counts["bad"] += 1
            print("MISMATCH", replay, "| route:", route, "|", str(e).splitlines()[0][:300], flush=True)
    ctx = V.Context(0)
    try:
        sessions.run_session(ctx, V, O, libs, family, index, seed=es.SEED if seed is None else seed, plan=plan, report=report)
    except AssertionError as e:   # the generator found no pose, or an item no place for its edit: not a parity matter
        counts["skipped"] += 1
        print("SKIPPED", replay, "|", str(e)[:200], flush=True)
    finally:
        ctx.close()
    return plan


def main(argv):
    O.build()
    libs = sweep.build_libs(tempfile.mkdtemp(prefix="fuzz_edits_"))
    counts = {"routes": 0, "bad": 0, "skipped": 0}
    t0 = time.time()
    if argv[:1] == ["--case"]:
        family, index = argv[1], int(argv[2])
        plan = run(libs, family, index, int(argv[3]) if len(argv) > 3 else None, counts)
        print("plan", plan or es.PLAN[(family, index)])
        print("edit fuzz case done:", counts["routes"], "routes,", counts["bad"], "mismatches")
    else:
        n = int(argv[0]) if argv else 24
        seed = int(argv[1]) if len(argv) > 1 else 1
        for number in range(n):
            family, index = es.FAMILIES[number % len(es.FAMILIES)], number // len(es.FAMILIES)
            run(libs, family, index, seed, counts)
            if number % 6 == 5:
                print(number + 1, "sessions,", counts["routes"], "routes,", counts["bad"], "mismatches, %.0f s" % (time.time() - t0), flush=True)
        print("edit fuzz done:", n, "sessions,", counts["skipped"], "skipped,", counts["routes"], "routes,", counts["bad"], "mismatches, seed", seed)
    sys.exit(1 if counts["bad"] else 0)


main(sys.argv[1:])
