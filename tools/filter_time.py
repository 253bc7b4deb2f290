"""Times the guided filter (vrt_filter_hdr) on device buffers at 1080p: python tools/filter_time.py [--json PATH] [--scene room|mis]

The input is a real one: an HDR accumulation of 4 jittered samples of VRT_MODE_FULL of the scene (the reference's room from inside,
or tests/emit_mis_worlds.py's lamp room from inside), its float mean (vrt_accum_resolve_hdr_device) and its guide planes
(vrt_accum_guides_device). Timed, each as the median of five windows of --calls calls between two events on a side stream after
as many warm-up calls (the windows' min and max are the run-to-run figure):
  * vrt_filter_hdr with both outputs for levels 0..5 (sigmas: the defaults), demodulation on and off. `level_ms` is the difference
    to the row with one level fewer: what the level with step 1 << (levels - 1) adds to the call (for levels 1: prepass + first level).
  * the accumulation route, vrt_accum_resolve_hdr_filtered_device at the defaults and at 5 levels, against
    vrt_accum_resolve_hdr_shown_device (the ID-aware blur on the same mean) and vrt_accum_resolve_hdr_device (no filter).
--var times the variance-guided filter instead (vrt_filter_hdr_var, all three outputs, sigmas: its defaults) for the same levels, with
the spatial estimate and with a supplied plane (the input's own spatial estimate, taken from a levels-0 call), beside vrt_filter_hdr
at the same level counts and the guide sigmas of the same defaults in the same session; and, at levels 0, the call with and without
the variance output: the difference is the prepass and the variance kernel (what profiles/filter_var_rate.jsonl holds).
--json appends one line per timing (what profiles/filter_rate.jsonl holds); --label NAME is recorded with each line (A/B builds)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vrt_import  # noqa: E402

W, H = 1920, 1080
SCENES = {"room": (14.5, 30.5, 16.5, 32.0, -10.0), "mis": (36.5, 44.5, 50.5, -20.0, -35.0)}   # tools/accum_rate.py's poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--label", default="this")
    ap.add_argument("--scene", default="room", choices=sorted(SCENES))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--levels", nargs="+", type=int, default=[0, 1, 2, 3, 4, 5])
    ap.add_argument("--var", action="store_true", help="the variance-guided filter beside the guide-only one (see above)")
    args = ap.parse_args()
    V = vrt_import.vrt()
    import torch
    from conftest import room_world
    if args.scene == "room":
        w = room_world(V)
    else:
        import emit_mis_worlds
        w = emit_mis_worlds.room(V)
    tex, dim = w.flatten()
    w.close()
    pose = SCENES[args.scene]
    ctx = V.Context(0)
    ctx.upload_octree(tex, dim)
    ctx.set_camera(*V.camera_block(pose[:3], pose[3], pose[4], W, H)[:3])
    ctx.set_params(ctx.default_params())
    ctx.accum_begin(W, H, 0, mode=V.MODE_FULL, jitter=True, hdr=True)
    ctx.accum_add(4)
    dev = "cuda:0"
    mean = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    planes = [torch.zeros((H, W, k), dtype=torch.float32, device=dev) for k in (3, 4, 1, 1)]
    out = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    out8 = torch.zeros((H, W), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.accum_resolve_hdr_device(mean.data_ptr(), None, None)
    ctx.accum_guides_device(*(p.data_ptr() for p in planes))
    ctx.synchronize()
    live = float((planes[3] > 0).float().mean())
    side = torch.cuda.Stream(device=dev)

    def timed(call):
        for _ in range(args.calls):
            call()
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            for _ in range(args.calls):
                call()
            e1.record(side)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.calls)
        return float(np.median(ms)), ms

    def note(**row):
        row.update(scene=args.scene, width=W, height=H, live_fraction=round(live, 4), calls_per_window=args.calls, build=args.label)
        print(json.dumps(row), flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(json.dumps(row) + "\n")

    if args.var:
        dv = V.default_filter_var()
        guide = {k: v for k, v in dv.items() if k != "sigma_lum"}
        outv = torch.zeros((H, W), dtype=torch.float32, device=dev)
        plane = torch.zeros((H, W), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ins = [mean.data_ptr()] + [p.data_ptr() for p in planes]
        ctx.filter_hdr_var_device(W, H, *ins, None, out.data_ptr(), None, plane.data_ptr(), dict(dv, levels=0))
        ctx.synchronize()
        prev = {}
        for levels in args.levels:
            rows = (("vrt_filter_hdr", None, lambda: ctx.filter_hdr_device(W, H, *ins, out.data_ptr(), out8.data_ptr(), dict(guide, levels=levels),
                                                                           "reinhard", 1.0, stream=side.cuda_stream)),
                    ("vrt_filter_hdr_var", "spatial", lambda: ctx.filter_hdr_var_device(W, H, *ins, None, out.data_ptr(), out8.data_ptr(), outv.data_ptr(),
                                                                                        dict(dv, levels=levels), "reinhard", 1.0, stream=side.cuda_stream)),
                    ("vrt_filter_hdr_var", "plane", lambda: ctx.filter_hdr_var_device(W, H, *ins, plane.data_ptr(), out.data_ptr(), out8.data_ptr(),
                                                                                      outv.data_ptr(), dict(dv, levels=levels), "reinhard", 1.0,
                                                                                      stream=side.cuda_stream)))
            if levels == 0:
                rows += (("vrt_filter_hdr_var", "no variance output", lambda: ctx.filter_hdr_var_device(
                    W, H, *ins, None, out.data_ptr(), out8.data_ptr(), None, dict(dv, levels=0), "reinhard", 1.0, stream=side.cuda_stream)),)
            for name, source, call in rows:
                med, ms = timed(call)
                key = (name, source)
                note(call=name, variance=source, levels=levels, demodulate=dv["demodulate"], ms_median=round(med, 5),
                     ms_windows=[round(m, 5) for m in ms], level_ms=None if key not in prev else round(med - prev[key], 5))
                prev[key] = med
        for name, levels, call in (("vrt_accum_resolve_hdr_filtered_device", None, lambda: ctx.accum_resolve_hdr_filtered_device(
                                        out.data_ptr(), out8.data_ptr(), guide, "reinhard", 1.0, stream=side.cuda_stream)),
                                   ("vrt_accum_resolve_hdr_filtered_var_device", None, lambda: ctx.accum_resolve_hdr_filtered_var_device(
                                        out.data_ptr(), out8.data_ptr(), outv.data_ptr(), None, "reinhard", 1.0, stream=side.cuda_stream))):
            med, ms = timed(call)
            note(call=name, levels=dv["levels"], demodulate=dv["demodulate"], ms_median=round(med, 5), ms_windows=[round(m, 5) for m in ms])
        ctx.close()
        return
    d = V.default_filter()
    for demod in (True, False):
        prev = None
        for levels in args.levels:
            f = dict(d, levels=levels, demodulate=demod)
            med, ms = timed(lambda: ctx.filter_hdr_device(W, H, mean.data_ptr(), *(p.data_ptr() for p in planes), out.data_ptr(), out8.data_ptr(),
                                                          f, "reinhard", 1.0, stream=side.cuda_stream))
            note(call="vrt_filter_hdr", levels=levels, demodulate=demod, ms_median=round(med, 5), ms_windows=[round(m, 5) for m in ms],
                 level_ms=None if prev is None else round(med - prev, 5))
            prev = med
    routes = (("vrt_accum_resolve_hdr_device", None, lambda: ctx.accum_resolve_hdr_device(out.data_ptr(), out8.data_ptr(), None, "reinhard", 1.0, stream=side.cuda_stream)),
              ("vrt_accum_resolve_hdr_shown_device", None, lambda: ctx.accum_resolve_hdr_shown_device(out.data_ptr(), out8.data_ptr(), "reinhard", 1.0, stream=side.cuda_stream)),
              ("vrt_accum_resolve_hdr_filtered_device", d["levels"], lambda: ctx.accum_resolve_hdr_filtered_device(out.data_ptr(), out8.data_ptr(), None, "reinhard", 1.0, stream=side.cuda_stream)),
              ("vrt_accum_resolve_hdr_filtered_device", 5, lambda: ctx.accum_resolve_hdr_filtered_device(out.data_ptr(), out8.data_ptr(), dict(d, levels=5), "reinhard", 1.0, stream=side.cuda_stream)))
    for name, levels, call in routes:
        med, ms = timed(call)
        note(call=name, levels=levels, demodulate=d["demodulate"] if levels is not None else None, ms_median=round(med, 5),
             ms_windows=[round(m, 5) for m in ms])
    ctx.close()


if __name__ == "__main__":
    main()
