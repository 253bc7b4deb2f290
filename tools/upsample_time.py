"""Times guided upsampling (vrt_upsample_hdr, vrt_guide_frame_device, vrt_accum_resolve_hdr_upsampled_device) on device buffers at 1080p:
python tools/upsample_time.py [--json PATH] [--label NAME]

The input is a real one, as tools/temporal_time.py's: the reference's room from inside. For each factor r in (2, 4) an HDR
accumulation of 4 jittered samples of VRT_MODE_FULL at 1920 / r x 1080 / r gives the LOW mean and planes, vrt_guide_frame_device the
HIGH planes at 1920 x 1080. Timed:
  * vrt_upsample_hdr with every output, as the median of five windows of --calls calls between two events on a side stream after as
    many warm-up calls. `bytes_per_pixel` is what the call must move at least per HIGH pixel -- 36 of high planes, 17 of outputs,
    48 / r^2 of the low side -- and `gb_per_s` that over the time. `unresolved_fraction` is read from the mask.
  * vrt_guide_frame_device at 1080p the same way (the march on the context's stream, the resolve on the side stream).
  * end to end at path depth 1 and 4, each as the median of five runs timed on the host around a device synchronise after one
    warm-up run: a 16-sample jittered HDR add at 960 x 540 plus vrt_accum_resolve_hdr_upsampled_device at factor 2, against the
    16-sample add at 1920 x 1080 plus vrt_accum_resolve_hdr_device.
--json appends one line per timing (what profiles/upsample_rate.jsonl holds); --label NAME is recorded with each line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vrt_import  # noqa: E402

W, H = 1920, 1080
POSE = (14.5, 30.5, 16.5, 32.0, -10.0)   # tools/filter_time.py's room pose


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--label", default="this")
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    V = vrt_import.vrt()
    import torch
    from conftest import room_world
    w = room_world(V)
    tex, dim = w.flatten()
    w.close()
    ctx = V.Context(0)
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    dev = "cuda:0"
    f32 = dict(dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(device=dev)

    def camera(width, height):
        return V.camera_block(POSE[:3], POSE[3], POSE[4], width, height)[:3]

    def planes(width, height):
        return [torch.zeros((height, width, k), **f32) for k in (3, 4, 1, 1)]

    def note(**row):
        row.update(scene="room", width=W, height=H, build=args.label)
        print(json.dumps(row), flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(json.dumps(row) + "\n")

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
            ctx.synchronize()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.calls)
        return float(np.median(ms)), ms

    hi = planes(W, H)
    out = torch.zeros((H, W, 3), **f32)
    out8 = torch.zeros((H, W), dtype=torch.int32, device=dev)
    mask = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.set_camera(*camera(W, H))
    ctx.guide_frame_device(W, H, *(p.data_ptr() for p in hi))
    ctx.synchronize()
    live = float((hi[3] > 0).float().mean())
    for r in (2, 4):
        lw, lh = W // r, H // r
        mean = torch.zeros((lh, lw, 3), **f32)
        lo = planes(lw, lh)
        torch.cuda.synchronize()
        ctx.set_camera(*camera(lw, lh))
        ctx.accum_begin(lw, lh, 0, mode=V.MODE_FULL, jitter=True, hdr=True)
        ctx.accum_add(4)
        ctx.accum_resolve_hdr_device(mean.data_ptr(), None, None)
        ctx.accum_guides_device(*(p.data_ptr() for p in lo))
        ctx.synchronize()
        u = {"factor": r, "offset_lo_x": 0.5, "offset_lo_y": 0.5}
        call = lambda: ctx.upsample_hdr_device(lw, lh, mean.data_ptr(), *(p.data_ptr() for p in lo), *(p.data_ptr() for p in hi),   # noqa: E731
                                               out.data_ptr(), out8.data_ptr(), mask.data_ptr(), u, "reinhard", 1.0, stream=side.cuda_stream)
        med, ms = timed(call)
        bpp = 36 + 17 + 48 / (r * r)
        note(call="vrt_upsample_hdr", factor=r, low=[lw, lh], ms_median=round(med, 5), ms_windows=[round(m, 5) for m in ms],
             bytes_per_high_pixel=bpp, gb_per_s=round(bpp * W * H / (med * 1e-3) / 1e9, 1), live_fraction=round(live, 4),
             unresolved_fraction=round(float((mask != 0).float().mean()), 5), calls_per_window=args.calls)
    ctx.set_camera(*camera(W, H))
    med, ms = timed(lambda: ctx.guide_frame_device(W, H, *(p.data_ptr() for p in hi), stream=side.cuda_stream))
    note(call="vrt_guide_frame_device", ms_median=round(med, 5), ms_windows=[round(m, 5) for m in ms], calls_per_window=args.calls)

    def run(low):
        width, height = (W // 2, H // 2) if low else (W, H)
        ctx.set_camera(*camera(width, height))
        ctx.accum_begin(width, height, 0, mode=V.MODE_FULL, jitter=True, hdr=True)
        ctx.accum_add(16)
        if low:
            ctx.accum_resolve_hdr_upsampled_device(out.data_ptr(), out8.data_ptr(), mask.data_ptr(), {"factor": 2}, "reinhard", 1.0)
        else:
            ctx.accum_resolve_hdr_device(out.data_ptr(), out8.data_ptr(), None, "reinhard", 1.0)
        ctx.synchronize()

    for depth in (1, 4):
        ctx.set_path_depth(depth)
        row = {}
        for low in (True, False):
            run(low)
            ms = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(low)
                ms.append((time.perf_counter() - t0) * 1e3)
            row["low" if low else "full"] = (float(np.median(ms)), ms)
        note(call="16-sample add + resolve", path_depth=depth, ms_540p_upsampled_median=round(row["low"][0], 4),
             ms_540p_upsampled_runs=[round(m, 4) for m in row["low"][1]], ms_1080p_median=round(row["full"][0], 4),
             ms_1080p_runs=[round(m, 4) for m in row["full"][1]], ratio=round(row["low"][0] / row["full"][0], 4))
    ctx.close()


if __name__ == "__main__":
    main()
