"""Times the temporal pass (vrt_temporal_hdr) and its accumulation form on device buffers at 1080p:
python tools/temporal_time.py [--json PATH] [--label NAME]

The input is a real one, as tools/filter_time.py's: HDR accumulations of 4 jittered samples of VRT_MODE_FULL of the reference's room
from inside at two poses a slow yaw and a fraction of a voxel apart; the first pose's mean and planes make the history (a first-frame
call), the second pose's are the frame. Timed, each as the median of five windows of --calls calls between two events on a side
stream after as many warm-up calls:
  * vrt_temporal_hdr with every output: on the history under the moved camera, under an identical camera, and as a first frame
    (no history). `bytes_per_pixel` is what the call must move at least -- 32 of inputs, 48 of history where one comes in, 64 of
    outputs -- and `gb_per_s` that over the time.
  * vrt_accum_resolve_hdr_temporal_device (every output, the defaults) against vrt_accum_resolve_hdr_filtered_var_device, the
    spatial-only form, and vrt_accum_resolve_hdr_device (no filter) from the same session.
With --mom the session instead alternates vrt_temporal_hdr with vrt_temporal_hdr_mom -- three pairs, the order swapped within
pairs -- on the same buffers, for each history (moved, identical, first frame) x search 0 / 1 x the variance plane given / NULL
(the plane is vrt_accum_variance_device's of the second pose, whose accumulation is begun with moments), and the two accumulation
forms the same way. The yardstick is the old call in the same session. With search 0 the new call moves 148 compulsory bytes per
pixel with a plane against 144. The share of pixels the search serves is read from the histories: live pixels without a history
at search 0 (an upper bound of those that enter the search: it counts positions outside the previous image too), and those the
search finds one for.
--json appends one line per timing (what profiles/temporal_rate.jsonl holds); --label NAME is recorded with each line."""
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
POSES = ((14.5, 30.5, 16.5, 32.0, -10.0), (14.8, 30.6, 16.3, 33.0, -10.0))   # tools/filter_time.py's room pose, then moved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--label", default="this")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--mom", action="store_true")
    args = ap.parse_args()
    V = vrt_import.vrt()
    import torch
    import temporal_worlds as TW
    from conftest import room_world
    w = room_world(V)
    tex, dim = w.flatten()
    w.close()
    ctx = V.Context(0)
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    dev = "cuda:0"
    cams = [V.camera_block(p[:3], p[3], p[4], W, H)[:3] for p in POSES]
    frames = []
    for cam in cams:
        mean = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        planes = [torch.zeros((H, W, k), dtype=torch.float32, device=dev) for k in (3, 4, 1, 1)]
        torch.cuda.synchronize()
        ctx.set_camera(*cam)
        ctx.accum_begin(W, H, 0, mode=V.MODE_FULL, jitter=True, hdr=True, moments=args.mom)
        ctx.accum_add(4)
        ctx.accum_resolve_hdr_device(mean.data_ptr(), None, None)
        ctx.accum_guides_device(*(p.data_ptr() for p in planes))
        ctx.synchronize()
        frames.append((mean, planes))
    hist = [torch.zeros((3, H, W, 4), dtype=torch.float32, device=dev) for _ in range(2)]
    integ, out = (torch.zeros((H, W, 3), dtype=torch.float32, device=dev) for _ in range(2))
    var, outv = (torch.zeros((H, W), dtype=torch.float32, device=dev) for _ in range(2))
    out8 = torch.zeros((H, W), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    jit = {"offset_x": 0.5, "offset_y": 0.5}

    def pass_(frame, cam, history, prev):
        mean, planes = frames[frame]
        ctx.temporal_hdr_device(W, H, cams[cam], mean.data_ptr(), planes[0].data_ptr(), planes[2].data_ptr(), planes[3].data_ptr(),
                                hist[0].data_ptr() if history else None, hist[1].data_ptr(), integ.data_ptr(), var.data_ptr(),
                                TW.prev_camera(cams[prev]) if history else None, jit, stream=side.cuda_stream)

    side = torch.cuda.Stream(device=dev)
    mean0, planes0 = frames[0]
    ctx.temporal_hdr_device(W, H, cams[0], mean0.data_ptr(), planes0[0].data_ptr(), planes0[2].data_ptr(), planes0[3].data_ptr(), None,
                            hist[0].data_ptr(), None, None, None, jit)
    ctx.synchronize()
    live = float((frames[1][1][3] > 0).float().mean())

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
        row.update(scene="room", width=W, height=H, live_fraction=round(live, 4), calls_per_window=args.calls, build=args.label)
        print(json.dumps(row), flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(json.dumps(row) + "\n")

    if args.mom:
        mvar = torch.zeros((H, W), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ctx.accum_variance_device(mvar.data_ptr())
        ctx.synchronize()

        def mom_(frame, cam, history, prev, search, plane, below=4):
            mean, planes = frames[frame]
            ctx.temporal_hdr_mom_device(W, H, cams[cam], mean.data_ptr(), planes[0].data_ptr(), planes[2].data_ptr(), planes[3].data_ptr(),
                                        mvar.data_ptr() if plane else None, hist[0].data_ptr() if history else None, hist[1].data_ptr(),
                                        integ.data_ptr(), var.data_ptr(), TW.prev_camera(cams[prev]) if history else None,
                                        dict(jit, measured_below=below, search=search), stream=side.cuda_stream)

        def alternate(old, new):
            """three pairs, the order swapped within pairs -> (old's three medians, new's three medians)"""
            a, b = [], []
            for k in range(3):
                for which in ((0, 1) if k % 2 == 0 else (1, 0)):
                    (a if which == 0 else b).append(timed(old if which == 0 else new)[0])
            return a, b

        mid = lambda v: float(np.median(v))                               # noqa: E731
        spread = lambda v: (max(v) - min(v)) / mid(v)                     # noqa: E731
        live_px = frames[1][1][3].reshape(H, W) > 0
        mom_(1, 1, True, 0, 0, True)
        torch.cuda.synchronize()
        found0 = hist[1][0, ..., 3] >= 2
        mom_(1, 1, True, 0, 1, True)
        torch.cuda.synchronize()
        found1 = hist[1][0, ..., 3] >= 2
        shares = dict(no_history_fraction_search0=round(float((live_px & ~found0).float().sum() / live_px.float().sum()), 5),
                      search_found_fraction=round(float((found1 & ~found0).float().sum() / live_px.float().sum()), 5))
        for what, (frame, cam, history), bpp in (("moved camera", (1, 1, True), 144), ("identical camera", (0, 0, True), 144),
                                                 ("first frame", (1, 1, False), 96)):
            for search in (0, 1):
                for plane in (True, False):
                    old, new = alternate(lambda: pass_(frame, cam, history, 0), lambda: mom_(frame, cam, history, 0, search, plane))
                    note(call="vrt_temporal_hdr_mom", against="vrt_temporal_hdr", history=what, search=search, plane=plane,
                         ms_old=[round(m, 5) for m in old], ms_new=[round(m, 5) for m in new], ms_old_median=round(mid(old), 5),
                         ms_new_median=round(mid(new), 5), ratio=round(mid(new) / mid(old), 4), old_spread=round(spread(old), 4),
                         bytes_per_pixel_old=bpp, bytes_per_pixel_new=bpp + (4 if plane else 0), bytes_ratio=round((bpp + (4 if plane else 0)) / bpp, 4),
                         **(shares if what == "moved camera" else {}))
        acc_old = lambda: ctx.accum_resolve_hdr_temporal_device(                     # noqa: E731
            hist[0].data_ptr(), hist[1].data_ptr(), integ.data_ptr(), out.data_ptr(), out8.data_ptr(), outv.data_ptr(), TW.prev_camera(cams[0]),
            None, None, "reinhard", 1.0, stream=side.cuda_stream)
        for search in (0, 1):
            acc_new = lambda: ctx.accum_resolve_hdr_temporal_mom_device(             # noqa: E731
                hist[0].data_ptr(), hist[1].data_ptr(), integ.data_ptr(), out.data_ptr(), out8.data_ptr(), outv.data_ptr(), TW.prev_camera(cams[0]),
                {"measured_below": 4, "search": search}, None, "reinhard", 1.0, stream=side.cuda_stream)
            old, new = alternate(acc_old, acc_new)
            note(call="vrt_accum_resolve_hdr_temporal_mom_device", against="vrt_accum_resolve_hdr_temporal_device", search=search,
                 ms_old=[round(m, 5) for m in old], ms_new=[round(m, 5) for m in new], ms_old_median=round(mid(old), 5),
                 ms_new_median=round(mid(new), 5), ratio=round(mid(new) / mid(old), 4), old_spread=round(spread(old), 4))
        ctx.close()
        return
    for what, call, bpp in (("moved camera", lambda: pass_(1, 1, True, 0), 144), ("identical camera", lambda: pass_(0, 0, True, 0), 144),
                            ("first frame", lambda: pass_(1, 1, False, 0), 96)):
        med, ms = timed(call)
        pass_(1, 1, True, 0)
        torch.cuda.synchronize()
        grown = float((hist[1][0, ..., 3] >= 2).float().mean()) if what == "moved camera" else None
        note(call="vrt_temporal_hdr", history=what, ms_median=round(med, 5), ms_windows=[round(m, 5) for m in ms], bytes_per_pixel=bpp,
             gb_per_s=round(bpp * W * H / (med * 1e-3) / 1e9, 1), history_found_fraction=None if grown is None else round(grown, 4))
    # the accumulation at the second pose is the context's current one
    routes = (("vrt_accum_resolve_hdr_device", lambda: ctx.accum_resolve_hdr_device(out.data_ptr(), out8.data_ptr(), None, "reinhard", 1.0,
                                                                                     stream=side.cuda_stream)),
              ("vrt_accum_resolve_hdr_filtered_var_device", lambda: ctx.accum_resolve_hdr_filtered_var_device(
                  out.data_ptr(), out8.data_ptr(), outv.data_ptr(), None, "reinhard", 1.0, stream=side.cuda_stream)),
              ("vrt_accum_resolve_hdr_temporal_device", lambda: ctx.accum_resolve_hdr_temporal_device(
                  hist[0].data_ptr(), hist[1].data_ptr(), integ.data_ptr(), out.data_ptr(), out8.data_ptr(), outv.data_ptr(),
                  TW.prev_camera(cams[0]), None, None, "reinhard", 1.0, stream=side.cuda_stream)))
    for name, call in routes:
        med, ms = timed(call)
        note(call=name, ms_median=round(med, 5), ms_windows=[round(m, 5) for m in ms])
    ctx.close()


if __name__ == "__main__":
    main()
