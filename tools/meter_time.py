"""Times auto-exposure (vrt_meter_hdr, vrt_tonemap_hdr) on device buffers at 1080p and 4K:
python tools/meter_time.py [--json PATH] [--label NAME] [--other-lib PATH --other-label NAME] [--quality PATH]

The inputs are real ones: the reference's room seen from inside and the dragon outdoors against the sky, each as the float mean of a
two-sample HDR accumulation of VRT_MODE_FULL, resolved on the device. Timed, as tools/upsample_time.py times its pass -- the median of
five windows of --calls calls between two events on a side stream after as many warm-up calls:
  * vrt_meter_hdr (the memset of the histogram, the histogram pass, the finishing step): 12 bytes read per pixel;
  * vrt_tonemap_hdr by the record: 12 bytes read, 4 written per pixel;
  * vrt_accum_resolve_hdr_device with the float mean and the bytes out, at the same size in the same run, the yardstick: 24 bytes of
    float64 sums read, 16 written per pixel.
`gb_per_s` is those bytes over the time. --json appends one line per timing (what profiles/meter_rate.jsonl holds).
--other-lib PATH times vrt_meter_hdr of a second build of libvrt_hip.so (the other form of the histogram's LDS add, built with
-DVRT_METER_MERGE=1 or 0) on the same device image in the same run, alternated with this build's (what profiles/meter_ab.txt holds).
--quality PATH writes the metered exposure at the defaults and the share of output bytes at 0 and at 255 with that exposure against
exposure 1, for both scenes at 1080p and both operators (what profiles/meter_quality.txt holds)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vrt_import  # noqa: E402

SIZES = {"1080p": (1920, 1080), "4K": (3840, 2160)}
SCENES = {"room": (14.5, 30.5, 16.5, 32.0, -10.0),        # tools/filter_time.py's room pose
          "dragon": (63.5, 60.5, 140.5, -90.0, -10.0)}    # the smoke test's dragon pose: sky around it


class OtherBuild:
    """vrt_meter_hdr of a second libvrt_hip.so, on a context of its own (the call is stateless: it needs one for its stream)"""
    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.vrt_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        self.L.vrt_meter_hdr.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        self.L.vrt_synchronize.argtypes = [C.c_void_p]
        self.L.vrt_destroy.argtypes = [C.c_void_p]
        self.h = C.c_void_p()
        assert self.L.vrt_create(0, C.byref(self.h)) == 0

    def meter(self, w, h, d_rgb, d_hist, d_rec, stream):
        assert self.L.vrt_meter_hdr(self.h, w, h, d_rgb, None, d_hist, d_rec, stream) == 0

    def close(self):
        self.L.vrt_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--label", default="this")
    ap.add_argument("--other-lib")
    ap.add_argument("--other-label", default="other")
    ap.add_argument("--quality")
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    V = vrt_import.vrt()
    import torch
    from conftest import MAPS, room_world
    worlds = {}
    w = room_world(V)
    worlds["room"] = w.flatten()
    w.close()
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    worlds["dragon"] = w.flatten()
    w.close()
    ctx = V.Context(0)
    ctx.set_params(ctx.default_params())
    other = OtherBuild(args.other_lib) if args.other_lib else None
    dev = "cuda:0"
    side = torch.cuda.Stream(device=dev)

    def note(**row):
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
        return float(np.median(ms)), [round(m, 5) for m in ms]

    quality = []
    for scene, pose in SCENES.items():
        ctx.upload_octree(*worlds[scene])
        for size, (W, H) in SIZES.items():
            px = W * H
            mean = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
            out8 = torch.zeros((H, W), dtype=torch.int32, device=dev)
            hist = torch.zeros(256, dtype=torch.int32, device=dev)
            rec = torch.zeros(4, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ctx.set_camera(*V.camera_block(pose[:3], pose[3], pose[4], W, H)[:3])
            ctx.accum_begin(W, H, 0, mode=V.MODE_FULL, hdr=True)
            ctx.accum_add(2)
            ctx.accum_resolve_hdr_device(mean.data_ptr(), None, None)
            ctx.meter_hdr_device(W, H, mean.data_ptr(), hist.data_ptr(), rec.data_ptr())
            ctx.synchronize()
            counts = hist.cpu().numpy().view(np.uint32)
            record = V.meter_resolve(counts)
            row = dict(scene=scene, size=size, width=W, height=H, build=args.label, calls_per_window=args.calls)
            shape = dict(bins_in_use=int(np.count_nonzero(counts)), largest_bin_share=round(float(counts.max()) / px, 4), exposure=record["exposure"])

            def rate(bpp, ms):
                return round(bpp * px / (ms * 1e-3) / 1e9, 1)

            mine = lambda: ctx.meter_hdr_device(W, H, mean.data_ptr(), hist.data_ptr(), rec.data_ptr(), stream=side.cuda_stream)   # noqa: E731
            if other:
                theirs = lambda: other.meter(W, H, mean.data_ptr(), hist.data_ptr(), rec.data_ptr(), side.cuda_stream)   # noqa: E731
                for rnd in range(3):   # alternated, the order swapped from round to round
                    for label, call in ((args.label, mine), (args.other_label, theirs))[::1 if rnd % 2 == 0 else -1]:
                        med, ms = timed(call)
                        note(call="vrt_meter_hdr", round=rnd, ms_median=round(med, 5), ms_windows=ms, bytes_per_pixel=12, gb_per_s=rate(12, med),
                             **dict(row, build=label), **shape)
                continue
            med, ms = timed(mine)
            note(call="vrt_meter_hdr", ms_median=round(med, 5), ms_windows=ms, bytes_per_pixel=12, gb_per_s=rate(12, med), **row, **shape)
            med, ms = timed(lambda: ctx.tonemap_hdr_device(px, mean.data_ptr(), out8.data_ptr(), rec.data_ptr(), "reinhard", 1.0, stream=side.cuda_stream))
            note(call="vrt_tonemap_hdr", ms_median=round(med, 5), ms_windows=ms, bytes_per_pixel=16, gb_per_s=rate(16, med), **row)
            med, ms = timed(lambda: ctx.accum_resolve_hdr_device(mean.data_ptr(), out8.data_ptr(), None, "reinhard", 1.0, stream=side.cuda_stream))
            note(call="vrt_accum_resolve_hdr_device", ms_median=round(med, 5), ms_windows=ms, bytes_per_pixel=40, gb_per_s=rate(40, med), **row)
            if args.quality and size == "1080p":
                for op in ("clamp", "reinhard"):
                    shares = {}
                    for name, state in (("metered", record), ("exposure 1", None)):
                        ctx.tonemap_hdr_device(px, mean.data_ptr(), out8.data_ptr(), rec.data_ptr() if state else None, op, 1.0)
                        ctx.synchronize()
                        b = out8.cpu().numpy().view(np.uint8).reshape(-1, 4)[:, :3]
                        shares[name] = (float((b == 0).mean()), float((b == 255).mean()), float(b.mean()))
                    quality.append((scene, op, record, shares))
    if args.quality:
        with open(args.quality, "a") as f:
            for scene, op, record, shares in quality:
                f.write(f"{scene} 1920x1080 {op}: metered luminance {record['metered']:.6g}, exposure {record['exposure']:.6g}, window {record['window']} pixels\n")
                for name, (z, s, m) in shares.items():
                    f.write(f"    {name:11s} bytes at 0: {100 * z:6.2f} %   at 255: {100 * s:6.2f} %   mean byte {m:6.1f}\n")
    if other:
        other.close()
    ctx.close()


if __name__ == "__main__":
    main()
