"""Times bloom (vrt_bloom_hdr) on device buffers at 1080p and 4K:
python tools/bloom_time.py [--json PATH] [--label NAME] [--other-lib PATH --other-label NAME] [--quality PATH]

The inputs are real ones: the lamp room of tests/emit_worlds.py seen from inside, towards its lamp, and the dragon outdoors against
the sky, each as the float mean of a two-sample HDR accumulation of VRT_MODE_FULL, resolved and metered on the device; the bloom reads
the record the meter left there. Timed, as tools/meter_time.py times its passes -- the median of five windows of --calls calls between
two events on a side stream after as many warm-up calls:
  * vrt_bloom_hdr at L = 1, 5 and 8 with the default threshold, knee and intensity, KARIS on, both outputs: 2 L launches a call;
  * the same call on a 32 x 8 frame at L = 1: two launches of one workgroup each, the floor a launch costs in this stream;
  * vrt_accum_resolve_hdr_device with the float mean and the bytes out, at the same size in the same run, the yardstick: 24 bytes of
    float64 sums read, 16 written per pixel.
The byte model of a call, `model_bytes`, counts per launch what it must read and write at least: the first level reads 12 bytes per
frame pixel and writes 16 per pixel of level 1; every further level reads 16 bytes per pixel of the level above and writes 16 per
pixel of its own; a step of the chain reads 16 per pixel of the coarser level and reads and writes 16 per pixel of its own; the
composite reads 12 + 16 and writes 12 + 4 per frame pixel. `gb_per_s` is those bytes over the time; `vs_yardstick` is the call's time
over the yardstick's. `launch_bound_levels` lists the levels whose own bytes would take less than the floor of a launch at the rate
the whole call achieves: below them the call pays for launches, not for bytes. --json appends one line per timing (what
profiles/bloom_rate.jsonl holds).
--other-lib PATH times vrt_bloom_hdr of a second build of libvrt_hip.so (the other form of the down-sampling kernel, built with
-DVRT_BLOOM_GATHER=1 or 0) on the same device image in the same run, alternated with this build's (what profiles/bloom_ab.txt holds).
--quality PATH writes, for both scenes at 1080p with the defaults under the clamp operator, once by the metered record and once at
exposure 1 without one, the share of colour bytes at 255 without and with bloom and the mean absolute byte change outside a 16-pixel
ring round the pixels above the threshold (what profiles/bloom_quality.txt holds)."""
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
LEVELS = (1, 5, 8)
RING = 16


class OtherBuild:
    """vrt_bloom_hdr of a second libvrt_hip.so, on a context of its own (the call is stateless: it needs one for its stream)"""
    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.vrt_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        self.L.vrt_bloom_hdr.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8
        self.L.vrt_destroy.argtypes = [C.c_void_p]
        self.h = C.c_void_p()
        assert self.L.vrt_create(0, C.byref(self.h)) == 0

    def bloom(self, w, h, d_rgb, b, d_rec, d_ws, d_f, d_rgba, stream):
        assert self.L.vrt_bloom_hdr(self.h, w, h, d_rgb, C.byref(b), None, d_rec, d_ws, d_f, d_rgba, stream) == 0

    def close(self):
        self.L.vrt_destroy(self.h)


def level_sizes(w, h, levels):
    out = [(w, h)]
    for _ in range(levels):
        out.append(((out[-1][0] + 1) >> 1, (out[-1][1] + 1) >> 1))
    return out


def model(w, h, levels):
    """-> (the call's bytes, {level: the bytes of the launches that belong to it}); level 0 is the composite"""
    px = [a * b for a, b in level_sizes(w, h, levels)]
    per = {0: (12 + 16 + 12 + 4) * px[0], 1: 12 * px[0] + 16 * px[1]}
    for l in range(2, levels + 1):
        per[l] = 16 * px[l - 1] + 16 * px[l]
    for l in range(1, levels):
        per[l] += 16 * px[l + 1] + 32 * px[l]
    return sum(per.values()), per


def luminance(rgb):
    """E1 of include/vrt.h on float32[H, W, 3]"""
    x = np.clip(np.nan_to_num(rgb, nan=0.0, posinf=65504.0, neginf=0.0), 0.0, 65504.0).astype(np.float32)
    return (np.float32(0.2126) * x[..., 0] + np.float32(0.7152) * x[..., 1]) + np.float32(0.0722) * x[..., 2]


def grown(mask, r):
    """the pixels within r (in the maximum norm) of a set pixel, by an integral image"""
    h, w = mask.shape
    s = np.zeros((h + 1, w + 1), np.int64)
    s[1:, 1:] = np.cumsum(np.cumsum(mask.astype(np.int64), axis=0), axis=1)
    y0, y1 = np.clip(np.arange(h) - r, 0, h), np.clip(np.arange(h) + r + 1, 0, h)
    x0, x1 = np.clip(np.arange(w) - r, 0, w), np.clip(np.arange(w) + r + 1, 0, w)
    return (s[y1][:, x1] - s[y0][:, x1] - s[y1][:, x0] + s[y0][:, x0]) > 0


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
    import emit_worlds as EW
    from conftest import MAPS
    worlds, poses = {}, {"lamp room": EW.POSE, "dragon": EW.DRAGON_POSE}
    w = EW.lamp_room(V)
    worlds["lamp room"] = w.flatten()
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

    # the floor of a launch: two launches of one workgroup each
    tiny = torch.ones((8, 32, 3), dtype=torch.float32, device=dev)
    tiny_ws = torch.zeros(V.bloom_workspace_bytes(32, 8, 1) // 4, dtype=torch.float32, device=dev)
    tiny_f, tiny_b = torch.zeros((8, 32, 3), dtype=torch.float32, device=dev), torch.zeros((8, 32), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    med, ms = timed(lambda: ctx.bloom_hdr_device(32, 8, tiny.data_ptr(), tiny_ws.data_ptr(), tiny_f.data_ptr(), tiny_b.data_ptr(), None,
                                                 {"levels": 1}, stream=side.cuda_stream))
    floor = med / 2
    note(call="vrt_bloom_hdr", scene="ones", size="32x8", levels=1, launches=2, build=args.label, ms_median=round(med, 5), ms_windows=ms,
         ms_per_launch=round(floor, 5), calls_per_window=args.calls)

    quality = []
    for scene, pose in poses.items():
        ctx.upload_octree(*worlds[scene])
        for size, (W, H) in SIZES.items():
            px = W * H
            mean = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
            f = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
            out8 = torch.zeros((H, W), dtype=torch.int32, device=dev)
            ws = torch.zeros(V.bloom_workspace_bytes(W, H, max(LEVELS)) // 4, dtype=torch.float32, device=dev)
            hist = torch.zeros(256, dtype=torch.int32, device=dev)
            rec = torch.zeros(4, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ctx.set_camera(*V.camera_block(pose[:3], pose[3], pose[4], W, H)[:3])
            ctx.accum_begin(W, H, 0, mode=V.MODE_FULL, hdr=True)
            ctx.accum_add(2)
            ctx.accum_resolve_hdr_device(mean.data_ptr(), None, None)
            ctx.meter_hdr_device(W, H, mean.data_ptr(), hist.data_ptr(), rec.data_ptr())
            ctx.synchronize()
            record = V.meter_resolve(hist.cpu().numpy().view(np.uint32))
            row = dict(scene=scene, size=size, width=W, height=H, build=args.label, calls_per_window=args.calls, exposure=record["exposure"])
            yard, yard_ms = timed(lambda: ctx.accum_resolve_hdr_device(mean.data_ptr(), out8.data_ptr(), None, "reinhard", 1.0, stream=side.cuda_stream))
            if not other:
                note(call="vrt_accum_resolve_hdr_device", ms_median=round(yard, 5), ms_windows=yard_ms, model_bytes=40 * px,
                     gb_per_s=round(40 * px / (yard * 1e-3) / 1e9, 1), **row)
            for levels in LEVELS:
                total, per = model(W, H, levels)
                bloom = {"levels": levels}
                mine = lambda: ctx.bloom_hdr_device(W, H, mean.data_ptr(), ws.data_ptr(), f.data_ptr(), out8.data_ptr(), rec.data_ptr(), bloom,   # noqa: E731
                                                    "reinhard", 1.0, stream=side.cuda_stream)

                def report(label, med, ms, **more):
                    rate = total / (med * 1e-3)
                    bound = [l for l in range(1, levels + 1) if per[l] / rate * 1e3 < floor]
                    note(call="vrt_bloom_hdr", levels=levels, launches=2 * levels, ms_median=round(med, 5), ms_windows=ms, model_bytes=total,
                         gb_per_s=round(rate / 1e9, 1), vs_yardstick=round(med / yard, 3), launch_floor_ms=round(2 * levels * floor, 5),
                         launch_bound_levels=bound, **dict(row, build=label), **more)

                if other:
                    b = V.Bloom(levels, V.BLOOM_KARIS, 1.0, 0.5, 0.2)
                    theirs = lambda: other.bloom(W, H, mean.data_ptr(), b, rec.data_ptr(), ws.data_ptr(), f.data_ptr(), out8.data_ptr(), side.cuda_stream)   # noqa: E731
                    for rnd in range(3):   # alternated, the order swapped from round to round
                        for label, call in ((args.label, mine), (args.other_label, theirs))[::1 if rnd % 2 == 0 else -1]:
                            report(label, *timed(call), round=rnd)
                    continue
                report(args.label, *timed(mine))
            if args.quality and size == "1080p":
                lum = luminance(mean.cpu().numpy())
                for name, d_rec, e in (("the metered exposure", rec.data_ptr(), record["exposure"]), ("exposure 1, no record", None, 1.0)):
                    ctx.tonemap_hdr_device(px, mean.data_ptr(), out8.data_ptr(), d_rec, "clamp", 1.0)
                    ctx.synchronize()
                    plain = out8.cpu().numpy().view(np.uint8).reshape(H, W, 4)[..., :3].astype(np.int32)
                    ctx.bloom_hdr_device(W, H, mean.data_ptr(), ws.data_ptr(), f.data_ptr(), out8.data_ptr(), d_rec, None, "clamp", 1.0)
                    ctx.synchronize()
                    glow = out8.cpu().numpy().view(np.uint8).reshape(H, W, 4)[..., :3].astype(np.int32)
                    bright = (lum * np.float32(e)) > 1.0
                    far = ~grown(bright, RING)
                    quality.append((scene, name, e, float(bright.mean()), float((plain == 255).mean()), float((glow == 255).mean()), float(far.mean()),
                                    float(np.abs(glow - plain)[far].mean()) if far.any() else float("nan"),
                                    float(np.abs(glow - plain)[~far].mean()) if (~far).any() else float("nan")))
    if args.quality:
        with open(args.quality, "a") as out:
            for scene, name, e, above, before, after, far_share, far_change, near_change in quality:
                out.write(f"{scene} 1920x1080, clamp, the defaults (L 5, KARIS, threshold 1, knee 0.5, intensity 0.2), {name} ({e:.6g}): "
                          f"{100 * above:.3f} % of the pixels above the threshold\n")
                out.write(f"    colour bytes at 255: {100 * before:6.3f} % without bloom, {100 * after:6.3f} % with it\n")
                out.write(f"    mean absolute byte change: {far_change:.4f} over the {100 * far_share:.2f} % of the pixels farther than {RING} pixels "
                          f"from one above the threshold, {near_change:.4f} over the others\n")
    if other:
        other.close()
    ctx.close()


if __name__ == "__main__":
    main()
