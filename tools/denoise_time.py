"""Times the display pass (quad.frag restatement) on device buffers: python tools/denoise_time.py [map] [W H].

--hdr         also times the HDR pass (vrt_denoise_hdr: floats and Reinhard bytes out) on the same frame as a float image, after
              the byte pass of every kind, and checks that the kinds agree bit for bit
--json PATH   appends one JSON line per timing to PATH (what profiles/denoise_hdr_rate.jsonl holds)
--root DIR    imports the package from another checkout DIR (e.g. the parent commit's, built) instead of this one: the same
              tool then times that checkout's byte pass in the same session; --label NAME names the checkout in the JSON lines"""
import json
import os
import sys

import numpy as np


def _flag(name, takes_value=False, default=None):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    v = sys.argv[i + 1] if takes_value else True
    del sys.argv[i:i + (2 if takes_value else 1)]
    return v


HDR = _flag("--hdr", default=False)
JSON_PATH = _flag("--json", True)
ROOT = _flag("--root", True, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LABEL = _flag("--label", True, "this")
sys.path.insert(0, ROOT)
import vrt_import  # noqa: E402

V = vrt_import.vrt()
import torch  # noqa: E402

POSES = {"dragon": (63.5, 60.5, 140.5, -90.0, -10.0), "monu9": (48.5, 60.5, 170.5, -90.0, -12.0),
         "nature": (60.5, 80.5, 330.5, -90.0, -12.0)}


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "dragon"
    W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1920, 1080)
    root = ROOT
    w = V.World()
    assert w.load_vox(os.path.join(root, "tests/golden/maps", name + ".vox"))
    tex, dim = w.flatten()
    ctx = V.Context(0)
    ctx.upload_octree(tex, dim)
    pose = POSES[name]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    ctx.set_camera(ip, iv, cp)
    ctx.set_params(ctx.default_params())
    rgba, idd = ctx.dispatch(W, H, 2)
    if os.environ.get("DENOISE_SYNTH"):        # every pixel summed with one radius: DENOISE_SYNTH=<dist>
        idd[..., 0] = 5
        idd[..., 1] = int(os.environ["DENOISE_SYNTH"])
    d_rgba = torch.from_numpy(rgba.view(np.int32).reshape(H, W)).cuda()
    d_id = torch.from_numpy(idd).cuda()
    outs = []
    # (VRT_OPT_DISPLAY_KERNEL, scheduling period): 2 / 3 = every wave walks the wave's common rows / every pixel its own box;
    # 0 = each wave the cheaper of the two (shipped)
    kinds = ((2, 0), (3, 0), (0, 0), (2, 16), (3, 16), (0, 16))
    # DENOISE_CHECK: the displayed frame against the oracle's committed hash, where tests/golden/frames.json holds this frame (the oracle
    # itself is run by tests/ only: tests/test_gpu_parity.py compares the display pass with its quad.frag restatement on rendered and synthetic fields)
    want = None
    if os.environ.get("DENOISE_CHECK") and not os.environ.get("DENOISE_SYNTH"):
        for g in json.load(open(os.path.join(root, "tests/golden/frames.json")))["frames"].values():
            if g.get("map") == name and g.get("width") == W and g.get("height") == H and g.get("mode") == 2 and "shown_fnv1a64" in g and \
                    "%016x" % V.fnv1a64(rgba) == g["rgba_fnv1a64"]:
                want = g["shown_fnv1a64"]
    def note(**kw):
        if JSON_PATH:
            kw["pass"] = kw.pop("pass_")
            with open(JSON_PATH, "a") as f:
                f.write(json.dumps(dict(kw, map=name, width=W, height=H, synth=os.environ.get("DENOISE_SYNTH"), checkout=LABEL)) + "\n")

    if HDR:   # the frame as a float image with an HDR range (up to 12), the pass writing both of its outputs
        x = rgba[..., :3].astype(np.float32) / np.float32(255.0)
        d_rgb = torch.from_numpy(np.ascontiguousarray(x * x * np.float32(12.0), np.float32)).cuda()
        houts = []
        for variant, period in kinds:
            ctx.set_denoise_variant(variant)
            ctx.set_tile_scheduling(period)
            d_f = torch.zeros_like(d_rgb)
            d_b = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            call = lambda: ctx.denoise_hdr_device(W, H, d_rgb.data_ptr(), d_id.data_ptr(), d_f.data_ptr(), d_b.data_ptr(), "reinhard", 1.0,
                                                  side.cuda_stream)
            for _ in range(int(os.environ.get("DENOISE_ITERS", 300))):
                call()
            n = int(os.environ.get("DENOISE_ITERS", 100))
            ms = []
            for _ in range(5):   # five windows: their spread is the run-to-run figure
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                for _ in range(n):
                    call()
                e1.record(side)
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / n)
            houts.append((d_f.cpu().numpy().view(np.uint32), d_b.cpu().numpy()))
            print("denoise HDR variant %d scheduling %2d  %s %dx%d  %.4f ms (min %.4f max %.4f)" % (variant, period, name, W, H, float(np.median(ms)), min(ms), max(ms)))
            note(pass_="hdr", variant=variant, scheduling=period, ms_median=float(np.median(ms)), ms_windows=ms, calls_per_window=n)
        print("HDR kinds agree:", all(bool(np.array_equal(houts[0][0], o[0]) and np.array_equal(houts[0][1], o[1])) for o in houts[1:]))
    for variant, period in kinds:   # without, then with feedback tile scheduling
        ctx.set_denoise_variant(variant)
        ctx.set_tile_scheduling(period)
        d_out = torch.zeros_like(d_rgba)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()      # a null stream handle would select the context's own stream
        stream = side.cuda_stream
        for _ in range(int(os.environ.get("DENOISE_ITERS", 300))):   # default: long enough for the clocks to settle
            ctx.denoise_device(W, H, d_rgba.data_ptr(), d_id.data_ptr(), d_out.data_ptr(), stream)
        n = int(os.environ.get("DENOISE_ITERS", 100))
        ms = []
        for _ in range(5 if JSON_PATH else 1):   # with --json five windows: their spread is the run-to-run figure
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            for _ in range(n):
                ctx.denoise_device(W, H, d_rgba.data_ptr(), d_id.data_ptr(), d_out.data_ptr(), stream)
            e1.record(side)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / n)
        outs.append(d_out.cpu().numpy())
        print("denoise variant %d scheduling %2d  %s %dx%d  %.4f ms" % (variant, period, name, W, H, float(np.median(ms))))
        note(pass_="byte", variant=variant, scheduling=period, ms_median=float(np.median(ms)), ms_windows=ms, calls_per_window=n)
    print("variants agree:", all(bool(np.array_equal(outs[0], o)) for o in outs[1:]))
    if want is not None:
        print("equal to the oracle's committed displayed frame:", "%016x" % V.fnv1a64(outs[-1].view(np.uint8).reshape(H, W, 4)) == want)
    elif os.environ.get("DENOISE_CHECK"):
        print("no committed displayed frame for this map / size / pose: kinds compared with each other only")


if __name__ == "__main__":
    main()
