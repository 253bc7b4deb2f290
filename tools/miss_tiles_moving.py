"""Miss tiles (VRT_OPT_MISS_TILES) with a camera that moves. The dispatcher builds a view's mask the second time it sees the view
(one miss_mask_kernel launch before that frame's trace), so three cameras: "static" (one build, then every frame gains),
"moving" (a new view every frame: no mask is ever built, the trace runs as with the option off), and "moving_x2" (every view
traced twice in a row: the second frame of each view builds its mask and uses it -- what a build per view costs against what it
saves). The feedback scheduler runs as in an application (default period). Prints one JSON line per (camera, option) run: the trace
kernel's mean time from hipEvents on its own dispatch packet, and wall time per frame over the whole loop (host enqueue included,
one sync at the end). Run it under `rocprofv3 --kernel-trace --stats` to read the mask kernel's own time beside the trace kernel's.
usage: tools/miss_tiles_moving.py [frames] [map] [width] [height] [mode: primary | primary_shadow] [scheduling period, -1: default]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vrt_import  # noqa: E402

V = vrt_import.vrt()
POSES = {"dragon": (63.5, 60.5, 140.5, -90.0, -10.0), "monu9": (48.5, 60.5, 170.5, -90.0, -12.0),
         "nature": (60.5, 80.5, 200.5, -90.0, -20.0)}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    name = sys.argv[2] if len(sys.argv) > 2 else "dragon"
    W = int(sys.argv[3]) if len(sys.argv) > 3 else 1920
    H = int(sys.argv[4]) if len(sys.argv) > 4 else 1080
    mode = V.MODES[sys.argv[5]] if len(sys.argv) > 5 else V.MODE_PRIMARY
    period = int(sys.argv[6]) if len(sys.argv) > 6 else -1
    w = V.World()
    assert w.load_vox(os.path.join(ROOT, "tests", "golden", "maps", name + ".vox"))
    ctx = V.Context(0)
    ctx.upload_octree(*w.flatten())
    x, y, z, yaw, pitch = POSES[name]
    # a slow orbit around the bench pose: 0.05 degrees and 0.02 units per frame -- every frame a new view (and a new mask)
    path = [V.camera_block((x + 0.02 * k, y, z - 0.01 * k), yaw + 0.05 * k, pitch, W, H)[:3] for k in range(n + 32)]
    moving, warm = path[:n], path[n:]   # the warm-up frames of the moving runs: views the timed loops never show
    static = [moving[0]] * n
    twice = [moving[k // 2] for k in range(n)]
    d_rgba, d_id = ctx.device_alloc(W * H * 4), ctx.device_alloc(W * H * 8)
    if period >= 0:
        ctx.set_tile_scheduling(period)   # 0: row-major starts, no measured tile costs
    try:
        for rep in range(2):
            for cams, cam_name in ((static, "static"), (moving, "moving"), (twice, "moving_x2")):
                for on in (1, 0):
                    ctx.set_option(V.OPT_MISS_TILES, on)
                    for ip, iv, cp in (cams[:32] if cams is static else warm):   # warm-up (views the timed loop does not repeat)
                        ctx.set_camera(ip, iv, cp)
                        ctx.dispatch_rows(W, H, 0, H, mode, d_rgba, d_id)
                    ctx.synchronize()
                    ctx.set_profiling(n)
                    t0 = time.perf_counter()
                    for ip, iv, cp in cams:
                        ctx.set_camera(ip, iv, cp)
                        ctx.dispatch_rows(W, H, 0, H, mode, d_rgba, d_id)
                    ctx.synchronize()
                    wall = (time.perf_counter() - t0) / n
                    k = np.asarray(ctx.profile_read(n), np.float64)
                    ctx.set_profiling(0)
                    print(json.dumps({"map": name, "width": W, "height": H, "mode": mode, "sched_period": period, "camera": cam_name, "miss_tiles": on,
                                      "rep": rep, "frames": n, "trace_kernel_ms_mean": round(float(k.mean()), 5),
                                      "trace_kernel_ms_median": round(float(np.median(k)), 5),
                                      "wall_ms_per_frame": round(wall * 1e3, 5)}), flush=True)
    finally:
        ctx.set_option(V.OPT_MISS_TILES, 1)
        ctx.device_free(d_rgba)
        ctx.device_free(d_id)
        ctx.close()
        w.close()


if __name__ == "__main__":
    main()
