"""Miss tiles (VRT_OPT_MISS_TILES) in an editing loop: a voxel in view is inserted or removed, the edit is patched onto the device
(Context.patch_voxel), and the frame is traced -- with the option on and off, on dragon.vox and the config-4 terrain window at
1080p, primary rays, the bench poses. Two loops per setting:
  every_frame  an edit before every frame: every frame's view key is new (it holds the tree generation), so no mask and no box list
               is ever made -- the option must cost nothing here
  hold_4       an edit, then four frames without one: the second frame after the edit makes the box list and the mask (host walk of
               the records + copy + one kernel), the two after it gain
Prints one JSON line per (map, loop, option): wall time per iteration (edit + patch + frames, one sync at the end) and per frame.
usage: tools/miss_tiles_edit.py [iterations]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vrt_import  # noqa: E402

V = vrt_import.vrt()
POSES = {"dragon": (63.5, 60.5, 140.5, -90.0, -10.0), "terrain": (512.5, 420.5, 1000.5, -90.0, -20.0)}
EDIT_AT = {"dragon": (40, 90, 60), "terrain": (512, 300, 700)}   # empty space both maps' bench views see


def load(name):
    w = V.World()
    if name == "terrain":
        tj = json.load(open(os.path.join(ROOT, "tests", "golden", "terrain.json")))
        wd = tj["window"]
        w.fill_heights(np.load(os.path.join(ROOT, "tests", "golden", "terrain_heights.npz"))["heights"], wd["x0"], wd["z0"], wd["nx"],
                       wd["nz"], tj["band"], tj["floor"])
    else:
        assert w.load_vox(os.path.join(ROOT, "tests", "golden", "maps", name + ".vox"))
    return w


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    W, H = 1920, 1080
    ctx = V.Context(0)
    d_rgba, d_id = ctx.device_alloc(W * H * 4), ctx.device_alloc(W * H * 8)
    try:
        for name in ("dragon", "terrain"):
            w = load(name)
            ctx.upload_octree(*w.flatten())
            p = POSES[name]
            ctx.set_camera(*V.camera_block(p[:3], p[3], p[4], W, H)[:3])
            x, y, z = EDIT_AT[name]
            state = [False]

            def edit():
                if state[0]:
                    w.remove(x, y, z)
                else:
                    w.insert(x, y, z, 0xff3030ff, 3.0, 0.0, 0.0)
                state[0] = not state[0]
                if ctx.patch_voxel(w, x, y, z) is None:
                    ctx.upload_octree(*w.flatten())

            for loop, frames in (("every_frame", 1), ("hold_4", 4)):
                for rep in range(2):
                    for on in (1, 0):
                        ctx.set_option(V.OPT_MISS_TILES, on)
                        for _ in range(4):   # warm-up
                            edit()
                            for _ in range(frames):
                                ctx.dispatch_rows(W, H, 0, H, V.MODE_PRIMARY, d_rgba, d_id)
                        ctx.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(iters):
                            edit()
                            for _ in range(frames):
                                ctx.dispatch_rows(W, H, 0, H, V.MODE_PRIMARY, d_rgba, d_id)
                        ctx.synchronize()
                        dt = (time.perf_counter() - t0) / iters
                        print(json.dumps({"map": name, "loop": loop, "miss_tiles": on, "rep": rep, "iterations": iters,
                                          "ms_per_iteration": round(dt * 1e3, 4), "ms_per_frame": round(dt * 1e3 / frames, 4)}),
                              flush=True)
            w.close()
    finally:
        ctx.set_option(V.OPT_MISS_TILES, 1)
        ctx.device_free(d_rgba)
        ctx.device_free(d_id)
        ctx.close()


if __name__ == "__main__":
    main()
