"""Miss tiles (VRT_OPT_MISS_TILES), a CPU model of what a mask is worth: no GPU, the oracle and the host library only. For a map, pose
and frame size it prints one JSON line with
  * mask_cleared: the fraction of 8 x 8 tiles the host mask (vrt_test_miss_mask: the mask the dispatcher hands the kernel) clears;
  * oracle_all_miss: the fraction of tiles whose every pixel is a miss in the oracle's frame -- what a perfect mask would clear;
  * wave_cost: a proxy for the marched work that is left. A wave is a tile and lasts as long as its longest lane, so a tile costs
    the maximum of the oracle's per-pixel fetch counts over its pixels; the figure is the sum of that over the tiles the mask
    traces, over the same sum with no mask. It is a model, not a measurement: it prices neither the prologue nor the stores.
usage: tests/fuzz/miss_tiles_model.py [map | all] [width height] [x y z yaw pitch]      (defaults: the bench poses and frame sizes)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import vrt_import  # noqa: E402
import oracle_py as O  # noqa: E402

V = vrt_import.vrt()
GOLDEN = os.path.join(ROOT, "tests", "golden")
BENCH = {  # bench.py POSES and the BASELINE configurations' frame sizes
    "dragon": ((63.5, 60.5, 140.5, -90.0, -10.0), 1920, 1080),
    "monu9": ((48.5, 60.5, 170.5, -90.0, -12.0), 1280, 720),
    "nature": ((60.5, 80.5, 200.5, -90.0, -20.0), 3840, 2160),
    "terrain": ((512.5, 420.5, 1000.5, -90.0, -20.0), 1920, 1080),
}


def world(name):
    w = V.World()
    if name == "terrain":   # BASELINE config 4: tests/golden/terrain.json over terrain_heights.npz
        t = json.load(open(os.path.join(GOLDEN, "terrain.json")))
        wd = t["window"]
        w.fill_heights(np.load(os.path.join(GOLDEN, "terrain_heights.npz"))["heights"], wd["x0"], wd["z0"], wd["nx"], wd["nz"],
                       t["band"], t["floor"])
    else:
        assert w.load_vox(os.path.join(GOLDEN, "maps", name + ".vox")), name
    return w


def tiles(a, fn):
    """a per-pixel (H, W) array -> fn over each 8 x 8 tile (frame edges: part tiles)"""
    H, W = a.shape
    th, tw = (H + 7) // 8, (W + 7) // 8
    p = np.zeros((th * 8, tw * 8), a.dtype)
    p[:H, :W] = a
    return fn(p.reshape(th, 8, tw, 8), axis=(1, 3))


def model(name, pose, W, H):
    w = world(name)
    tex, dim = w.flatten()
    w.close()
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    _, idd, fetch, _ = O.render(O.make_scene(tex, dim, ip, iv, cp), W, H, 0, want_fetch_map=True)
    hit = np.asarray(idd).reshape(H, W, 2)[..., 0] != 0
    cost = tiles(fetch.astype(np.float64), np.max)
    all_miss = tiles(hit, np.max) == 0
    out = {"map": name, "pose": list(pose), "width": W, "height": H, "tiles": int(cost.size),
           "oracle_all_miss": round(float(all_miss.mean()), 4)}
    r = V.miss_mask(tex, ip, iv, cp, W, H)
    if r is None:
        out.update(mask="none", mask_cleared=0.0, wave_cost=1.0)
    else:
        mask, boxes, whole = r
        assert not (all_miss[mask == 0] == 0).any(), "the mask clears a tile with a hit"
        out.update(boxes=boxes, whole_view=whole, mask_cleared=round(float((mask == 0).mean()), 4),
                   wave_cost=round(float(cost[mask != 0].sum() / cost.sum()), 4),
                   wave_cost_perfect_mask=round(float(cost[~all_miss].sum() / cost.sum()), 4))
    print(json.dumps(out), flush=True)


def main():
    a = sys.argv[1:]
    names = list(BENCH) if not a or a[0] == "all" else [a[0]]
    for name in names:
        pose, W, H = BENCH[name]
        if len(a) >= 3:
            W, H = int(a[1]), int(a[2])
        if len(a) >= 8:
            pose = tuple(float(v) for v in a[3:8])
        model(name, pose, W, H)


if __name__ == "__main__":
    main()
