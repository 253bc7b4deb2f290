"""World-query rate on one MI355X: vrt_cast_rays (octree_ray_cast + get_placement_coord per ray) through host buffers and
through device buffers, for batches of 1, 64, 4,096, 65,536 (BASELINE config 1's 256x256 shared-origin frame) and
1,048,576 random rays, on dragon.vox and the config-4 terrain window -- beside vrth_world_ray_cast_many, the same casts on
one host thread. Prints one JSON object per line; --out writes them to a file too.

    python3 tools/query_rate.py --out profiles/query_rate.jsonl
    rocprofv3 --kernel-trace --stats -d <dir> -o q -- python3 tools/query_rate.py --reps 5   (kernel time)
"""
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

BATCHES = (1, 64, 4096, 65536, 1 << 20)


def config1_dirs(V, pos, yaw, pitch, W=256, H=256):
    """the per-pixel directions of a W x H frame from the camera block (what a config-1 loop casts from one origin)"""
    ip, iv, cp, _ = V.camera_block(pos, yaw, pitch, W, H)
    ip = np.asarray(ip, np.float64).reshape(4, 4).T
    iv = np.asarray(iv, np.float64).reshape(4, 4).T
    u = (np.arange(W) + 0.5) / W * 2 - 1
    v = (np.arange(H) + 0.5) / H * 2 - 1
    uu, vv = np.meshgrid(u, v)
    clip = np.stack([uu.ravel(), vv.ravel(), -np.ones(W * H), np.ones(W * H)])
    eye = ip @ clip
    eye[2], eye[3] = -1.0, 0.0
    d = (iv @ eye)[:3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(d, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-rays", type=int, default=65536, help="rays timed on the host loop per scene")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    V = vrt_import.vrt()
    from conftest import terrain_world
    scenes = {}
    w = V.World()
    assert w.load_vox(os.path.join(ROOT, "tests", "golden", "maps", "dragon.vox"))
    scenes["dragon"] = (w, (63.5, 60.5, 140.5), -90.0, -10.0, (0, 0, 0), (128, 128, 128))
    # the pose bench.py renders the terrain window from: the frame looks at the terrain
    scenes["terrain"] = (terrain_world(V), (512.5, 420.5, 1000.5), -90.0, -20.0, (224, 0, 224), (800, 120, 800))
    ctx = V.Context(0)
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    rng = np.random.default_rng(1)
    for name, (w, pos, yaw, pitch, lo, hi) in scenes.items():
        tex, dim = w.flatten()
        ctx.upload_octree(tex, dim)
        frame = config1_dirs(V, pos, yaw, pitch)
        origin = np.asarray(pos, np.float32)
        for n in BATCHES:
            if n == 65536:   # config 1: one origin, the frame's directions
                o, d, form = origin, frame, "shared_origin_256x256"
            else:
                o = rng.uniform(np.asarray(lo) - 64, np.asarray(hi) + 64, (n, 3)).astype(np.float32)
                d = rng.normal(0, 1, (n, 3)).astype(np.float32)
                form = "random"
            ctx.cast_rays(o, d)   # warm-up: code object, scratch buffers
            reps = args.reps if n < (1 << 20) else max(3, args.reps // 4)
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                hit, _, _, _, steps = ctx.cast_rays(o, d)
                t.append(time.perf_counter() - t0)
            med = float(np.median(t))
            # divergence: per wave of 64 rays, the longest ray's steps against the mean
            s = steps[: (len(steps) // 64) * 64].reshape(-1, 64) if len(steps) >= 64 else steps.reshape(1, -1)
            emit({"scene": name, "form": form, "rays": n, "path": "device_host_buffers", "median_ms": round(med * 1e3, 4),
                  "rays_per_s": round(n / med), "hits": int(hit.sum()), "steps_mean": round(float(steps.mean()), 2),
                  "wave_max_over_mean": round(float((s.max(1) / np.maximum(s.mean(1), 1e-9)).mean()), 3), "reps": reps})
        # the host loop: vrth_world_ray_cast_many, one thread, the config-1 frame from its origin
        k = min(args.host_rays, len(frame))
        t0 = time.perf_counter()
        hh, hc = w.ray_cast_many(tuple(map(float, origin)), frame[:k])
        dt = time.perf_counter() - t0
        dev = ctx.cast_rays(origin, frame[:k])
        # rays answered differently: the host tree's hits on leaves with record words 0/0, which the device tree holds as
        # empty space (include/vrt.h; tests/test_gpu_queries.py checks that these are the only differences)
        same = (hh == 1) == dev[0]
        same &= np.where(dev[0], (hc == dev[1]).all(1), True)
        emit({"scene": name, "form": "shared_origin_256x256", "rays": k, "path": "host_ray_cast_many_1_thread",
              "median_ms": round(dt * 1e3, 3), "rays_per_s": round(k / dt), "rays_differing_from_device": int((~same).sum())})
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
