"""Rate of vrt_shade_rays_device on one MI355X, kernel time from the events attached to each launch (vrt_set_profiling):
  (a) the 1080p dragon frame's rays as a batch (width 1920), each mode, alternated launch by launch with the frame kernel of the
      same frame and mode -- the same work with every per-view shortcut available (ray tables, the shared eye lookup, the
      tightened root, the empty-space march loop, miss tiles, tile scheduling). The frame kernels are the parent commit's,
      unchanged. The batch's rays are made here in numpy, so they are the frame's rays up to rounding, not bit for bit.
  (b) 2 M random incoherent rays through the dragon, each mode.
  (c) 2 M probe rays: origins in the cells in front of surfaces, cosine-distributed directions about the face normal, mode 2,
      n_samples 1 and 16.
--hdr measures vrt_shade_rays_hdr_device instead (float mean, tone-mapped bytes and id_dist written, no d_sums), alternated launch
by launch with the plain vrt_shade_rays_device call of the same build on the same rays: each mode, 1 and 16 samples, on the 1080p
dragon frame's rays and on a list of 1 M random rays.
Prints one JSON object per line; --out writes them to a file too.

    python3 tools/shade_rays_rate.py --out profiles/shade_rays_rate.jsonl
    python3 tools/shade_rays_rate.py --hdr --out profiles/shade_rays_hdr_rate.jsonl

--path-depth D [D ...] measures mode 2 of (a)'s batch and of (c)'s probes once per path depth (vrt_set_path_depth) instead:

    python3 tools/shade_rays_rate.py --path-depth 1 2 4 8 --append --out profiles/path_depth_rate.jsonl   (after tools/accum_rate.py's rows)

--sun R [R ...] (with --path-depth) measures each of them once per sun disc too (vrt_set_sun_disc) and records it (sun_disc):

    python3 tools/shade_rays_rate.py --path-depth 1 4 --sun 0 0.00465 0.05 --append --out profiles/sun_disc_rate.jsonl

--emit E [E ...] (with --path-depth) measures them in tests/emit_worlds.py's lamp room instead of the dragon (which has no emitter),
once per setting of emitter sampling (vrt_set_emitter_sampling, 0 or 1), and records it (emitter_sampling):

    python3 tools/shade_rays_rate.py --path-depth 1 4 --emit 0 1 --append --out profiles/emit_rate.jsonl

--emit-power M [M ...] (with --emit) measures sampling on once per importance mode too (vrt_set_emitter_importance, 0 uniform or 1
power) and records it (emitter_importance); --emit-world power_room takes tests/emit_power_worlds.py's room (a merged lamp of size 4
and 256 dim singles) instead of the lamp room:

    python3 tools/shade_rays_rate.py --path-depth 1 4 --emit 0 1 --emit-power 0 1 --emit-world power_room --append --out profiles/emit_power_rate.jsonl

--emit-mis F [F ...] (with --emit-power) measures sampling on at mode 1 once per value of the MIS flag too (vrt_set_emitter_mis, 0 or
1) and records it (emitter_mis); --emit-world mis_room takes tests/emit_mis_worlds.py's room, the frame's rays from its INSIDE_POSE:

    python3 tools/shade_rays_rate.py --path-depth 1 4 --emit 0 1 --emit-power 1 --emit-mis 0 1 --emit-world mis_room --append --out profiles/emit_mis_rate.jsonl

--guides measures vrt_guide_rays_device (all four outputs written) alternated call by call with vrt_shade_rays_device in
VRT_MODE_PRIMARY on the same rays -- the same march with its shading on top -- on the 1080p dragon frame's rays and on a list of
1 M random rays; wall time around each call and a synchronise (the guide launches take no profiling slot):

    python3 tools/shade_rays_rate.py --guides --append --out profiles/guides_rate.jsonl   (after tools/accum_rate.py --guides)

--glass (with --guides) measures in the lamp room of tests/emit_worlds.py instead, on 1 M rays from its eye and on 1 M rays from random
origins inside it, and alternates a third call with them: vrt_guide_rays_device with guides past glass on (vrt_set_guide_glass, read
at the call): glass_guide_call_ms, glass_over_plain.

    python3 tools/shade_rays_rate.py --guides --glass --append --out profiles/guides_glass_rate.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vrt_import  # noqa: E402

POSE = ((63.5, 60.5, 140.5), -90.0, -10.0)   # the golden 1080p dragon frame


def frame_rays(V, W, H, pose=POSE):
    """comp:624-641 in float64, rounded to float32 at the end"""
    ip, iv, cp, _ = V.camera_block(pose[0], pose[1], pose[2], W, H)
    ipm = np.asarray(ip, np.float64).reshape(4, 4).T
    ivm = np.asarray(iv, np.float64).reshape(4, 4).T
    u = np.arange(W) / W * 2 - 1
    v = np.arange(H) / H * 2 - 1
    uu, vv = np.meshgrid(u, v)
    view = ipm @ np.stack([uu.ravel(), vv.ravel(), -np.ones(W * H), np.ones(W * H)])
    view = view[:3] / view[3]
    view /= np.linalg.norm(view, axis=0, keepdims=True)
    d = (ivm[:3, :3] @ view).T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (ip, iv, cp), np.asarray(cp[:3], np.float32), np.ascontiguousarray(d, np.float32)


def cosine_dirs(rng, normals):
    n = len(normals)
    r1, r2 = rng.random(n), rng.random(n)
    phi = 2 * np.pi * r2
    x, z, y = np.sqrt(1 - r1) * np.cos(phi), np.sqrt(1 - r1) * np.sin(phi), np.sqrt(r1)
    up = np.where(np.abs(normals[:, 2:3]) < 0.999, np.array([[0.0, 0.0, 1.0]]), np.array([[1.0, 0.0, 0.0]]))
    t = np.cross(up, normals)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(normals, t)
    return np.ascontiguousarray(t * x[:, None] + b * z[:, None] + normals * y[:, None], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rays", type=int, default=1 << 21)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hdr", action="store_true", help="the HDR calls beside the plain ones (see above)")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--guides", action="store_true", help="vrt_guide_rays_device beside mode-0 vrt_shade_rays_device (see above)")
    ap.add_argument("--glass", action="store_true", help="with --guides: in the lamp room, guides past glass beside the plain ones (see above)")
    ap.add_argument("--path-depth", nargs="+", type=int, default=None, metavar="D", help="mode 2 once per path depth (see above)")
    ap.add_argument("--sun", nargs="+", type=float, default=None, metavar="R", help="with --path-depth: once per sun disc (vrt_set_sun_disc)")
    ap.add_argument("--emit", nargs="+", type=int, default=None, choices=(0, 1), metavar="E",
                    help="with --path-depth: in the lamp room, once per setting of emitter sampling (vrt_set_emitter_sampling)")
    ap.add_argument("--emit-power", nargs="+", type=int, default=None, choices=(0, 1), metavar="M",
                    help="with --emit: sampling on once per importance mode (vrt_set_emitter_importance)")
    ap.add_argument("--emit-mis", nargs="+", type=int, default=None, choices=(0, 1), metavar="F",
                    help="with --emit-power: sampling on at mode 1 once per MIS flag (vrt_set_emitter_mis)")
    ap.add_argument("--emit-world", default="lamp_room", choices=("lamp_room", "power_room", "mis_room"), help="with --emit: the world")
    args = ap.parse_args()
    if args.emit_mis and not args.emit_power:
        ap.error("--emit-mis goes with --emit-power")
    if args.emit_power and not args.emit:
        ap.error("--emit-power goes with --emit")
    if args.sun and not args.path_depth:
        ap.error("--sun goes with --path-depth")
    if args.emit and not args.path_depth:
        ap.error("--emit goes with --path-depth")
    if args.glass and not args.guides:
        ap.error("--glass goes with --guides")
    V = vrt_import.vrt()
    if args.glass:
        import emit_worlds
        w = emit_worlds.lamp_room(V)
    elif args.emit:
        import emit_worlds
        if args.emit_world == "power_room":
            import emit_power_worlds
            w = emit_power_worlds.room(V)
        elif args.emit_world == "mis_room":
            import emit_mis_worlds
            w = emit_mis_worlds.room(V)
        else:
            w = emit_worlds.lamp_room(V)
    else:
        w = V.World()
        assert w.load_vox(os.path.join(ROOT, "tests", "golden", "maps", "dragon.vox"))
    ctx = V.Context(0)
    ctx.upload_octree(*w.flatten())
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    def upload(o, d):
        d_o, d_d = ctx.device_alloc(o.nbytes), ctx.device_alloc(d.nbytes)
        ctx.device_write(d_o, o)
        ctx.device_write(d_d, d)
        return d_o, d_d

    def timed(launches, reps):
        """launches: callables, run in turn `reps` times with per-launch events -> one array of kernel ms per callable"""
        for f in launches:   # warm-up: code objects, scratch
            f()
        ctx.synchronize()
        ctx.set_profiling(len(launches) * reps)
        for _ in range(reps):
            for f in launches:
                f()
        ms = ctx.profile_read(len(launches) * reps)
        ctx.set_profiling(0)
        assert len(ms) == len(launches) * reps, "a launch was not timed"
        return [ms[i::len(launches)] for i in range(len(launches))]

    def finish():
        ctx.close()
        if args.out:
            with open(args.out, "a" if args.append else "w") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")

    if args.guides:
        import time
        W, H = 1920, 1080
        _, origin, dirs = frame_rays(V, W, H)
        rng = np.random.default_rng(1)
        n_list = 1 << 20
        lo = rng.uniform((-64, -64, -64), (192, 160, 128), (n_list, 3)).astype(np.float32)
        ld = rng.normal(0, 1, (n_list, 3)).astype(np.float32)
        cases = (("frame_rays_1080p_dragon", origin.reshape(1, 3), dirs, 0, W), ("random_rays_1m_dragon", lo, ld, 3, n_list))
        if args.glass:
            eye = np.array(emit_worlds.EYE, np.float32).reshape(1, 3)
            inside = rng.uniform((emit_worlds.LO + 1,) * 3, (emit_worlds.HI,) * 3, (n_list, 3)).astype(np.float32)
            cases = (("eye_rays_1m_lamp_room", eye, ld, 0, n_list), ("random_rays_1m_lamp_room", inside, ld, 3, n_list))

        def guide_call(glass, n, d_o, stride, d_d, outs, width):
            ctx.set_guide_glass(glass)
            ctx.guide_rays_device(n, d_o, stride, d_d, *outs, width=width)

        for case, o, d, stride, width in cases:
            n = len(d)
            d_o, d_d = upload(o, d)
            d_rgba, d_id = ctx.device_alloc(n * 4), ctx.device_alloc(n * 8)
            d_n, d_a, d_z, d_h = ctx.device_alloc(n * 12), ctx.device_alloc(n * 16), ctx.device_alloc(n * 4), ctx.device_alloc(n)
            calls = [lambda: ctx.shade_rays_device(n, d_o, stride, d_d, d_rgba, d_id, mode=0, width=width),
                     lambda: guide_call(False, n, d_o, stride, d_d, (d_n, d_a, d_z, d_h), width)]
            if args.glass:
                calls.append(lambda: guide_call(True, n, d_o, stride, d_d, (d_n, d_a, d_z, d_h), width))
            ms = [[] for _ in calls]
            for rep in range(args.reps + 2):   # the first two rounds: code objects
                for i, f in enumerate(calls):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    f()
                    ctx.synchronize()
                    if rep >= 2:
                        ms[i].append((time.perf_counter() - t0) * 1e3)
            pm, gm = float(np.median(ms[0])), float(np.median(ms[1]))
            row = {"case": case, "rays": n, "primary_call_ms": round(pm, 4), "guide_call_ms": round(gm, 4), "guide_over_primary": round(gm / pm, 3),
                   "primary_ms_min_max": [round(min(ms[0]), 4), round(max(ms[0]), 4)], "guide_ms_min_max": [round(min(ms[1]), 4), round(max(ms[1]), 4)],
                   "guide_rays_per_s": round(n / (gm * 1e-3)), "reps": args.reps}
            if args.glass:
                xm = float(np.median(ms[2]))
                row.update(glass_guide_call_ms=round(xm, 4), glass_ms_min_max=[round(min(ms[2]), 4), round(max(ms[2]), 4)],
                           glass_over_plain=round(xm / gm, 3))
            emit(row)
            ctx.set_guide_glass(False)
            for p in (d_o, d_d, d_rgba, d_id, d_n, d_a, d_z, d_h):
                ctx.device_free(p)
        finish()
        return

    if args.hdr:
        W, H = 1920, 1080
        _, origin, dirs = frame_rays(V, W, H)
        rng = np.random.default_rng(1)
        n_list = 1 << 20
        lo = rng.uniform((-64, -64, -64), (192, 160, 128), (n_list, 3)).astype(np.float32)
        ld = rng.normal(0, 1, (n_list, 3)).astype(np.float32)
        for case, o, d, stride, width in (("frame_rays_1080p_dragon", origin.reshape(1, 3), dirs, 0, W),
                                          ("random_rays_1m_dragon", lo, ld, 3, n_list)):
            n = len(d)
            d_o, d_d = upload(o, d)
            d_rgb, d_rgba, d_id = ctx.device_alloc(n * 12), ctx.device_alloc(n * 4), ctx.device_alloc(n * 8)
            for mode in (0, 1, 2):
                for n_samples in (1, 16):
                    reps = args.reps if n_samples == 1 or mode != 2 else max(3, args.reps // 4)
                    plain, hdr = timed([lambda: ctx.shade_rays_device(n, d_o, stride, d_d, d_rgba, d_id, mode=mode, width=width,
                                                                      n_samples=n_samples),
                                        lambda: ctx.shade_rays_hdr_device(n, d_o, stride, d_d, d_rgb, d_rgba, d_id, mode=mode, width=width,
                                                                          n_samples=n_samples, tonemap="reinhard")], reps)
                    pm, hm = float(np.median(plain)), float(np.median(hdr))
                    emit({"case": case, "mode": mode, "rays": n, "n_samples": n_samples, "plain_kernel_ms": round(pm, 4),
                          "hdr_kernel_ms": round(hm, 4), "hdr_over_plain": round(hm / pm, 3),
                          "plain_ms_min_max": [round(float(plain.min()), 4), round(float(plain.max()), 4)],
                          "hdr_ms_min_max": [round(float(hdr.min()), 4), round(float(hdr.max()), 4)],
                          "hdr_rays_per_s": round(n / (hm * 1e-3)), "reps": reps})
            for p in (d_o, d_d, d_rgb, d_rgba, d_id):
                ctx.device_free(p)
        finish()
        return

    if args.path_depth:
        W, H = 1920, 1080
        world = "dragon"
        box = ((-64, -64, -64), (192, 160, 128))
        pose = POSE
        if args.emit:   # the probes start inside the room
            world = args.emit_world
            box = ((emit_worlds.LO + 1,) * 3, (emit_worlds.HI,) * 3)
            pose = (emit_worlds.POSE[:3], emit_worlds.POSE[3], emit_worlds.POSE[4])
            if args.emit_world == "mis_room":
                pose = (emit_mis_worlds.INSIDE_POSE[:3], emit_mis_worlds.INSIDE_POSE[3], emit_mis_worlds.INSIDE_POSE[4])
        _, origin, dirs = frame_rays(V, W, H, pose)
        rng = np.random.default_rng(1)
        n_probe = args.rays
        o = rng.uniform(box[0], box[1], (n_probe, 3)).astype(np.float32)
        d = rng.normal(0, 1, (n_probe, 3)).astype(np.float32)
        hit, coord, place, _, _ = ctx.cast_rays(o, d)
        face = (place - coord)[hit].astype(np.float64)
        ok = np.abs(face).sum(1) == 1
        cells, normals = place[hit][ok], face[ok]
        pick = rng.integers(0, len(cells), n_probe)
        po = (cells[pick] + rng.random((n_probe, 3))).astype(np.float32)
        pd = cosine_dirs(rng, normals[pick])
        for case, ro, rd, stride, width in ((f"frame_rays_1080p_{world}", origin.reshape(1, 3), dirs, 0, W),
                                            (f"probe_rays_{world}", po, pd, 3, n_probe)):
            n = len(rd)
            d_o, d_d = upload(ro, rd)
            d_rgba, d_id = ctx.device_alloc(n * 4), ctx.device_alloc(n * 8)
            for depth, sun, em, imp, mis in [(dd, r, e, m, f) for dd in args.path_depth for r in (args.sun or [None]) for e in (args.emit or [None])
                                             for m in ((args.emit_power if e else args.emit_power[:1]) if args.emit_power else [None])
                                             for f in ((args.emit_mis if e and m == 1 else args.emit_mis[:1]) if args.emit_mis else [None])]:
                ctx.set_path_depth(depth)
                if sun is not None:
                    ctx.set_sun_disc(sun)
                if em is not None:
                    ctx.set_emitter_sampling(em)
                if imp is not None:
                    ctx.set_emitter_importance(imp if em else 0)
                if mis is not None:
                    ctx.set_emitter_mis(mis if em and imp == 1 else 0)
                for n_samples in (1, 4):
                    (ms,) = timed([lambda: ctx.shade_rays_device(n, d_o, stride, d_d, d_rgba, d_id, mode=2, width=width, n_samples=n_samples)],
                                  max(3, args.reps // 2))
                    m = float(np.median(ms))
                    emit({"case": case, "mode": 2, "path_depth": depth, **({} if sun is None else {"sun_disc": sun}),
                          **({} if em is None else {"emitter_sampling": em}),
                          **({"emitter_importance": imp} if imp is not None and em else {}),
                          **({"emitter_mis": mis} if mis is not None and em and imp == 1 else {}), "rays": n, "n_samples": n_samples, "batch_kernel_ms": round(m, 4),
                          "kernel_ms_min_max": [round(float(ms.min()), 4), round(float(ms.max()), 4)],
                          "per_sample_ms": round(m / n_samples, 4), "paths_per_s": round(n * n_samples / (m * 1e-3)), "reps": len(ms)})
            for p in (d_o, d_d, d_rgba, d_id):
                ctx.device_free(p)
        finish()
        return

    # (a) the frame's rays against the frame kernel
    W, H = 1920, 1080
    cam, origin, dirs = frame_rays(V, W, H)
    ctx.set_camera(*cam)
    n = W * H
    d_o, d_d = upload(origin.reshape(1, 3), dirs)
    d_rgba, d_id = ctx.device_alloc(n * 4), ctx.device_alloc(n * 8)
    for mode in (0, 1, 2):
        for _ in range(40):   # let the frame kernel's scheduler and miss mask settle, as in a frame loop
            ctx.dispatch_rows(W, H, 0, H, mode, d_rgba, d_id)
        frame, batch = timed([lambda: ctx.dispatch_rows(W, H, 0, H, mode, d_rgba, d_id),
                              lambda: ctx.shade_rays_device(n, d_o, 0, d_d, d_rgba, d_id, mode=mode, width=W)], args.reps)
        fm, bm = float(np.median(frame)), float(np.median(batch))
        emit({"case": "a_frame_rays_1080p_dragon", "mode": mode, "rays": n, "frame_kernel_ms": round(fm, 4), "batch_kernel_ms": round(bm, 4),
              "batch_over_frame": round(bm / fm, 3), "batch_rays_per_s": round(n / (bm * 1e-3)), "reps": args.reps})
    for p in (d_o, d_d, d_rgba, d_id):
        ctx.device_free(p)

    # (b) random incoherent rays
    rng = np.random.default_rng(1)
    n = args.rays
    o = rng.uniform((-64, -64, -64), (192, 160, 128), (n, 3)).astype(np.float32)
    d = rng.normal(0, 1, (n, 3)).astype(np.float32)
    d_o, d_d = upload(o, d)
    d_rgba, d_id = ctx.device_alloc(n * 4), ctx.device_alloc(n * 8)
    for mode in (0, 1, 2):
        (ms,) = timed([lambda: ctx.shade_rays_device(n, d_o, 3, d_d, d_rgba, d_id, mode=mode, width=n)], max(3, args.reps // 2))
        m = float(np.median(ms))
        emit({"case": "b_random_rays_dragon", "mode": mode, "rays": n, "batch_kernel_ms": round(m, 4), "batch_rays_per_s": round(n / (m * 1e-3))})

    # (c) probes: from the cell in front of a hit surface, cosine-distributed about its normal
    hit, coord, place, _, _ = ctx.cast_rays(o, d)
    face = (place - coord)[hit].astype(np.float64)
    ok = np.abs(face).sum(1) == 1   # unit voxels: the placement cell is a face neighbour
    cells, normals = place[hit][ok], face[ok]
    pick = rng.integers(0, len(cells), n)
    po = (cells[pick] + rng.random((n, 3))).astype(np.float32)
    pd = cosine_dirs(rng, normals[pick])
    ctx.device_write(d_o, po)
    ctx.device_write(d_d, pd)
    for n_samples in (1, 16):
        (ms,) = timed([lambda: ctx.shade_rays_device(n, d_o, 3, d_d, d_rgba, d_id, mode=2, width=n, n_samples=n_samples)], max(3, args.reps // 4))
        m = float(np.median(ms))
        emit({"case": "c_probe_rays_dragon", "mode": 2, "rays": n, "n_samples": n_samples, "surfaces": int(len(cells)),
              "batch_kernel_ms": round(m, 4), "paths_per_s": round(n * n_samples / (m * 1e-3))})
    for p in (d_o, d_d, d_rgba, d_id):
        ctx.device_free(p)
    finish()


if __name__ == "__main__":
    main()
