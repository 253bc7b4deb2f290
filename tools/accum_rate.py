"""Progressive-accumulation rate on one MI355X: wall time of one vrt_accum_add of n samples (n = 1, 4, 16, 64; the adds after
the first, i.e. without pass 1 on the opaque path) on the 1080p dragon and nature frames and the 1080p room from inside, beside
n times the frame time of vrt_dispatch in the same mode (vrt_dispatch_timed: events around each launch). --mode picks the modes
(default: full), --jitter accumulates jittered samples (VRT_ACCUM_JITTER). --lens APERTURE FOCUS (repeatable) adds the same
accumulation with that thin lens (vrt_set_lens) beside it, with the side of the dispatcher's one-eye proofs the lens takes
(shared: one eye lookup and one first lookup for every origin; per_lane: either made per lane) and its cost over the lens-free one. Prints one JSON object per line; --out
writes them to a file too.

    python3 tools/accum_rate.py --out profiles/accum_rate.jsonl
    python3 tools/accum_rate.py --mode primary primary_shadow full --jitter --out profiles/accum_jitter_rate.jsonl
    python3 tools/accum_rate.py --mode primary primary_shadow full --jitter --lens 0.1 40 --lens 10 40 --out profiles/accum_lens_rate.jsonl
    rocprofv3 --kernel-trace --stats -d <dir> -o a -- python3 tools/accum_rate.py --reps 3   (kernel times)

--adaptive MIN MAX TOL measures adaptive accumulations (vrt_accum_begin_adaptive) instead: on each scene, primary + jitter, full,
and full + jitter + a thin lens (--adaptive-lens, default 0.1 40), `--rounds` adds of one round each, and for every add its wall
time, the fraction of pixels still active after it (vrt_accum_counts) and its ratio to the add of the same round of the plain
accumulation (the median of --reps runs of each).

    python3 tools/accum_rate.py --adaptive 4 64 24 --out profiles/accum_adaptive_rate.jsonl

--hdr measures every accumulation a second time as an HDR accumulation (vrt_accum_keep_hdr: float64 sums of the samples' float
colours beside the integer sums) and records its add time and ratio beside the plain one (hdr_add_ms, hdr_vs_plain), and the
time of one vrt_accum_resolve_hdr_device beside vrt_accum_resolve_device (resolve_ms, hdr_resolve_ms).

    python3 tools/accum_rate.py --hdr --out profiles/accum_hdr_rate.jsonl
    python3 tools/accum_rate.py --hdr --mode primary primary_shadow full --jitter --out profiles/accum_hdr_jitter_rate.jsonl

--path-depth D [D ...] measures every accumulation once per path depth (vrt_set_path_depth; VRT_MODE_FULL only honours it) and
records the depth and the time per sample (path_depth, per_sample_ms); --scenes and --samples restrict the scenes and the sample
counts of an add.

    python3 tools/accum_rate.py --path-depth 1 2 4 8 --scenes dragon_1080p room_inside_1080p --out profiles/path_depth_rate.jsonl

--sun R [R ...] (with --path-depth) measures each of them once per sun disc too (vrt_set_sun_disc, tan_radius R; 0 is the point sun)
and records it (sun_disc):

    python3 tools/accum_rate.py --path-depth 1 4 --sun 0 0.00465 0.05 --scenes dragon_1080p room_inside_1080p --out profiles/sun_disc_rate.jsonl

--emit E [E ...] (with --path-depth) measures each of them once per setting of emitter sampling too (vrt_set_emitter_sampling, 0 or
1) and records it (emitter_sampling, and the length of the list: emitters). The scene lamp_room_1080p is tests/emit_worlds.py's
lamp room seen from inside, which has emitters; the room fixture and the maps have none, so their two settings launch the same
kernels:

    python3 tools/accum_rate.py --path-depth 1 4 --emit 0 1 --scenes lamp_room_1080p room_inside_1080p --samples 16 --out profiles/emit_rate.jsonl

--emit-power M [M ...] (with --emit) measures each setting with sampling on once per importance mode too (vrt_set_emitter_importance, 0
uniform or 1 power) and records it (emitter_importance); with sampling off the mode is not read and the row is measured once. The
scene power_room_1080p is tests/emit_power_worlds.py's room seen from inside: a merged lamp of size 4 and 256 dim singles:

    python3 tools/accum_rate.py --path-depth 1 4 --emit 0 1 --emit-power 0 1 --scenes power_room_1080p lamp_room_1080p --samples 16 --out profiles/emit_power_rate.jsonl

--emit-mis F [F ...] (with --emit-power) measures each setting with sampling on and mode 1 once per value of the MIS flag too
(vrt_set_emitter_mis, 0 or 1) and records it (emitter_mis); elsewhere the flag is not read and the row is measured once. The scene
mis_room_1080p is tests/emit_mis_worlds.py's room seen from inside, looking at the foot of the lamp on the floor:

    python3 tools/accum_rate.py --path-depth 1 4 --emit 0 1 --emit-power 1 --emit-mis 0 1 --scenes mis_room_1080p power_room_1080p --samples 16 --out profiles/emit_mis_rate.jsonl

--variant V (with --path-depth) measures with vrt_set_variant(V) and records it (variant); 1 takes the record-array kernels.

--guides measures the guide planes (vrt_accum_guides_device) instead: on each scene of --scenes, from the corner, jittered and through a
thin lens (the first --lens, default 0.1 40), the wall time of one guide call that catches up --samples new samples (guide_ms: the
guide kernel over them plus the resolve), of a call with nothing new (resolve_ms: the resolve alone), the guide time per sample
between them (guide_per_sample_ms), and beside it one vrt_accum_add of as many samples of VRT_MODE_PRIMARY from the same source
(primary_add_ms, primary_per_sample_ms: the same march with its shading; the corner's is the repeat path, which marches nothing):

    python3 tools/accum_rate.py --guides --scenes dragon_1080p room_inside_1080p --samples 16 --out profiles/guides_rate.jsonl

--glass (with --guides) measures every row twice in the same process, with guides past glass off and on (vrt_set_guide_glass, read by
the begin; "glass": false / true in the row), the plain form first:

    python3 tools/accum_rate.py --guides --glass --scenes room_inside_1080p lamp_room_1080p --samples 16 --out profiles/guides_glass_rate.jsonl

--moments measures accumulations that keep luminance moments (vrt_accum_keep_moments) beside the same HDR accumulations without, in
the same process: on each scene of --scenes, VRT_MODE_FULL at each --path-depth (default 1), from the corner and jittered, the wall time
of one add of --samples samples each way, alternated (hdr_add_ms, moments_add_ms, their per-sample times and ratio), of one
vrt_accum_variance_device (variance_ms), and of one vrt_accum_resolve_hdr_filtered_var_device at the defaults on the accumulation
without moments (the spatial estimate) and with (the measured plane): filtered_var_spatial_ms, filtered_var_moments_ms.

    python3 tools/accum_rate.py --moments --path-depth 1 4 --scenes dragon_1080p room_inside_1080p --samples 16 --out profiles/moments_rate.jsonl

--out replaces the file: tools/shade_rays_rate.py --path-depth ... --append adds the ray batches' rows to it, so it runs second.
--adaptive takes none of --path-depth, --scenes and --samples (it measures its own scenes and rounds) and refuses them.
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

SAMPLES = (1, 4, 16, 64)
SCENES = {   # name -> (map, pose): the golden 1080p / 4K frames' poses
    "dragon_1080p": ("dragon", (63.5, 60.5, 140.5), -90.0, -10.0),
    "nature_1080p": ("nature", (60.5, 80.5, 200.5), -90.0, -20.0),
    "room_inside_1080p": ("room", (14.5, 30.5, 16.5), 32.0, -10.0),
    "lamp_room_1080p": ("lamp", (36.5, 44.5, 50.5), -38.0, 8.0),   # tests/emit_worlds.py: POSE
    "power_room_1080p": ("power", (36.5, 44.5, 50.5), -38.0, 8.0),   # tests/emit_power_worlds.py: POSE
    "mis_room_1080p": ("mis", (36.5, 44.5, 50.5), -20.0, -35.0),   # tests/emit_mis_worlds.py: INSIDE_POSE
}
DEFAULT_SCENES = sorted(s for s in SCENES if SCENES[s][0] not in ("lamp", "power", "mis"))   # the lamp rooms: on request (--scenes), for --emit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--mode", nargs="+", default=["full"], choices=["primary", "primary_shadow", "full"])
    ap.add_argument("--jitter", action="store_true", help="jittered samples (anti-aliasing)")
    ap.add_argument("--lens", nargs=2, type=float, action="append", default=[], metavar=("APERTURE", "FOCUS"),
                    help="also with this thin lens (repeatable)")
    ap.add_argument("--adaptive", nargs=3, type=int, metavar=("MIN", "MAX", "TOL"), help="adaptive accumulations (see above)")
    ap.add_argument("--adaptive-lens", nargs=2, type=float, default=(0.1, 40.0), metavar=("APERTURE", "FOCUS"))
    ap.add_argument("--rounds", type=int, default=32)
    ap.add_argument("--hdr", action="store_true", help="each accumulation again with HDR sums, beside the plain one")
    ap.add_argument("--path-depth", nargs="+", type=int, default=None, metavar="D", help="once per path depth (vrt_set_path_depth)")
    ap.add_argument("--sun", nargs="+", type=float, default=None, metavar="R", help="with --path-depth: once per sun disc (vrt_set_sun_disc)")
    ap.add_argument("--emit", nargs="+", type=int, default=None, choices=(0, 1), metavar="E",
                    help="with --path-depth: once per setting of emitter sampling (vrt_set_emitter_sampling)")
    ap.add_argument("--emit-power", nargs="+", type=int, default=None, choices=(0, 1), metavar="M",
                    help="with --emit: sampling on once per importance mode (vrt_set_emitter_importance)")
    ap.add_argument("--emit-mis", nargs="+", type=int, default=None, choices=(0, 1), metavar="F",
                    help="with --emit-power: sampling on at mode 1 once per MIS flag (vrt_set_emitter_mis)")
    ap.add_argument("--variant", type=int, default=None, metavar="V",
                    help="with --path-depth: the traversal variant (vrt_set_variant; 1: the record-array kernels), recorded as variant")
    ap.add_argument("--guides", action="store_true", help="the guide planes beside primary-mode adds (see above)")
    ap.add_argument("--glass", action="store_true", help="with --guides: each row with guides past glass off and on (see above)")
    ap.add_argument("--moments", action="store_true", help="HDR accumulations with luminance moments beside those without (see above)")
    ap.add_argument("--scenes", nargs="+", default=DEFAULT_SCENES, choices=sorted(SCENES))
    ap.add_argument("--samples", nargs="+", type=int, default=list(SAMPLES), metavar="N", help="samples per timed add")
    args = ap.parse_args()
    if args.adaptive and (args.path_depth or args.sun or args.emit or args.emit_power or args.emit_mis or args.scenes != DEFAULT_SCENES or args.samples != list(SAMPLES)):
        ap.error("--adaptive takes none of --path-depth, --sun, --emit, --emit-power, --emit-mis, --scenes, --samples")
    if args.sun and not args.path_depth:
        ap.error("--sun goes with --path-depth")
    if args.emit and not args.path_depth:
        ap.error("--emit goes with --path-depth")
    if args.emit_power and not args.emit:
        ap.error("--emit-power goes with --emit")
    if args.emit_mis and not args.emit_power:
        ap.error("--emit-mis goes with --emit-power")
    if args.glass and not args.guides:
        ap.error("--glass goes with --guides")
    V = vrt_import.vrt()
    if args.adaptive:
        return adaptive_main(V, args)
    if args.guides:
        return guides_main(V, args)
    if args.moments:
        return moments_main(V, args)
    from conftest import MAPS, room_world
    W, H = 1920, 1080
    ctx = V.Context(0)
    d_rgba, d_id = ctx.device_alloc(W * H * 4), ctx.device_alloc(W * H * 8)
    d_rgb = ctx.device_alloc(W * H * 12) if args.hdr else None
    rows = []
    last_spread = [0.0, 0.0]   # of the last add_ms(): the fastest and the slowest timed add
    for name, depth, sun, emit, imp, mis in [(s, d, r, e, m, f) for s in SCENES if s in args.scenes for d in (args.path_depth or [None]) for r in (args.sun or [None])
                                             for e in (args.emit or [None]) for m in ((args.emit_power if e else args.emit_power[:1]) if args.emit_power else [None])
                                             for f in ((args.emit_mis if e and m == 1 else args.emit_mis[:1]) if args.emit_mis else [None])]:
        m, pos, yaw, pitch = SCENES[name]
        if m == "room":
            w = room_world(V)
        elif m == "lamp":
            import emit_worlds
            w = emit_worlds.lamp_room(V)
        elif m == "power":
            import emit_power_worlds
            w = emit_power_worlds.room(V)
        elif m == "mis":
            import emit_mis_worlds
            w = emit_mis_worlds.room(V)
        else:
            w = V.World()
            assert w.load_vox(os.path.join(MAPS, m + ".vox"))
        tex, dim = w.flatten()
        w.close()
        ctx.upload_octree(tex, dim)
        ip, iv, cp, _ = V.camera_block(pos, yaw, pitch, W, H)
        ctx.set_camera(ip, iv, cp)
        ctx.set_params(ctx.default_params())
        if args.variant is not None:
            ctx.set_variant(args.variant)
        if depth is not None:
            ctx.set_path_depth(depth)
        if sun is not None:
            ctx.set_sun_disc(sun)
        if emit is not None:
            ctx.set_emitter_sampling(emit)
        if imp is not None:
            ctx.set_emitter_importance(imp if emit else 0)
        if mis is not None:
            ctx.set_emitter_mis(mis if emit and imp == 1 else 0)
        opaque = V.tree_is_opaque(tex)
        for mname in args.mode:
            mode = V.MODES[mname]
            ctx.dispatch_timed(W, H, 0, H, mode, d_rgba, d_id, 5)
            frame_ms = float(np.median(ctx.dispatch_timed(W, H, 0, H, mode, d_rgba, d_id, max(args.reps, 5))))
            for n in args.samples:
                base_ms = None
                for lens in [None] + args.lens:
                    ctx.set_lens(*(lens or (0.0, 1.0)))

                    def add_ms(hdr):
                        ctx.accum_begin(W, H, 0, mode=mode, jitter=args.jitter, **({"hdr": True} if hdr else {}))
                        ctx.accum_add(n)          # the first add: pass 1 or the frame once per accumulation, code object load
                        ctx.synchronize()
                        ts = []
                        for _ in range(args.reps):
                            t0 = time.perf_counter()
                            ctx.accum_add(n)
                            ctx.synchronize()
                            ts.append((time.perf_counter() - t0) * 1e3)
                        last_spread[:] = [min(ts), max(ts)]
                        return float(np.median(ts))

                    def resolve_ms(hdr):
                        ts = []
                        for _ in range(args.reps + 1):
                            t0 = time.perf_counter()
                            if hdr:
                                ctx.accum_resolve_hdr_device(d_rgb, d_rgba, None, "reinhard", 1.0)
                            else:
                                ctx.accum_resolve_device(d_rgba, None, None)
                            ctx.synchronize()
                            ts.append((time.perf_counter() - t0) * 1e3)
                        return float(np.median(ts[1:]))

                    ms = add_ms(False)
                    plain_resolve = resolve_ms(False) if args.hdr else None
                    row = {"scene": name, "width": W, "height": H, "path": "opaque" if opaque else "general", "n": n,
                           "add_ms": round(ms, 4), "n_frames_ms": round(n * frame_ms, 4), "frame_ms": round(frame_ms, 4),
                           "ratio": round(ms / (n * frame_ms), 3), "reps": args.reps}
                    if args.mode != ["full"] or args.jitter or args.lens:
                        row.update(mode=mname, jitter=bool(args.jitter))
                    if depth is not None:
                        row.update(path_depth=depth, per_sample_ms=round(ms / n, 4), add_ms_min_max=[round(v, 4) for v in last_spread])
                        if args.variant is not None:
                            row.update(variant=args.variant)
                    if sun is not None:
                        row.update(sun_disc=sun)
                    if emit is not None:
                        row.update(emitter_sampling=emit, emitters=len(ctx.emitters()))
                        if emit and row["emitters"]:
                            row["path"] = "general"   # the opaque routes are not taken
                        if imp is not None and emit:
                            row.update(emitter_importance=imp)
                        if mis is not None and emit and imp == 1:
                            row.update(emitter_mis=mis)
                    if lens is None:
                        base_ms = ms
                    else:
                        sel = V.lens_choice(tex, cp, iv, lens[0])
                        row.update(aperture=lens[0], focus=lens[1], side="shared" if sel["eye_shared"] and sel["first_shared"] else "per_lane",
                                   eye_shared=sel["eye_shared"], first_shared=sel["first_shared"], vs_lens_free=round(ms / base_ms, 3))
                    if args.hdr:
                        hms = add_ms(True)
                        row.update(hdr_add_ms=round(hms, 4), hdr_vs_plain=round(hms / ms, 3), resolve_ms=round(plain_resolve, 4),
                                   hdr_resolve_ms=round(resolve_ms(True), 4))
                    print(json.dumps(row), flush=True)
                    rows.append(row)
            ctx.set_lens(0.0, 1.0)
    ctx.device_free(d_rgba)
    ctx.device_free(d_id)
    if d_rgb:
        ctx.device_free(d_rgb)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def _scenes(V, ctx, W, H, names=DEFAULT_SCENES):
    from conftest import MAPS, room_world
    for name, (m, pos, yaw, pitch) in SCENES.items():
        if name not in names or (name not in DEFAULT_SCENES and m != "lamp"):
            continue
        if m == "room":
            w = room_world(V)
        elif m == "lamp":   # on request: through its pane (--guides --glass)
            import emit_worlds
            w = emit_worlds.lamp_room(V)
        else:
            w = V.World()
            assert w.load_vox(os.path.join(MAPS, m + ".vox"))
        tex, dim = w.flatten()
        w.close()
        ctx.upload_octree(tex, dim)
        ip, iv, cp, _ = V.camera_block(pos, yaw, pitch, W, H)
        ctx.set_camera(ip, iv, cp)
        ctx.set_params(ctx.default_params())
        yield name, tex


def _round_times(ctx, W, H, mode, jitter, adaptive, rounds):
    """one accumulation, one round per add: [(ms, active fraction or None)] per add"""
    ctx.accum_begin(W, H, 0, mode=mode, jitter=jitter, adaptive=adaptive)
    ctx.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        ctx.accum_add(1)
        ctx.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        out.append((ms, ctx.accum_counts()[1] / (W * H) if adaptive else None))
    return out


def adaptive_main(V, args):
    W, H = 1920, 1080
    rule = tuple(args.adaptive)
    ctx = V.Context(0)
    configs = (("primary", True, None), ("full", False, None), ("full", True, tuple(args.adaptive_lens)))
    rows = []
    for name, tex in _scenes(V, ctx, W, H):
        opaque = V.tree_is_opaque(tex)
        for mname, jitter, lens in configs:
            mode = V.MODES[mname]
            ctx.set_lens(*(lens or (0.0, 1.0)))
            _round_times(ctx, W, H, mode, jitter, rule, 2)          # code objects, buffers
            _round_times(ctx, W, H, mode, jitter, None, 2)
            reps = max(1, args.reps)
            plain = np.median([[t for t, _ in _round_times(ctx, W, H, mode, jitter, None, args.rounds)] for _ in range(reps)], axis=0)
            runs = [_round_times(ctx, W, H, mode, jitter, rule, args.rounds) for _ in range(reps)]
            adapt = np.median([[t for t, _ in r] for r in runs], axis=0)
            for r in range(args.rounds):
                row = {"scene": name, "width": W, "height": H, "path": "opaque" if opaque else "general", "mode": mname,
                       "jitter": jitter, "aperture": lens[0] if lens else 0.0, "focus": lens[1] if lens else 1.0,
                       "min": rule[0], "max": rule[1], "tol": rule[2], "round": r + 1, "add_ms": round(float(adapt[r]), 4),
                       "active_after": round(runs[0][r][1], 5), "plain_add_ms": round(float(plain[r]), 4),
                       "ratio": round(float(adapt[r] / plain[r]), 3), "reps": reps}
                print(json.dumps(row), flush=True)
                rows.append(row)
            ctx.set_lens(0.0, 1.0)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def guides_main(V, args):
    W, H = 1920, 1080
    ctx = V.Context(0)
    d_planes = [ctx.device_alloc(W * H * 4 * k) for k in (3, 4, 1, 1)]
    lens = tuple(args.lens[0]) if args.lens else (0.1, 40.0)
    rows = []

    def timed(body, before=None):
        ts = []
        for _ in range(args.reps + 1):
            if before:
                before()
                ctx.synchronize()
            t0 = time.perf_counter()
            body()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])   # the first: code object load, buffers

    for name, tex in _scenes(V, ctx, W, H, args.scenes):
        for source, jitter, ln in (("corner", False, None), ("jitter", True, None), ("lens", False, lens)):
            ctx.set_lens(*(ln or (0.0, 1.0)))
            for n, glass in [(n, g) for n in args.samples for g in ((False, True) if args.glass else (False,))]:
                ctx.set_guide_glass(glass)
                ctx.accum_begin(W, H, 0, mode=V.MODES["primary"], jitter=jitter)
                ctx.accum_add(n)
                ctx.accum_guides_device(*d_planes)
                ctx.synchronize()
                guide = timed(lambda: ctx.accum_guides_device(*d_planes), before=lambda: ctx.accum_add(n))
                resolve = timed(lambda: ctx.accum_guides_device(*d_planes))
                ctx.accum_begin(W, H, 0, mode=V.MODES["primary"], jitter=jitter)
                ctx.accum_add(n)
                ctx.synchronize()
                add = timed(lambda: ctx.accum_add(n))
                row = {"scene": name, "width": W, "height": H, "source": source, "n": n, "guide_ms": round(guide[0], 4),
                       "guide_ms_min_max": [round(guide[1], 4), round(guide[2], 4)], "resolve_ms": round(resolve[0], 4),
                       "guide_per_sample_ms": round((guide[0] - resolve[0]) / n, 4), "primary_add_ms": round(add[0], 4),
                       "primary_add_ms_min_max": [round(add[1], 4), round(add[2], 4)], "primary_per_sample_ms": round(add[0] / n, 4),
                       "guide_vs_primary": round((guide[0] - resolve[0]) / add[0], 3), "reps": args.reps}
                if ln:
                    row.update(aperture=ln[0], focus=ln[1])
                if args.glass:
                    row["glass"] = glass
                print(json.dumps(row), flush=True)
                rows.append(row)
        ctx.set_lens(0.0, 1.0)
        ctx.set_guide_glass(False)
    for d in d_planes:
        ctx.device_free(d)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def moments_main(V, args):
    W, H = 1920, 1080
    ctx = V.Context(0)
    d_rgb, d_rgba, d_var, d_plane = (ctx.device_alloc(W * H * k) for k in (12, 4, 4, 4))
    rows = []

    def timed(body):
        ts = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            body()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])   # the first: code object load, buffers

    for name, tex in _scenes(V, ctx, W, H, args.scenes):
        opaque = V.tree_is_opaque(tex)
        for depth in args.path_depth or [1]:
            ctx.set_path_depth(depth)
            for source, jitter in (("corner", False), ("jitter", True)):
                for n in args.samples:
                    ts = {False: [], True: []}
                    for r in range(2 * max(args.reps, 1) + 2):          # alternated, the first of each untimed
                        moments = bool(r & 1)
                        ctx.accum_begin(W, H, 0, mode=V.MODES["full"], jitter=jitter, hdr=True, moments=moments)
                        ctx.accum_add(n)          # the first add: pass 1 once per accumulation, code object load
                        ctx.synchronize()
                        t0 = time.perf_counter()
                        ctx.accum_add(n)
                        ctx.synchronize()
                        if r >= 2:
                            ts[moments].append((time.perf_counter() - t0) * 1e3)
                    hdr_ms, mom_ms = float(np.median(ts[False])), float(np.median(ts[True]))
                    # the accumulation begun last keeps moments: its plane, then the filtered resolve on it and on one without
                    var = timed(lambda: ctx.accum_variance_device(d_plane))
                    with_plane = timed(lambda: ctx.accum_resolve_hdr_filtered_var_device(d_rgb, d_rgba, d_var))
                    ctx.accum_begin(W, H, 0, mode=V.MODES["full"], jitter=jitter, hdr=True)
                    ctx.accum_add(2 * n)
                    spatial = timed(lambda: ctx.accum_resolve_hdr_filtered_var_device(d_rgb, d_rgba, d_var))
                    row = {"scene": name, "width": W, "height": H, "path": "opaque" if opaque else "general", "source": source,
                           "path_depth": depth, "n": n, "hdr_add_ms": round(hdr_ms, 4), "moments_add_ms": round(mom_ms, 4),
                           "hdr_add_ms_min_max": [round(min(ts[False]), 4), round(max(ts[False]), 4)],
                           "moments_add_ms_min_max": [round(min(ts[True]), 4), round(max(ts[True]), 4)],
                           "hdr_per_sample_ms": round(hdr_ms / n, 4), "moments_per_sample_ms": round(mom_ms / n, 4),
                           "moments_vs_hdr": round(mom_ms / hdr_ms, 4), "variance_ms": round(var[0], 4),
                           "filtered_var_spatial_ms": round(spatial[0], 4), "filtered_var_moments_ms": round(with_plane[0], 4),
                           "filtered_var_moments_ms_min_max": [round(with_plane[1], 4), round(with_plane[2], 4)], "reps": args.reps}
                    print(json.dumps(row), flush=True)
                    rows.append(row)
        ctx.set_path_depth(1)
    for d in (d_rgb, d_rgba, d_var, d_plane):
        ctx.device_free(d)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
