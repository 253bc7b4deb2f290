"""Frame time through the HOST-buffer entry points (what a main.cpp-style caller with std::vector images sees): a host clock around
each call, which ends in the wait for the context's stream. Frames are 1080p, ray batches 2^20 rays.

--json: one JSON line per form instead of the table ({"form", "ms", "calls", "lib"}; lib: VRT_HIP_LIB, the library under the clock)
and nothing of the asynchronous forms -- what an A/B of two builds of the library collects, one process per build and round."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vrt_import  # noqa: E402

V = vrt_import.vrt()


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    W, H = 1920, 1080
    w = V.World()
    assert w.load_vox(os.path.join(root, "tests/golden/maps/dragon.vox"))
    tex, dim = w.flatten()
    ctx = V.Context(0)
    ctx.upload_octree(tex, dim)
    ip, iv, cp, _ = V.camera_block((63.5, 60.5, 140.5), -90.0, -10.0, W, H)
    ctx.set_camera(ip, iv, cp)
    ctx.set_params(ctx.default_params())
    L, h = ctx._L, ctx._h
    rgba = np.zeros((H, W, 4), np.uint8)
    idd = np.zeros((H, W, 2), np.int32)
    shown = np.zeros((H, W, 4), np.uint8)
    as_json = "--json" in sys.argv[1:]
    px = (H, W)
    rgb, out_rgb, integ = (np.zeros(px + (3,), np.float32) for _ in range(3))
    normal, albedo = np.zeros(px + (3,), np.float32), np.zeros(px + (4,), np.float32)
    depth, cover, var, out_var = (np.zeros(px, np.float32) for _ in range(4))
    hist = [np.zeros((3,) + px + (4,), np.float32) for _ in range(2)]
    t = V.Context._temporal(None, (np.eye(4, dtype=np.float32).reshape(16), cp))
    cam = [a.ctypes.data for a in (ip, iv, cp)]
    # 2^20 rays: the frame's eye, towards points of the model's box
    n = 1 << 20
    rng = np.random.default_rng(7)
    o = np.ascontiguousarray(np.broadcast_to(np.float32((63.5, 60.5, 140.5)), (n, 3)))
    d = (rng.uniform(0.0, 126.0, (n, 3)) - o).astype(np.float32)
    box = np.float32(V.WORLD_BOX)
    hits = np.zeros(n, V.RAY_HIT_DTYPE)
    r_rgba, r_id, r_rgb = np.zeros((n, 4), np.uint8), np.zeros((n, 2), np.int32), np.zeros((n, 3), np.float32)
    r_n, r_a, r_z, r_h = np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    p = lambda a: a.ctypes.data   # noqa: E731

    def accum():
        """an HDR accumulation of two jittered samples for the accumulation's forms; the first guide call marches its guides"""
        ctx.accum_begin(W, H, 3, mode=2, jitter=True, hdr=True)
        ctx.accum_add(2)
        return 0

    for name, fn in [
        ("vrt_dispatch primary -> rgba + id/dist", lambda: L.vrt_dispatch(h, W, H, 0, rgba.ctypes.data, idd.ctypes.data)),
        ("vrt_dispatch primary -> rgba only", lambda: L.vrt_dispatch(h, W, H, 0, rgba.ctypes.data, None)),
        ("vrt_dispatch full -> rgba + id/dist", lambda: L.vrt_dispatch(h, W, H, 2, rgba.ctypes.data, idd.ctypes.data)),
        ("vrt_denoise_host", lambda: L.vrt_denoise_host(h, W, H, rgba.ctypes.data, idd.ctypes.data, shown.ctypes.data)),
        ("vrt_dispatch_frame full -> shown only", lambda: L.vrt_dispatch_frame(h, W, H, 2, shown.ctypes.data, None, None)),
        ("vrt_denoise_hdr_host", lambda: L.vrt_denoise_hdr_host(h, W, H, p(rgb), p(idd), None, p(out_rgb), p(shown))),
        ("vrt_filter_hdr_host", lambda: L.vrt_filter_hdr_host(h, W, H, p(rgb), p(normal), p(albedo), p(depth), p(cover), None, None, p(out_rgb), p(shown))),
        ("vrt_filter_hdr_var_host", lambda: L.vrt_filter_hdr_var_host(h, W, H, p(rgb), p(normal), p(albedo), p(depth), p(cover), p(var), None, None,
                                                                    p(out_rgb), p(shown), p(out_var))),
        ("vrt_temporal_hdr_host", lambda: L.vrt_temporal_hdr_host(h, W, H, *cam, p(rgb), p(normal), p(depth), p(cover), p(hist[0]), C.byref(t), p(hist[1]),
                                                                p(out_rgb), p(var))),
        ("vrt_cast_rays", lambda: L.vrt_cast_rays(h, n, p(o), 3, p(d), p(box[0]), p(box[1]), p(hits))),
        ("vrt_shade_rays full", lambda: L.vrt_shade_rays(h, n, p(o), 3, p(d), 1024, 2, 5, 1, p(r_rgba), p(r_id))),
        ("vrt_shade_rays_hdr full", lambda: L.vrt_shade_rays_hdr(h, n, p(o), 3, p(d), 1024, 2, 5, 1, None, p(r_rgb), p(r_rgba), p(r_id))),
        ("vrt_guide_rays", lambda: L.vrt_guide_rays(h, n, p(o), 3, p(d), 1024, p(r_n), p(r_a), p(r_z), p(r_h))),
        (None, accum),
        ("vrt_accum_resolve", lambda: L.vrt_accum_resolve(h, p(rgba), p(idd), p(shown))),
        ("vrt_accum_resolve_hdr", lambda: L.vrt_accum_resolve_hdr(h, p(out_rgb), None, p(rgba), p(shown))),
        ("vrt_accum_guides", lambda: L.vrt_accum_guides(h, p(normal), p(albedo), p(depth), p(cover))),
        ("vrt_accum_resolve_hdr_filtered_var", lambda: L.vrt_accum_resolve_hdr_filtered_var(h, None, None, p(out_rgb), p(shown), p(var))),
        ("vrt_accum_resolve_hdr_temporal", lambda: L.vrt_accum_resolve_hdr_temporal(h, C.byref(t), None, None, p(hist[0]), p(hist[1]), p(integ),
                                                                                  p(out_rgb), p(shown), p(var))),
    ]:
        if name is None:   # a set-up step, not a form
            fn()
            continue
        for _ in range(3):
            assert fn() == 0, name
        t0 = time.perf_counter()
        calls = 20
        for _ in range(calls):
            fn()
        ms = (time.perf_counter() - t0) / calls * 1e3
        if as_json:
            print(json.dumps({"form": name, "ms": round(ms, 4), "calls": calls, "lib": os.path.relpath(V.HIP_LIB, root)}), flush=True)
        else:
            print("%-42s %8.3f ms per call" % (name, ms))
    if as_json:
        return

    # the asynchronous, double-buffered form into page-locked buffers: two frames in flight
    for both in (True, False):
        bufs = [(ctx.host_alloc((H, W, 4), np.uint8), ctx.host_alloc((H, W, 2), np.int32) if both else None) for _ in range(2)]
        for mode, label in ((0, "primary"), (2, "full")):
            tickets = []
            for i in range(4):
                tickets.append(ctx.dispatch_async(W, H, mode, *bufs[i & 1]))
            for t in set(tickets):
                ctx.dispatch_wait(t)
            n = 40
            t0 = time.perf_counter()
            for i in range(n):
                ctx.dispatch_async(W, H, mode, *bufs[i & 1])
            ctx.dispatch_wait(0)
            ctx.dispatch_wait(1)
            dt = (time.perf_counter() - t0) / n
            ok = np.array_equal(bufs[0][0], bufs[1][0]) and (not both or np.array_equal(bufs[0][1], bufs[1][1]))
            print("%-58s %8.3f ms per frame  (both lanes hold the same frame: %s)" %
                  (f"vrt_dispatch_async {label} -> pinned rgba" + (" + id/dist" if both else " only"), dt * 1e3, ok))
        for a, b in bufs:
            ctx.host_free(a)
            if b is not None:
                ctx.host_free(b)


if __name__ == "__main__":
    main()
