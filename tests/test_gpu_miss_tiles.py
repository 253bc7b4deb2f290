"""Miss tiles (include/vrt.h VRT_OPT_MISS_TILES) on the device: with the option on and off every launch shape writes the same bytes --
whole frames, row ranges, row-tile shards (compact and at their frame place), four-view launches, the feedback scheduler's measuring
and ordered launches, two streams sharing one cached mask, frames after patches and after compaction, eyes inside a solid and
inside glass (the v3 kernels: no mask), a projection the ray-table check refuses (no mask) -- and the bench frame equals the oracle's."""
import os

import numpy as np
import pytest

from conftest import MAPS

pytestmark = pytest.mark.gpu

POSE = (63.5, 60.5, 140.5, -90.0, -10.0)   # bench.py's dragon pose


@pytest.fixture(scope="module")
def dragon(V):
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    yield w
    w.close()


@pytest.fixture()
def ctx(V, dragon):
    c = V.Context(0)
    tex, dim = dragon.flatten()
    c.upload_octree(tex, dim)
    _warm(c, V)
    yield c
    c.close()


def _cam(ctx, V, pose, W, H):
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    ctx.set_camera(ip, iv, cp)
    return ip, iv, cp


def _same(got, ref, what):
    for g, r, part in zip(got, ref, ("rgba", "id_dist")):
        if not np.array_equal(g, r):
            bad = np.argwhere(np.any(g != r, axis=-1) if g.ndim == 3 else g != r)
            raise AssertionError(f"{what} {part}: {len(bad)} pixels differ, first at {tuple(bad[0])}")


def _warm(ctx, V, restore=None):
    """enough mask requests with an unchanged tree for the dispatcher to make its box list (max(64, records / 512) of them); a
    small frame at the bench pose, then the camera `restore` (inv_proj, inv_view, cam_pos) back"""
    ctx.set_option(V.OPT_MISS_TILES, 1)
    _cam(ctx, V, POSE, 64, 48)
    for _ in range(160):
        ctx.dispatch(64, 48, V.MODE_PRIMARY)
    if restore is not None:
        ctx.set_camera(*restore)


def _on_off(ctx, V, run, what):
    """run() with the option on, then off, then on again (a view's mask is built the second time the view is seen, so the third run
    reads it): all three the same bytes"""
    out = []
    for on in (1, 0, 1):
        ctx.set_option(V.OPT_MISS_TILES, on)
        out.append(run())
    ctx.set_option(V.OPT_MISS_TILES, 1)
    _same(out[0], out[1], what + " (on / off)")
    _same(out[2], out[1], what + " (on again / off)")
    return out[1]


def test_whole_frames_match_off_and_oracle(V, O, ctx, dragon):
    W, H = 1920, 1080
    _cam(ctx, V, POSE, W, H)
    for mode in (V.MODE_PRIMARY, V.MODE_PRIMARY_SHADOW):
        _on_off(ctx, V, lambda: ctx.dispatch(W, H, mode), f"1080p mode {mode}")
    W, H = 480, 270
    cam = _cam(ctx, V, POSE, W, H)
    tex, dim = dragon.flatten()
    for mode in (V.MODE_PRIMARY, V.MODE_PRIMARY_SHADOW):
        ctx.set_option(V.OPT_MISS_TILES, 1)
        rgba, idd = ctx.dispatch(W, H, mode)
        ref_rgba, ref_id, _, _ = O.render(O.make_scene(tex, dim, *cam), W, H, mode)
        _same((rgba, idd), (np.asarray(ref_rgba).reshape(H, W, 4), np.asarray(ref_id).reshape(H, W, 2)), f"oracle mode {mode}")


def test_rows_shards_and_tiles(V, ctx):
    W, H = 1280, 720
    _cam(ctx, V, POSE, W, H)
    d_rgba, d_id = ctx.device_alloc(W * H * 4), ctx.device_alloc(W * H * 8)
    try:
        def rows():   # a row range that starts inside a frame tile: a wave's rows straddle two rows of the mask
            ctx.device_write(d_rgba, np.zeros(W * H * 4, np.uint8))
            ctx.device_write(d_id, np.zeros(W * H * 8, np.uint8))
            ctx.dispatch_rows(W, H, 37, 611, V.MODE_PRIMARY_SHADOW, d_rgba, d_id)
            return ctx.device_read(d_rgba, (H, W, 4), np.uint8), ctx.device_read(d_id, (H, W, 2), np.int32)
        _on_off(ctx, V, rows, "rows 37..611")
        for tile_rows, n_shards in ((5, 3), (8, 2), (13, 4)):
            for shard in range(n_shards):
                def shard_run(shard=shard):   # compact outputs: the shard's rows one after the other
                    ctx.device_write(d_rgba, np.zeros(W * H * 4, np.uint8))
                    ctx.device_write(d_id, np.zeros(W * H * 8, np.uint8))
                    ctx.dispatch_shard(W, H, tile_rows, shard, n_shards, V.MODE_PRIMARY, d_rgba, d_id)
                    return ctx.device_read(d_rgba, (H, W, 4), np.uint8), ctx.device_read(d_id, (H, W, 2), np.int32)
                _on_off(ctx, V, shard_run, f"shard {shard}/{n_shards} of {tile_rows}-row tiles")

            def tiles_run():   # every shard at its frame place
                ctx.device_write(d_rgba, np.zeros(W * H * 4, np.uint8))
                ctx.device_write(d_id, np.zeros(W * H * 8, np.uint8))
                for s in range(n_shards):
                    ctx.dispatch_tiles(W, H, tile_rows, s, n_shards, V.MODE_PRIMARY_SHADOW, d_rgba, d_id)
                return ctx.device_read(d_rgba, (H, W, 4), np.uint8), ctx.device_read(d_id, (H, W, 2), np.int32)
            _on_off(ctx, V, tiles_run, f"tiles {tile_rows}/{n_shards}")
    finally:
        ctx.device_free(d_rgba)
        ctx.device_free(d_id)


def test_four_view_launches(V, ctx):
    W, H = 640, 360
    poses = [POSE, (20.5, 70.5, 120.5, -60.0, -20.0), (150.5, 40.5, 60.5, 180.0, 0.0), (63.5, 200.5, 40.5, 90.0, -80.0)]
    bufs = [(ctx.device_alloc(W * H * 4), ctx.device_alloc(W * H * 8)) for _ in poses]
    try:
        views = []
        for p, (a, b) in zip(poses, bufs):
            ip, iv, cp, _ = V.camera_block(p[:3], p[3], p[4], W, H)
            views.append((ip, iv, cp, a, b))

        def run(tile_rows=H, shard=0, n=1):
            for a, b in bufs:
                ctx.device_write(a, np.zeros(W * H * 4, np.uint8))
                ctx.device_write(b, np.zeros(W * H * 8, np.uint8))
            ctx.dispatch_views(W, H, tile_rows, shard, n, V.MODE_PRIMARY_SHADOW, views)
            return (np.stack([ctx.device_read(a, (H, W, 4), np.uint8) for a, _ in bufs]),
                    np.stack([ctx.device_read(b, (H, W, 2), np.int32) for _, b in bufs]))
        _on_off(ctx, V, run, "four views")
        _on_off(ctx, V, lambda: run(8, 1, 3), "four views, shard 1/3 of 8-row tiles")
    finally:
        for a, b in bufs:
            ctx.device_free(a)
            ctx.device_free(b)


def test_scheduler_measuring_and_ordered_launches(V, ctx):
    W, H = 1920, 1080
    _cam(ctx, V, POSE, W, H)
    for period in (1, 3):
        ctx.set_tile_scheduling(period)

        def run():
            outs = [ctx.dispatch(W, H, V.MODE_PRIMARY) for _ in range(5)]   # measuring launches, then ordered ones
            for o in outs[1:]:
                _same(o, outs[0], f"period {period}: launch to launch")
            return outs[-1]
        _on_off(ctx, V, run, f"scheduler period {period}")
    ctx.set_tile_scheduling(16)


def test_two_streams_share_a_mask(V, ctx):
    """vrt_dispatch_async alternates two streams: the mask built on the first is read on the second after its build event"""
    W, H = 1280, 720
    _cam(ctx, V, POSE, W, H)
    ctx.set_option(V.OPT_MISS_TILES, 0)
    ref = ctx.dispatch(W, H, V.MODE_PRIMARY)
    ctx.set_option(V.OPT_MISS_TILES, 1)
    outs = [(np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 2), np.int32)) for _ in range(4)]
    tickets = [ctx.dispatch_async(W, H, V.MODE_PRIMARY, r, i) for r, i in outs[:2]]
    for t in tickets:
        ctx.dispatch_wait(t)
    tickets = [ctx.dispatch_async(W, H, V.MODE_PRIMARY, r, i) for r, i in outs[2:]]
    for t in tickets:
        ctx.dispatch_wait(t)
    for k, o in enumerate(outs):
        _same(o, ref, f"async frame {k}")


def test_after_patches_and_compaction(V, O, ctx, dragon):
    """edits in view change the occupancy boxes: the masks built before them must not be reused"""
    W, H = 640, 360
    cam = _cam(ctx, V, POSE, W, H)
    _on_off(ctx, V, lambda: ctx.dispatch(W, H, V.MODE_PRIMARY_SHADOW), "before edits")
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    try:
        # a solid box out in the sky the camera sees, then a voxel removed from the model
        lo, hi = (40, 90, 60), (47, 97, 67)
        g = np.stack(np.meshgrid(*[np.arange(lo[k], hi[k] + 1) for k in range(3)], indexing="ij"), -1).reshape(-1, 3)
        w.insert_many(g.astype(np.int32), np.full(len(g), 0xff3030ff, np.uint32), 3.0, 0.0, 0.0)
        if ctx.patch_box(w, lo, hi) is None:
            ctx.upload_octree(*w.flatten())
        _warm(ctx, V, cam)
        f_box = _on_off(ctx, V, lambda: ctx.dispatch(W, H, V.MODE_PRIMARY_SHADOW), "after a box edit")
        tex, dim = w.flatten()
        ref = O.render(O.make_scene(tex, dim, *cam), W, H, V.MODE_PRIMARY_SHADOW)
        _same(f_box, (np.asarray(ref[0]).reshape(H, W, 4), np.asarray(ref[1]).reshape(H, W, 2)), "after a box edit vs oracle")
        x, y, z = (int(v) for v in g[len(g) // 2])
        w.remove(x, y, z)
        w.remove(lo[0], lo[1], lo[2])
        for p in ((x, y, z), lo):
            if ctx.patch_voxel(w, *p) is None:
                ctx.upload_octree(*w.flatten())
        _warm(ctx, V, cam)
        _on_off(ctx, V, lambda: ctx.dispatch(W, H, V.MODE_PRIMARY_SHADOW), "after voxel edits")
        ctx.compact()
        _warm(ctx, V, cam)
        f_c = _on_off(ctx, V, lambda: ctx.dispatch(W, H, V.MODE_PRIMARY_SHADOW), "after compaction")
        tex, dim = w.flatten()
        ref = O.render(O.make_scene(tex, dim, *cam), W, H, V.MODE_PRIMARY_SHADOW)
        _same(f_c, (np.asarray(ref[0]).reshape(H, W, 4), np.asarray(ref[1]).reshape(H, W, 2)), "after compaction vs oracle")
    finally:
        w.close()


def test_eye_inside_a_solid_and_inside_glass(V, ctx):
    W, H = 320, 180
    # inside a voxel of the model (refraction byte 255: the v4 kernels, the box around the eye marks the whole view)
    _cam(ctx, V, (40.5, 5.5, 44.5, -90.0, -10.0), W, H)
    _on_off(ctx, V, lambda: ctx.dispatch(W, H, V.MODE_PRIMARY_SHADOW), "eye in the model")
    # inside glass (a medium: the v3 kernels, which take no mask)
    w = V.World()
    g = np.stack(np.meshgrid(np.arange(0, 6), np.arange(0, 6), np.arange(0, 6), indexing="ij"), -1).reshape(-1, 3)
    w.insert_many(g.astype(np.int32), np.full(len(g), 0xc8dcff50, np.uint32), 1.5, 0.0, 0.0)
    w.insert_many(np.array([[20, 2, 2], [2, 20, 2]], np.int32), np.full(2, 0xa0a0a0ff, np.uint32), 3.0, 0.0, 0.0)
    ctx.upload_octree(*w.flatten())
    w.close()
    _cam(ctx, V, (2.5, 2.5, 2.5, 0.0, 10.0), W, H)
    _on_off(ctx, V, lambda: ctx.dispatch(W, H, V.MODE_PRIMARY_SHADOW), "eye in glass")


def test_projection_without_tables(V, ctx):
    W, H = 320, 180
    ip, iv, cp, _ = V.camera_block(POSE[:3], POSE[3], POSE[4], W, H)
    ip = np.array(ip, np.float32).reshape(-1).copy()
    ip[4] = np.float32(0.01)   # x depends on v: the ray-table check refuses the projection
    ctx.set_camera(ip, iv, cp)
    _on_off(ctx, V, lambda: ctx.dispatch(W, H, V.MODE_PRIMARY), "non-separable projection")


def test_many_views_recycle_masks(V, ctx):
    """more views than the mask cache holds, each drawn twice: the recycled masks are rebuilt for their new view"""
    W, H = 256, 144
    rng = np.random.default_rng(3)
    poses = [(float(x), float(y), float(z), float(yaw), float(pitch)) for x, y, z, yaw, pitch in
             zip(rng.uniform(-40, 160, 11), rng.uniform(10, 120, 11), rng.uniform(-40, 200, 11), rng.uniform(-180, 180, 11),
                 rng.uniform(-60, 30, 11))]
    for rep in range(2):
        for k, p in enumerate(poses):
            _cam(ctx, V, p, W, H)
            _on_off(ctx, V, lambda: ctx.dispatch(W, H, V.MODE_PRIMARY), f"view {k} pass {rep}")


def test_device_skips_the_cleared_tiles(V, ctx, dragon):
    """the mask really reaches the kernel: at the bench pose, the waves of the tiles the host mask clears take a fraction of their
    clock ticks with the option on (per-tile ticks through vrt_set_tile_order's d_tile_cost), and no mask is read on a view's
    first frame (built on its second)"""
    W, H = 1920, 1080
    ip, iv, cp = _cam(ctx, V, POSE, W, H)
    tex, _ = dragon.flatten()
    mask, _, whole = V.miss_mask(tex, ip, iv, cp, W, H)
    assert not whole
    cleared = (mask == 0).reshape(-1)
    assert cleared.mean() > 0.35
    n = mask.size
    d_cost, d_rgba, d_id = ctx.device_alloc(n * 4), ctx.device_alloc(W * H * 4), ctx.device_alloc(W * H * 8)
    try:
        ctx.set_tile_order(1, None, d_cost)

        def ticks():
            ctx.dispatch_rows(W, H, 0, H, V.MODE_PRIMARY, d_rgba, d_id)
            return ctx.device_read(d_cost, (n,), np.uint32).astype(np.float64)
        ctx.set_option(V.OPT_MISS_TILES, 0)
        ticks()
        off = np.mean([ticks()[cleared].mean() for _ in range(3)])
        ctx.set_option(V.OPT_MISS_TILES, 1)
        ctx.set_camera(*V.camera_block((POSE[0] + 0.25, POSE[1], POSE[2]), POSE[3], POSE[4], W, H)[:3])
        first = ticks()[cleared].mean()    # a view not seen before: no mask yet
        ctx.set_camera(ip, iv, cp)
        ticks()                            # the bench view's first sight with the option on
        on = np.mean([ticks()[cleared].mean() for _ in range(3)])   # seen before: its mask is built and read
        assert on < 0.5 * off, (on, off)
        assert first > 0.7 * off, (first, off)
    finally:
        ctx.set_tile_order(0)
        ctx.set_option(V.OPT_MISS_TILES, 1)
        for p in (d_cost, d_rgba, d_id):
            ctx.device_free(p)
