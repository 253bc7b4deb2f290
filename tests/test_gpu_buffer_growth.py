"""Every device buffer a context keeps, at changing sizes. The context owns about thirty allocations (scratch images, query and ray
staging, the accumulation's groups, the lanes, the record array, the caches) and grows each one where a call finds it too small:
a growth that handed out a stale pointer, kept a stale count, or freed a block that work in flight still used would change a
result. So every host-buffer entry point runs on ONE context at a small size, at a larger size that makes every one of its buffers
grow, and at the small size again -- and each result must equal, byte for byte (float images bit for bit), the same call on a
fresh context that only ever saw that size.

Also here: the device resolves on a caller's stream right after a growth (the join with the context's stream), a scene whose
record array grows by upload and by patches, and three contexts created, filled and destroyed in a row.

The world is test_gpu_dispatch_interleaved's corner world: a floor, a wall and a pillar, a few hundred voxels."""
import numpy as np
import pytest

import temporal_worlds as TW

pytestmark = pytest.mark.gpu

F = np.float32
POSE = (50.5, 40.5, 50.5, -135.0, -43.0)
# frame shape and ray / point count of each step: small, one that outgrows every buffer (72 x 40 is ragged in the 8 x 8 trace tiles
# and in the display pass's tiles), small again
STEPS = ((16, 8, 1), (72, 40, 1000), (16, 8, 3))
TOLERANCE = 8
GUIDES = ("normal", "albedo", "depth", "coverage")


def _world(V, extra=0):
    """the corner world; `extra` more voxels stacked on its floor (more records, same place)"""
    vox = [(x, 10, z) for x in range(20, 36) for z in range(20, 36)]
    vox += [(20, y, z) for y in range(11, 19) for z in range(20, 36, 2)]
    vox += [(x, y, 30) for x in (28, 29) for y in range(11, 24)]
    vox += [(22 + i % 12, 11 + i // 144, 21 + (i // 12) % 12) for i in range(extra)]
    w = V.World()
    for i, (x, y, z) in enumerate(vox):
        w.insert(x, y, z, [0x50b43cff, 0x644628ff, 0xa0a0a0ff][i % 3])
    return w


def _context(V, tex, dim):
    c = V.Context(0)
    c.upload_octree(tex, dim)
    return c


def _inputs(n):
    """n rays from outside wide root 0 into the content, n points around it; the same for every context"""
    rng = np.random.default_rng(1000 + n)
    o = np.stack([rng.uniform(-40, -4, n), rng.uniform(14, 60, n), rng.uniform(-40, 50, n)], axis=1)
    t = np.stack([rng.uniform(21, 35, n), rng.uniform(10, 20, n), rng.uniform(21, 35, n)], axis=1)
    pts = rng.integers(18, 38, (n, 3)).astype(np.int32)
    return o.astype(F), (t - o).astype(F), pts


def _async(ctx, w, h):
    """one frame on each lane"""
    outs = [(np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 2), np.int32)) for _ in range(2)]
    tickets = [ctx.dispatch_async(w, h, mode, r, i) for mode, (r, i) in zip((1, 2), outs)]
    assert sorted(tickets) == [0, 1]
    for t in tickets:
        ctx.dispatch_wait(t)
    return outs[0] + outs[1]


def _accum(ctx, w, h, resolve, **kw):
    ctx.accum_begin(w, h, 3, mode=2, **kw)
    ctx.accum_add(2)
    ctx.accum_add(1)
    return resolve()


def _hdr(ctx):
    return ctx.accum_resolve_hdr("reinhard", 1.5) + ctx.accum_resolve_hdr_shown("reinhard", 1.5)


def _adaptive(ctx):
    return ctx.accum_resolve() + ctx.accum_counts()[:1]


def run_all(V, ctx, w, h, n):
    """every host-buffer entry point once, at frame shape w x h and n rays / points -> {call: tuple of arrays}"""
    cam = V.camera_block(POSE[:3], POSE[3], POSE[4], w, h)[:3]
    ctx.set_camera(*cam)
    o, d, pts = _inputs(n)
    out = {}
    for mode in (0, 1, 2):
        out[f"dispatch {mode}"] = ctx.dispatch(w, h, mode)
    rgba, idd = out["dispatch 2"]
    out["dispatch_frame"] = ctx.dispatch_frame(w, h, 2)
    out["dispatch_async"] = _async(ctx, w, h)
    out["denoise"] = (ctx.denoise(rgba, idd),)
    out["denoise_hdr"] = ctx.denoise_hdr(rgba[:, :, :3].astype(F) * F(3.0 / 255.0), idd, "reinhard", 0.5)
    out["cast_rays"] = ctx.cast_rays(o, d)
    out["find_voxels"] = ctx.find_voxels(pts)
    out["shade_rays"] = ctx.shade_rays(o, d, 2, width=8, first_sample=5, n_samples=2)
    out["shade_rays_hdr"] = ctx.shade_rays_hdr(o, d, 2, width=8, first_sample=5, n_samples=2, tonemap="reinhard", exposure=1.5)
    rays = ctx.guide_rays(o, d, width=8)
    out["guide_rays"] = tuple(rays[k] for k in ("normal", "albedo", "depth", "hit"))
    out["accum plain"] = _accum(ctx, w, h, ctx.accum_resolve)
    out["accum jitter"] = _accum(ctx, w, h, ctx.accum_resolve, jitter=True)
    out["accum adaptive"] = _accum(ctx, w, h, lambda: _adaptive(ctx), jitter=True, adaptive=(2, 4, TOLERANCE))
    out["accum hdr"] = _accum(ctx, w, h, lambda: _hdr(ctx), jitter=True, hdr=True)
    # what reads that HDR accumulation through the accumulation's own staging: its guide planes, the filtered resolves, the temporal
    # resolve without and with a history
    g = ctx.accum_guides()
    out["accum_guides"] = tuple(g[k] for k in GUIDES)
    out["accum filtered"] = ctx.accum_resolve_hdr_filtered(None, "reinhard", 1.5)
    out["accum filtered var"] = ctx.accum_resolve_hdr_filtered_var(None, "reinhard", 1.5)
    first = ctx.accum_resolve_hdr_temporal(None, None, None, None, "reinhard", 1.5)
    out["accum temporal"] = first
    out["accum temporal, history"] = ctx.accum_resolve_hdr_temporal(first[0], TW.prev_camera(cam), None, None, "reinhard", 1.5)
    # ... and the stateless host forms on the planes and the mean just resolved, through the context's
    mean = out["accum hdr"][0]
    out["filter_hdr"] = ctx.filter_hdr(mean, g, None, "reinhard", 1.5)
    out["filter_hdr_var"] = ctx.filter_hdr_var(mean, g, None, None, "reinhard", 1.5)
    out["temporal_hdr"] = ctx.temporal_hdr(cam, mean, g, first[0], TW.prev_camera(cam))
    return out


def _same(got, want, when):
    assert got.keys() == want.keys()
    for what in want:
        assert len(got[what]) == len(want[what]), (what, when)
        for k, (a, b) in enumerate(zip(got[what], want[what])):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert a.dtype == b.dtype and a.shape == b.shape, (what, k, when)
            assert a.size > 0 and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}, output {k} ({when}) differs from a fresh context's"


@pytest.fixture(scope="module")
def scene(V):
    w = _world(V)
    tex, dim = w.flatten()
    w.close()
    return tex, dim


@pytest.fixture(scope="module")
def fresh(V, scene):
    """each step's calls on a context of its own, which never sees another size"""
    ref = []
    for w, h, n in STEPS:
        c = _context(V, *scene)
        try:
            ref.append(run_all(V, c, w, h, n))
        finally:
            c.close()
    hits = ref[1]["cast_rays"][0]
    assert hits.sum() > 100 and ref[1]["find_voxels"][0].any(), "the large step's rays and points do not see the world"
    assert len(np.unique(ref[1]["dispatch 2"][0].reshape(-1, 4), axis=0)) > 8, "the large frame does not see the world"
    return ref


def test_every_entry_point_small_large_small_equals_fresh_contexts(V, scene, fresh):
    ctx = _context(V, *scene)
    try:
        for (w, h, n), want in zip(STEPS, fresh):
            _same(run_all(V, ctx, w, h, n), want, f"{w} x {h}, {n} rays, after the sizes before it")
    finally:
        ctx.close()


def _device_resolves(V, ctx, stream):
    """an accumulation that outgrows the one before it, then on `stream`: the three device resolves, two more samples at once,
    the three resolves again -> the sixteen images"""
    import torch
    w, h = STEPS[1][:2]
    ctx.set_camera(*V.camera_block(POSE[:3], POSE[3], POSE[4], w, h)[:3])
    _accum(ctx, 16, 8, lambda: _hdr(ctx), jitter=True, hdr=True)
    shapes = (((h, w, 4), torch.uint8), ((h, w, 2), torch.int32), ((h, w, 4), torch.uint8),    # resolve_device: bytes, id_dist, shown
              ((h, w, 3), torch.float32), ((h, w, 4), torch.uint8), ((h, w, 4), torch.uint8),  # resolve_hdr_device: mean, bytes, shown
              ((h, w, 3), torch.float32), ((h, w, 4), torch.uint8))                            # resolve_hdr_shown_device: filtered mean, bytes
    bufs = [[torch.zeros(s, dtype=t, device="cuda:0") for s, t in shapes] for _ in range(2)]
    torch.cuda.synchronize()
    ctx.accum_begin(w, h, 3, mode=2, jitter=True, hdr=True)
    for b in bufs:
        ctx.accum_add(2)
        p = [x.data_ptr() for x in b]
        ctx.accum_resolve_device(p[0], p[1], p[2], stream=stream)
        ctx.accum_resolve_hdr_device(p[3], p[4], p[5], "reinhard", 1.5, stream=stream)
        ctx.accum_resolve_hdr_shown_device(p[6], p[7], "reinhard", 1.5, stream=stream)
    ctx.synchronize()
    torch.cuda.synchronize()
    return {"device resolves": tuple(x.cpu().numpy() for b in bufs for x in b)}


def test_device_resolves_on_a_callers_stream_after_a_growth(V, scene):
    import torch
    side = torch.cuda.Stream(device="cuda:0")
    got = {}
    for name, stream in (("own", None), ("side", side.cuda_stream)):
        ctx = _context(V, *scene)
        try:
            got[name] = _device_resolves(V, ctx, stream)
        finally:
            ctx.close()
    first, second = got["own"]["device resolves"][:8], got["own"]["device resolves"][8:]
    assert not np.array_equal(first[3], second[3]), "the second resolve holds no more samples than the first"
    _same(got["side"], got["own"], "on a caller's stream")


def _frame_of(V, tex, dim, w, h):
    c = _context(V, tex, dim)
    try:
        return run_frames(V, c, w, h)
    finally:
        c.close()


def run_frames(V, ctx, w, h):
    ctx.set_camera(*V.camera_block(POSE[:3], POSE[3], POSE[4], w, h)[:3])
    return {f"dispatch {mode}": ctx.dispatch(w, h, mode) for mode in (1, 2)}


def test_a_record_array_that_grows_by_upload_and_by_patches(V, scene):
    w, h = STEPS[1][:2]
    ctx = _context(V, *scene)
    big = _world(V, extra=300)
    try:
        _same(run_frames(V, ctx, w, h), _frame_of(V, *scene, w, h), "the small world")
        small = ctx.scene_info()["n_records"]
        tex, dim = big.flatten()
        ctx.upload_octree(tex, dim)
        uploaded = ctx.scene_info()["n_records"]
        assert uploaded > small, "the second world has no more records than the first"
        _same(run_frames(V, ctx, w, h), _frame_of(V, tex, dim, w, h), "a larger world uploaded")
        patched = 0
        for i in range(64):   # one voxel at a time onto the wall's top, each a patch that appends its sub-tree to the record array
            x, y, z = 20, 19 + i // 16, 20 + i % 16
            big.insert(x, y, z, 0xffd2d2ff)
            if ctx.patch_voxel(big, x, y, z) is None:
                ctx.upload_octree(*big.flatten())
                uploaded = ctx.scene_info()["n_records"]
            else:
                patched += 1
            if patched >= 4 and ctx.scene_info()["n_records"] > uploaded:
                break
        assert patched >= 4 and ctx.scene_info()["n_records"] > uploaded, "no patch made the record array outgrow the upload"
        _same(run_frames(V, ctx, w, h), _frame_of(V, *big.flatten(), w, h), "patched past the uploaded records")
    finally:
        big.close()
        ctx.close()


def test_three_contexts_in_a_row(V, scene, fresh):
    """create, fill every buffer, destroy -- three times in one process; each behaves as a first context does"""
    w, h, n = STEPS[1]
    for k in range(3):
        ctx = _context(V, *scene)
        try:
            _same(run_all(V, ctx, w, h, n), fresh[1], f"context {k + 1} of three")
        finally:
            ctx.close()
