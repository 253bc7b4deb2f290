"""Progressive accumulation of VRT_MODE_FULL on the MI355X (vrt_accum_*) against the checker (tests/oracle_samples.c: the oracle's
frame at initRNG sample index k). Every sample is pinned byte for byte; means, the display pass, both device paths (the
sample-looped bounce of opaque scenes and the general kernel), the restart rule and the error states are checked."""
import os

import numpy as np
import pytest

import oracle_samples
from conftest import MAPS

pytestmark = pytest.mark.gpu

SAMPLES = (0, 1, 2, 37, 2 ** 20 + 3, 2 ** 31 - 1)
SCENES = {   # name -> (map, W, H, pose), the golden frames' poses
    "dragon": ("dragon", 256, 144, (63.5, 60.5, 140.5, -90.0, -10.0)),
    "terrain": ("terrain", 240, 136, (512.5, 420.5, 1000.5, -90.0, -20.0)),
    "room_inside": ("room", 256, 144, (14.5, 30.5, 16.5, 32.0, -10.0)),
    "room_outside": ("room", 256, 144, (98.5, 34.5, 52.5, 197.0, -8.0)),
    "dragon_inside": ("dragon", 101, 67, (60.3, 30.7, 25.2, 37.0, 12.0)),
}


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    return oracle_samples.build(tmp_path_factory.mktemp("oracle_samples"))


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _setup(ctx, V, O, product_scenes, m, W, H, pose, records=None):
    tex, dim = product_scenes[m]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    if records is None:
        ctx.upload_octree(tex, dim)
    else:
        ctx.upload_records(*records)
    ctx.set_camera(ip, iv, cp)
    ctx.set_params(ctx.default_params())
    return O.make_scene(tex, dim, ip, iv, cp), (ip, iv, cp)


def _same(got, ref, what):
    if not np.array_equal(got, ref):
        bad = np.argwhere(np.any(got != ref, axis=-1))
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} pixels differ; first at (x={x}, y={y}): got {got[y, x]} want {ref[y, x]}")


def _accumulate(ctx, W, H, first, chunks):
    ctx.accum_begin(W, H, first)
    total = 0
    for n in chunks:
        total += n
        assert ctx.accum_add(n) == total
    return ctx.accum_resolve()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_each_sample_is_the_checker_sample(ctx, V, O, S, product_scenes, name):
    m, W, H, pose = SCENES[name]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    for k in SAMPLES:
        ref_rgba, ref_id = oracle_samples.render_sample(S, scene, W, H, O.MODE_FULL, k)
        rgba, idd, shown = _accumulate(ctx, W, H, k, [1])
        _same(rgba, ref_rgba, f"{name} sample {k} rgba8")
        _same(idd, ref_id, f"{name} sample {k} id_dist")
        _same(shown, O.denoise(ref_rgba, ref_id), f"{name} sample {k} shown")


def test_record_only_upload(ctx, V, O, S, product_scenes):
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    rec = w.records()
    w.close()
    m, W, H, pose = SCENES["dragon"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose, records=rec)
    for k in (0, 37, 2 ** 31 - 1):
        ref_rgba, ref_id = oracle_samples.render_sample(S, scene, W, H, O.MODE_FULL, k)
        rgba, idd, _ = _accumulate(ctx, W, H, k, [1])
        _same(rgba, ref_rgba, f"records sample {k} rgba8")
        _same(idd, ref_id, f"records sample {k} id_dist")


@pytest.mark.parametrize("name", ["dragon", "room_outside"])
def test_means_chunking_and_display_pass(ctx, V, O, S, product_scenes, name):
    m, W, H, pose = SCENES[name]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    first = 5
    acc = np.zeros((H, W, 4), np.uint64)
    ref_id = None
    for k in range(first, first + 16):
        r, i = oracle_samples.render_sample(S, scene, W, H, O.MODE_FULL, k)
        acc += r
        if ref_id is None:
            ref_id = i
        assert np.array_equal(i, ref_id), f"id_dist of sample {k} differs"
    mean = ((acc + 8) // 16).astype(np.uint8)
    mean[..., 3] = 255
    results = [_accumulate(ctx, W, H, first, ch) for ch in ([1] * 16, [1, 3, 12], [16])]
    for rgba, idd, _ in results:
        _same(rgba, mean, f"{name} mean of 16")
        _same(idd, ref_id, f"{name} id_dist")
    assert np.any(mean != oracle_samples.render_sample(S, scene, W, H, O.MODE_FULL, first)[0])
    want_shown = O.denoise(mean, ref_id)
    for dk in (2, 3, 0):   # VRT_OPT_DISPLAY_KERNEL, the shipped setting last
        ctx.set_option(V.OPT_DISPLAY_KERNEL, dk)
        _same(ctx.accum_resolve()[2], want_shown, f"{name} shown, display kernel {dk}")


def test_opaque_and_general_paths_agree(ctx, V, O, product_scenes):
    m, W, H, pose = SCENES["dragon"]
    _setup(ctx, V, O, product_scenes, m, W, H, pose)
    assert V.tree_is_opaque(product_scenes[m][0])
    try:
        ctx.set_option(V.OPT_FULL_OPAQUE, 0)
        general = _accumulate(ctx, W, H, 11, [2, 6])
    finally:
        ctx.set_option(V.OPT_FULL_OPAQUE, 1)
    opaque = _accumulate(ctx, W, H, 11, [8])
    for a, b, what in zip(general, opaque, ("rgba8", "id_dist", "shown")):
        _same(a, b, f"general vs opaque {what}")


@pytest.mark.parametrize("key,rows", [("dragon_1080p_full/mode2", (538, 542)), ("room_inside_1080p_full/mode2", (700, 702))])
def test_full_size(ctx, V, O, S, golden, product_scenes, key, rows):
    g = golden["frames"]["frames"][key]
    W, H = g["width"], g["height"]
    scene, _ = _setup(ctx, V, O, product_scenes, g["map"], W, H, g["pose"])
    rgba, idd, _ = _accumulate(ctx, W, H, 0, [1])
    frame, frame_id = ctx.dispatch(W, H, V.MODE_FULL)
    _same(rgba, frame, f"{key} sample 0 vs vrt_dispatch")
    _same(idd, frame_id, f"{key} id_dist vs vrt_dispatch")
    assert "%016x" % V.fnv1a64(rgba) == g["rgba_fnv1a64"]
    assert "%016x" % V.fnv1a64(idd) == g["id_dist_fnv1a64"]
    r0, r1 = rows
    acc = np.zeros((r1 - r0, W, 4), np.uint64)
    for k in range(64):
        acc += oracle_samples.render_sample(S, scene, W, H, O.MODE_FULL, k, row0=r0, row1=r1)[0][r0:r1]
    mean = ((acc + 32) // 64).astype(np.uint8)
    mean[..., 3] = 255
    rgba, idd2, _ = _accumulate(ctx, W, H, 0, [64])
    _same(rgba[r0:r1], mean, f"{key} mean of 64, rows {r0}-{r1}")
    _same(idd2, frame_id, f"{key} id_dist of 64")


def test_restart_rule(ctx, V, O, product_scenes):
    m, W, H, pose = SCENES["dragon"]
    _, (ip, iv, cp) = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    ctx.accum_begin(W, H, 0)
    assert ctx.accum_add(1) == 1
    assert ctx.accum_add(2) == 3
    ctx.set_camera(ip, iv, cp)              # the same bytes again: no restart
    ctx.set_params(ctx.default_params())
    assert ctx.accum_add(1) == 4
    cp2 = np.array(cp, np.float32).copy()
    cp2[0] += np.float32(0.25)
    ctx.set_camera(ip, iv, cp2)             # moved: restart
    assert ctx.accum_add(2) == 2
    ctx.set_camera(ip, iv, cp)
    assert ctx.accum_add(1) == 1
    assert ctx.accum_add(1) == 2
    p = ctx.default_params()
    p.highlighted[:] = (40, 40, 40)
    ctx.set_params(p)                       # another uniform: restart
    assert ctx.accum_add(1) == 1
    assert ctx.accum_add(1) == 2
    ctx.patch_begin()
    with pytest.raises(V.VrtError):        # no sample inside an open patch batch
        ctx.accum_add(1)
    ctx.patch_end()                         # the tree may have changed: restart
    assert ctx.accum_add(1) == 1
    ctx.set_params(ctx.default_params())
    tex, dim = product_scenes[m]
    assert ctx.accum_add(1) == 1
    ctx.upload_octree(tex, dim)             # an upload is a tree change
    assert ctx.accum_add(3) == 3
    ctx.compact()
    assert ctx.accum_add(1) == 1
    # after all of that the resolved mean is still the mean of the samples since the last restart
    rgba, _, _ = ctx.accum_resolve()
    ref, _, _ = _accumulate(ctx, W, H, 0, [1])
    _same(rgba, ref, "after restarts")


def test_error_states(V, product_scenes):
    c = V.Context(0)
    try:
        L, h = c._L, c._h
        tot = np.zeros(1, np.uint32)
        assert L.vrt_accum_add(h, 1, None) == -5                    # before a begin
        assert L.vrt_accum_resolve(h, None, None, None) == -5
        assert L.vrt_accum_begin(h, 0, 16, 0) == -1
        c.accum_begin(64, 48, 0)
        assert L.vrt_accum_resolve(h, None, None, None) == -5       # no sample yet
        assert L.vrt_accum_add(h, 1, None) == -5                    # no scene
        m, W, H, pose = SCENES["dragon"]
        tex, dim = product_scenes[m]
        c.upload_octree(tex, dim)
        assert L.vrt_accum_add(h, 1, None) == -5                    # no camera
        ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], 64, 48)
        c.set_camera(ip, iv, cp)
        assert L.vrt_accum_add(h, 0, None) == -1                    # zero samples
        assert L.vrt_accum_add(h, 1, tot.ctypes.data_as(V.C.POINTER(V.C.c_uint32))) == 0 and tot[0] == 1
        assert L.vrt_accum_add(h, 1 << 24, None) == -1              # beyond the cap, refused before any launch
        assert L.vrt_accum_resolve_device(h, None, None, 1, None) == -1   # the display pass needs d_rgba8
        rgba, idd, shown = c.accum_resolve()
        assert rgba.shape == (48, 64, 4) and np.all(rgba[..., 3] == 255)
    finally:
        c.close()


def test_no_interference_with_frames(ctx, V, O, S, product_scenes):
    m, W, H, pose = SCENES["dragon"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    _accumulate(ctx, W, H, 3, [4])
    ref_rgba, ref_id, _, _ = O.render(scene, W, H, O.MODE_FULL)
    rgba, idd = ctx.dispatch(W, H, V.MODE_FULL)
    _same(rgba, ref_rgba, "frame after an accumulation")
    _same(idd, ref_id, "frame id_dist after an accumulation")
    shown, rgba2, _ = ctx.dispatch_frame(W, H, V.MODE_FULL)
    _same(rgba2, ref_rgba, "dispatch_frame after an accumulation")
    _same(shown, O.denoise(ref_rgba, ref_id), "shown frame after an accumulation")
