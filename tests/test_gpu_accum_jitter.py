"""Anti-aliased progressive accumulation on the MI355X (vrt_accum_begin_ex with VRT_ACCUM_JITTER, and modes 0 / 1) against the
checker (tests/oracle_jitter.c: the oracle's frame at jittered sample k). Single samples are pinned byte for byte in all three
modes on every scene shape and upload path, under every ray-table, empty-octant and opaque-path setting and every available
variant; so are means under any chunking, the display pass, 1080p row bands, the restart rule, the error codes and frames
around an accumulation."""
import os

import numpy as np
import pytest

import oracle_jitter
from conftest import MAPS

pytestmark = pytest.mark.gpu

SAMPLES = (0, 1, 2, 7, 255, 2 ** 32 - 1)
SCENES = {   # name -> (map, W, H, pose); sizes that are not multiples of 8
    "dragon": ("dragon", 100, 61, (63.5, 60.5, 140.5, -90.0, -10.0)),
    "monu9": ("monu9", 90, 53, (48.5, 60.5, 170.5, -90.0, -12.0)),
    "nature": ("nature", 94, 57, (60.5, 80.5, 200.5, -90.0, -20.0)),
    "room_inside": ("room", 100, 61, (14.5, 30.5, 16.5, 32.0, -10.0)),
    "room_outside": ("room", 100, 61, (98.5, 34.5, 52.5, 197.0, -8.0)),
    "terrain": ("terrain", 98, 59, (512.5, 420.5, 1000.5, -90.0, -20.0)),
}
MODES = (0, 1, 2)


@pytest.fixture(scope="module")
def J(tmp_path_factory):
    return oracle_jitter.build(tmp_path_factory.mktemp("oracle_jitter"))


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


def _accumulate(ctx, W, H, mode, first, chunks, jitter=True):
    ctx.accum_begin(W, H, first, mode=mode, jitter=jitter)
    total = 0
    for n in chunks:
        total += n
        assert ctx.accum_add(n) == total
    return ctx.accum_resolve()


def _check_samples(ctx, J, O, scene, W, H, what, samples=SAMPLES, modes=MODES):
    for mode in modes:
        _, frame_id = oracle_jitter.render(J, scene, W, H, mode, 0, jitter=False)
        for k in samples:
            ref_rgba, _ = oracle_jitter.render(J, scene, W, H, mode, k)
            rgba, idd, shown = _accumulate(ctx, W, H, mode, k, [1])
            _same(rgba, ref_rgba, f"{what} mode {mode} sample {k} rgba8")
            _same(idd, frame_id, f"{what} mode {mode} sample {k} id_dist")
            _same(shown, O.denoise(ref_rgba, frame_id), f"{what} mode {mode} sample {k} shown")


@pytest.mark.parametrize("name", sorted(SCENES))
def test_each_jittered_sample_is_the_checker_sample(ctx, V, O, J, product_scenes, name):
    m, W, H, pose = SCENES[name]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    _check_samples(ctx, J, O, scene, W, H, name)


def test_record_only_upload(ctx, V, O, J, product_scenes):
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    rec = w.records()
    w.close()
    m, W, H, pose = SCENES["dragon"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose, records=rec)
    _check_samples(ctx, J, O, scene, W, H, "records", samples=(0, 7, 2 ** 32 - 1))


def test_every_setting_and_variant_gives_the_same_samples(ctx, V, O, J, product_scenes):
    m, W, H, pose = SCENES["dragon"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    refs = {(mode, k): oracle_jitter.render(J, scene, W, H, mode, k)[0] for mode in MODES for k in (1, 6)}
    settings = [(V.OPT_RAY_TABLES, 0), (V.OPT_EMPTY_OCTANTS, 0), (V.OPT_EMPTY_OCTANTS, 2), (V.OPT_FULL_OPAQUE, 0)]
    defaults = {V.OPT_RAY_TABLES: 1, V.OPT_EMPTY_OCTANTS: 1, V.OPT_FULL_OPAQUE: 1}
    try:
        for opt, val in settings:
            ctx.set_option(opt, val)
            for (mode, k), ref in refs.items():
                _same(_accumulate(ctx, W, H, mode, k, [1])[0], ref, f"option {opt}={val} mode {mode} sample {k}")
            ctx.set_option(opt, defaults[opt])
        for var in V.available_variants():
            ctx.set_variant(var)
            for (mode, k), ref in refs.items():
                _same(_accumulate(ctx, W, H, mode, k, [1])[0], ref, f"variant {var} mode {mode} sample {k}")
    finally:
        ctx.set_variant(0)
        for opt, val in defaults.items():
            ctx.set_option(opt, val)


@pytest.mark.parametrize("name", ["dragon", "room_outside"])
def test_means_chunking_and_display_pass(ctx, V, O, J, product_scenes, name):
    m, W, H, pose = SCENES[name]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    first = 5
    for mode in MODES:
        acc = np.zeros((H, W, 4), np.uint64)
        for k in range(first, first + 16):
            acc += oracle_jitter.render(J, scene, W, H, mode, k)[0]
        mean = ((acc + 8) // 16).astype(np.uint8)
        mean[..., 3] = 255
        _, frame_id = oracle_jitter.render(J, scene, W, H, mode, 0, jitter=False)
        for chunks in ([16], [1, 15], [4, 4, 4, 4]):
            rgba, idd, shown = _accumulate(ctx, W, H, mode, first, chunks)
            _same(rgba, mean, f"{name} mode {mode} mean of 16 as {chunks}")
            _same(idd, frame_id, f"{name} mode {mode} id_dist")
            _same(shown, O.denoise(mean, frame_id), f"{name} mode {mode} shown")
        assert np.any(mean != oracle_jitter.render(J, scene, W, H, mode, first)[0]), "the mean should differ from one sample"


@pytest.mark.parametrize("name", ["dragon", "nature"])
def test_full_size(ctx, V, O, J, product_scenes, name):
    m, _, _, pose = SCENES[name]
    W, H = 1920, 1080
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    r0, r1 = 537, 541
    for mode in MODES:
        frame, frame_id = ctx.dispatch(W, H, mode)
        acc = np.zeros((r1 - r0, W, 4), np.uint64)
        for k in range(4):
            acc += oracle_jitter.render(J, scene, W, H, mode, k, row0=r0, row1=r1)[0][r0:r1]
        mean = ((acc + 2) // 4).astype(np.uint8)
        mean[..., 3] = 255
        rgba, idd, _ = _accumulate(ctx, W, H, mode, 0, [4])
        _same(rgba[r0:r1], mean, f"{name} mode {mode} mean of 4, rows {r0}-{r1}")
        _same(idd, frame_id, f"{name} mode {mode} id_dist vs vrt_dispatch")
        rgba1, _, _ = _accumulate(ctx, W, H, mode, 0, [1])
        _same(rgba1, frame, f"{name} mode {mode} jittered sample 0 vs vrt_dispatch")


def test_unjittered_primary_modes_resolve_to_the_frame(ctx, V, O, product_scenes):
    for name in ("dragon", "room_inside"):
        m, W, H, pose = SCENES[name]
        _setup(ctx, V, O, product_scenes, m, W, H, pose)
        for mode in (0, 1):
            frame, frame_id = ctx.dispatch(W, H, mode)
            for first, chunks in ((0, [1]), (9, [3, 5]), (2 ** 32 - 1, [16])):
                rgba, idd, shown = _accumulate(ctx, W, H, mode, first, chunks, jitter=False)
                _same(rgba, frame, f"{name} mode {mode} unjittered {chunks}")
                _same(idd, frame_id, f"{name} mode {mode} unjittered id_dist")
                _same(shown, O.denoise(frame, frame_id), f"{name} mode {mode} unjittered shown")


def test_restart_rule_and_begin_ex_restarts(ctx, V, O, J, product_scenes):
    m, W, H, pose = SCENES["dragon"]
    scene, (ip, iv, cp) = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    ctx.accum_begin(W, H, 0, mode=V.MODE_PRIMARY_SHADOW, jitter=True)
    assert ctx.accum_add(1) == 1
    assert ctx.accum_add(2) == 3
    ctx.set_camera(ip, iv, cp)               # the same bytes: no restart
    assert ctx.accum_add(1) == 4
    cp2 = np.array(cp, np.float32).copy()
    cp2[1] += np.float32(0.5)
    ctx.set_camera(ip, iv, cp2)              # moved: restart, and the frame's id_dist is the new one
    assert ctx.accum_add(2) == 2
    _, idd, _ = ctx.accum_resolve()
    _same(idd, ctx.dispatch(W, H, V.MODE_PRIMARY_SHADOW)[1], "id_dist after a restart")
    ctx.set_camera(ip, iv, cp)
    assert ctx.accum_add(1) == 1
    ctx.patch_begin()
    with pytest.raises(V.VrtError):         # no sample inside an open patch batch
        ctx.accum_add(1)
    ctx.patch_end()
    assert ctx.accum_add(1) == 1             # the tree may have changed: restart
    ctx.accum_begin(W, H, 3, mode=V.MODE_FULL, jitter=True)   # begin_ex restarts with its own mode and flags
    assert ctx.accum_add(1) == 1
    rgba, idd, _ = ctx.accum_resolve()
    ref, _ = oracle_jitter.render(J, scene, W, H, O.MODE_FULL, 3)
    _same(rgba, ref, "full sample 3 after a restart in another mode")
    _same(idd, oracle_jitter.render(J, scene, W, H, O.MODE_FULL, 0, jitter=False)[1], "full id_dist")


def test_error_codes(V, product_scenes):
    c = V.Context(0)
    try:
        L, h = c._L, c._h
        assert L.vrt_accum_begin_ex(h, 64, 48, 3, 0, 0) == -1       # unknown mode
        assert L.vrt_accum_begin_ex(h, 64, 48, -1, 0, 1) == -1
        assert L.vrt_accum_begin_ex(h, 64, 48, 2, 0, 2) == -1       # unknown flag
        assert L.vrt_accum_begin_ex(h, 64, 48, 0, 0, 0x80000001) == -1
        assert L.vrt_accum_begin_ex(h, 0, 48, 0, 0, 1) == -1        # the frame checks of vrt_accum_begin
        assert L.vrt_accum_add(h, 1, None) == -5                    # nothing begun by the refused calls
        assert L.vrt_accum_begin_ex(h, 64, 48, 1, 0, 1) == 0
        assert L.vrt_accum_resolve(h, None, None, None) == -5       # no sample yet
        assert L.vrt_accum_add(h, 1, None) == -5                    # no scene
        m, W, H, pose = SCENES["dragon"]
        tex, dim = product_scenes[m]
        c.upload_octree(tex, dim)
        assert L.vrt_accum_add(h, 1, None) == -5                    # no camera
        ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], 64, 48)
        c.set_camera(ip, iv, cp)
        assert L.vrt_accum_add(h, 0, None) == -1                    # zero samples
        assert L.vrt_accum_add(h, 1, None) == 0
        assert L.vrt_accum_add(h, 1 << 24, None) == -1              # beyond the cap
        c.patch_begin()
        assert L.vrt_accum_add(h, 1, None) == -5                    # inside an open patch batch
        c.patch_end()
        assert L.vrt_accum_add(h, 1, None) == 0
        rgba = np.zeros((48, 64, 4), np.uint8)
        assert L.vrt_accum_resolve(h, rgba.ctypes.data, None, None) == 0 and np.all(rgba[..., 3] == 255)
    finally:
        c.close()


def test_frames_and_unjittered_accumulations_around_jittered_ones(ctx, V, O, J, product_scenes):
    m, W, H, pose = SCENES["room_outside"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    plain = _accumulate(ctx, W, H, V.MODE_FULL, 3, [4], jitter=False)
    for mode in MODES:
        _accumulate(ctx, W, H, mode, 3, [2, 2])
        ref_rgba, ref_id, _, _ = O.render(scene, W, H, mode)
        rgba, idd = ctx.dispatch(W, H, mode)
        _same(rgba, ref_rgba, f"mode {mode} frame after a jittered accumulation")
        _same(idd, ref_id, f"mode {mode} frame id_dist after a jittered accumulation")
        shown, rgba2, _ = ctx.dispatch_frame(W, H, mode)
        _same(rgba2, ref_rgba, f"mode {mode} dispatch_frame after a jittered accumulation")
        _same(shown, O.denoise(ref_rgba, ref_id), f"mode {mode} shown frame")
    again = _accumulate(ctx, W, H, V.MODE_FULL, 3, [4], jitter=False)
    for a, b, what in zip(plain, again, ("rgba8", "id_dist", "shown")):
        _same(a, b, f"unjittered full accumulation around jittered ones: {what}")
