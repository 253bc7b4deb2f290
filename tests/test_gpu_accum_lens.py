"""Thin-lens progressive accumulation on the MI355X (vrt_set_lens) against the checker (tests/oracle_lens.c: the oracle's frame
at lens sample k). Single samples are pinned byte for byte in all three modes, with and without jitter, on every scene shape
and upload path, under every ray-table, empty-octant and opaque-path setting and every available variant; lens poses chosen
with the dispatcher's own proofs (vrt_test_lens_select) take each one-eye shortcut on both sides. Means under any chunking,
the display pass, a 1080p frame, the restart rule, aperture 0, the error codes and frames around a lens accumulation too."""
import numpy as np
import pytest

import oracle_jitter
import oracle_lens
from test_accum_lens import _focus_world
from test_gpu_accum_jitter import SCENES, _same, _setup

pytestmark = pytest.mark.gpu

SAMPLES = (0, 1, 2, 7, 255, 2 ** 32 - 1)
MODES = (0, 1, 2)
LENS = {   # scene -> (aperture, focus distance) of the scene sweep
    "dragon": (2.0, 60.0), "monu9": (1.5, 50.0), "nature": (2.5, 90.0), "room_inside": (0.75, 20.0),
    "room_outside": (1.25, 45.0), "terrain": (6.0, 400.0),
}


@pytest.fixture(scope="module")
def LL(tmp_path_factory):
    return oracle_lens.build(tmp_path_factory.mktemp("oracle_lens"))


@pytest.fixture(scope="module")
def J(tmp_path_factory):
    return oracle_jitter.build(tmp_path_factory.mktemp("oracle_jitter"))


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _accumulate(ctx, W, H, mode, first, chunks, jitter):
    ctx.accum_begin(W, H, first, mode=mode, jitter=jitter)
    total = 0
    for n in chunks:
        total += n
        assert ctx.accum_add(n) == total
    return ctx.accum_resolve()


def _check(ctx, LL, J, O, scene, W, H, ap, focus, what, samples=SAMPLES, modes=MODES, jitters=(False, True)):
    ctx.set_lens(ap, focus)
    try:
        for mode in modes:
            _, frame_id = oracle_jitter.render(J, scene, W, H, mode, 0, jitter=False)
            for jitter in jitters:
                for k in samples:
                    ref, _ = oracle_lens.render(LL, scene, W, H, mode, k, ap, focus, jitter=jitter)
                    rgba, idd, shown = _accumulate(ctx, W, H, mode, k, [1], jitter)
                    tag = f"{what} aperture {ap} mode {mode} jitter {jitter} sample {k}"
                    _same(rgba, ref, f"{tag} rgba8")
                    _same(idd, frame_id, f"{tag} id_dist")
                    _same(shown, O.denoise(ref, frame_id), f"{tag} shown")
    finally:
        ctx.set_lens(0.0, 1.0)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_each_lens_sample_is_the_checker_sample(ctx, V, O, LL, J, product_scenes, name):
    m, W, H, pose = SCENES[name]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    ap, focus = LENS[name]
    _check(ctx, LL, J, O, scene, W, H, ap, focus, name)


def test_record_only_upload(ctx, V, O, LL, J, product_scenes):
    import os
    from conftest import MAPS
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    rec = w.records()
    w.close()
    m, W, H, pose = SCENES["dragon"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose, records=rec)
    _check(ctx, LL, J, O, scene, W, H, *LENS["dragon"], "records", samples=(0, 7, 2 ** 32 - 1))


def test_every_setting_and_variant_gives_the_same_samples(ctx, V, O, LL, product_scenes):
    m, W, H, pose = SCENES["room_outside"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    ap, focus = LENS["room_outside"]
    refs = {(mode, k, j): oracle_lens.render(LL, scene, W, H, mode, k, ap, focus, jitter=j)[0]
            for mode in MODES for k in (1, 6) for j in (False, True)}
    settings = [(V.OPT_RAY_TABLES, 0), (V.OPT_EMPTY_OCTANTS, 0), (V.OPT_EMPTY_OCTANTS, 2), (V.OPT_FULL_OPAQUE, 0)]
    defaults = {V.OPT_RAY_TABLES: 1, V.OPT_EMPTY_OCTANTS: 1, V.OPT_FULL_OPAQUE: 1}
    ctx.set_lens(ap, focus)
    try:
        for opt, val in settings:
            ctx.set_option(opt, val)
            for (mode, k, j), ref in refs.items():
                _same(_accumulate(ctx, W, H, mode, k, [1], j)[0], ref, f"option {opt}={val} mode {mode} sample {k} jitter {j}")
            ctx.set_option(opt, defaults[opt])
        for var in V.available_variants():
            ctx.set_variant(var)
            for (mode, k, j), ref in refs.items():
                _same(_accumulate(ctx, W, H, mode, k, [1], j)[0], ref, f"variant {var} mode {mode} sample {k} jitter {j}")
    finally:
        ctx.set_variant(0)
        ctx.set_lens(0.0, 1.0)
        for opt, val in defaults.items():
            ctx.set_option(opt, val)


# lens poses -> (map, W, H, pose, aperture, focus, the proofs the dispatcher must reach)
POSES = {
    "inside_one_empty_node": ("dragon", 72, 45, (63.5, 60.5, 140.5, -90.0, -10.0), 0.1, 40.0,
                              dict(eye_shared=True, first_shared=True, no_medium=True, empty=True)),
    "across_a_node_boundary": ("dragon", 72, 45, (64.0, 60.5, 140.5, -90.0, -10.0), 0.3, 40.0,
                               dict(eye_shared=True, first_shared=False)),
    "across_many_nodes": ("terrain", 72, 45, (512.5, 420.5, 1000.5, -90.0, -20.0), 3.0, 300.0,
                          dict(eye_shared=False, first_shared=False, no_medium=True, empty=True)),
    "into_the_glass": ("room", 72, 45, (14.5, 30.5, 16.5, 32.0, -10.0), 40.0, 25.0,
                       dict(eye_shared=False, no_medium=False, empty=False, root_shift=10)),
    "eye_in_a_medium": ("room", 72, 45, (31.5, 26.5, 31.5, 32.0, -10.0), 0.2, 12.0,
                        dict(eye_shared=True, no_medium=False, empty=False)),
    "medium_per_lane": ("room", 72, 45, (31.5, 26.5, 31.5, 32.0, -10.0), 3.0, 12.0,
                        dict(eye_shared=False, first_shared=False, no_medium=False)),
}


@pytest.mark.parametrize("name", sorted(POSES))
def test_both_sides_of_every_selection(ctx, V, O, LL, J, product_scenes, name):
    m, W, H, pose, ap, focus, want = POSES[name]
    scene, (ip, iv, cp) = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    got = V.lens_choice(product_scenes[m][0], cp, iv, ap)
    assert got["box_valid"] and all(got[k] == v for k, v in want.items()), f"{name}: {got}"
    _check(ctx, LL, J, O, scene, W, H, ap, focus, name, samples=(1, 2, 7, 255))


def test_opaque_scene_on_the_per_lane_side(ctx, V, O, LL, J):
    """the origins of a lens in front of a wall reach into it: an opaque tree, but not every origin in empty space -- the general
    full path tracer with per-lane media instead of the opaque chain"""
    tex, dim = _focus_world(V)
    W, H = 72, 45
    ip, iv, cp, _ = V.camera_block((20.3, 15.2, 2.1), -90.0, -40.0, W, H)
    assert V.tree_is_opaque(tex)
    got = V.lens_choice(tex, cp, iv, 3.0)
    assert got["box_valid"] and not got["empty"] and not got["eye_shared"]
    ctx.upload_octree(tex, dim)
    ctx.set_camera(ip, iv, cp)
    ctx.set_params(ctx.default_params())
    scene = O.make_scene(tex, dim, ip, iv, cp)
    _check(ctx, LL, J, O, scene, W, H, 3.0, 1.7, "opaque per lane", samples=(1, 2, 7, 255))
    ip, iv, cp, _ = V.camera_block((20.3, 15.2, 40.7), -90.0, 0.0, W, H)   # and far from the wall: the opaque chain
    assert V.lens_choice(tex, cp, iv, 3.0)["empty"]
    ctx.set_camera(ip, iv, cp)
    _check(ctx, LL, J, O, O.make_scene(tex, dim, ip, iv, cp), W, H, 3.0, 39.7, "opaque chain", samples=(1, 7), modes=(2,))


@pytest.mark.parametrize("name", ["dragon", "room_outside"])
def test_means_chunking_and_display_pass(ctx, V, O, LL, J, product_scenes, name):
    m, W, H, pose = SCENES[name]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    ap, focus = LENS[name]
    first = 5
    ctx.set_lens(ap, focus)
    try:
        for mode in MODES:
            jitter = mode != 1
            acc = np.zeros((H, W, 4), np.uint64)
            for k in range(first, first + 16):
                acc += oracle_lens.render(LL, scene, W, H, mode, k, ap, focus, jitter=jitter)[0]
            mean = ((acc + 8) // 16).astype(np.uint8)
            mean[..., 3] = 255
            _, frame_id = oracle_jitter.render(J, scene, W, H, mode, 0, jitter=False)
            for chunks in ([16], [1, 15], [4, 4, 4, 4]):
                rgba, idd, shown = _accumulate(ctx, W, H, mode, first, chunks, jitter)
                _same(rgba, mean, f"{name} mode {mode} mean of 16 as {chunks}")
                _same(idd, frame_id, f"{name} mode {mode} id_dist")
                _same(shown, O.denoise(mean, frame_id), f"{name} mode {mode} shown")
    finally:
        ctx.set_lens(0.0, 1.0)


def test_full_size(ctx, V, O, LL, product_scenes):
    m, _, _, pose = SCENES["dragon"]
    W, H = 1920, 1080
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    r0, r1 = 537, 541
    ap, focus = LENS["dragon"]
    ctx.set_lens(ap, focus)
    try:
        for mode in MODES:
            frame, frame_id = ctx.dispatch(W, H, mode)
            acc = np.zeros((r1 - r0, W, 4), np.uint64)
            for k in range(4):
                acc += oracle_lens.render(LL, scene, W, H, mode, k, ap, focus, jitter=True, row0=r0, row1=r1)[0][r0:r1]
            mean = ((acc + 2) // 4).astype(np.uint8)
            mean[..., 3] = 255
            rgba, idd, _ = _accumulate(ctx, W, H, mode, 0, [4], True)
            _same(rgba[r0:r1], mean, f"mode {mode} mean of 4, rows {r0}-{r1}")
            _same(idd, frame_id, f"mode {mode} id_dist vs vrt_dispatch")
            rgba1, _, _ = _accumulate(ctx, W, H, mode, 0, [1], True)
            _same(rgba1, frame, f"mode {mode} lens sample 0 vs vrt_dispatch")
    finally:
        ctx.set_lens(0.0, 1.0)


def test_aperture_zero_is_the_lens_free_accumulation(ctx, V, O, product_scenes):
    m, W, H, pose = SCENES["room_inside"]
    _setup(ctx, V, O, product_scenes, m, W, H, pose)
    for mode in MODES:
        for jitter in (False, True):
            ref = _accumulate(ctx, W, H, mode, 9, [3, 5], jitter)
            ctx.set_lens(0.0, 17.0)
            try:
                got = _accumulate(ctx, W, H, mode, 9, [3, 5], jitter)
            finally:
                ctx.set_lens(0.0, 1.0)
            for a, b, what in zip(ref, got, ("rgba8", "id_dist", "shown")):
                _same(b, a, f"mode {mode} jitter {jitter} aperture 0: {what}")


def test_restart_rule(ctx, V, O, LL, product_scenes):
    m, W, H, pose = SCENES["dragon"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    ctx.set_lens(1.0, 30.0)
    try:
        ctx.accum_begin(W, H, 4, mode=V.MODE_PRIMARY, jitter=True)
        assert ctx.accum_add(1) == 1
        assert ctx.accum_add(2) == 3
        ctx.set_lens(1.0, 30.0)               # the same lens again: no restart
        assert ctx.accum_add(1) == 4
        ctx.set_lens(1.0, 31.0)               # a new focus distance: restart at `first`
        assert ctx.accum_add(1) == 1
        rgba, _, _ = ctx.accum_resolve()
        _same(rgba, oracle_lens.render(LL, scene, W, H, O.MODE_PRIMARY, 4, 1.0, 31.0, jitter=True)[0], "sample 4 after the restart")
        ctx.set_lens(2.0, 31.0)               # a new aperture: restart
        assert ctx.accum_add(2) == 2
        ctx.set_lens(0.0, 31.0)               # and off
        assert ctx.accum_add(1) == 1
    finally:
        ctx.set_lens(0.0, 1.0)


def test_error_codes(V):
    c = V.Context(0)
    try:
        L, h = c._L, c._h
        for ap, f in ((-1.0, 5.0), (float("nan"), 5.0), (float("inf"), 5.0), (-float("inf"), 5.0), (1.0, 0.0), (1.0, -0.0),
                      (1.0, -3.0), (1.0, float("nan")), (1.0, float("inf"))):
            assert L.vrt_set_lens(h, ap, f) == -1, (ap, f)
        assert L.vrt_set_lens(None, 1.0, 5.0) == -1
        assert L.vrt_set_lens(h, 0.0, 1.0) == 0 and L.vrt_set_lens(h, 2.5, 1e-3) == 0
    finally:
        c.close()


def test_frames_and_lens_free_accumulations_around_a_lens_accumulation(ctx, V, O, product_scenes):
    m, W, H, pose = SCENES["room_outside"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    plain = {mode: _accumulate(ctx, W, H, mode, 3, [4], True) for mode in MODES}
    ctx.set_lens(*LENS["room_outside"])
    try:
        for mode in MODES:
            _accumulate(ctx, W, H, mode, 3, [2, 2], True)
            ref_rgba, ref_id, _, _ = O.render(scene, W, H, mode)
            rgba, idd = ctx.dispatch(W, H, mode)            # frames stay pinhole with a lens set
            _same(rgba, ref_rgba, f"mode {mode} frame with a lens set")
            _same(idd, ref_id, f"mode {mode} frame id_dist with a lens set")
    finally:
        ctx.set_lens(0.0, 1.0)
    for mode in MODES:
        again = _accumulate(ctx, W, H, mode, 3, [4], True)
        for a, b, what in zip(plain[mode], again, ("rgba8", "id_dist", "shown")):
            _same(b, a, f"mode {mode} lens-free accumulation around a lens one: {what}")
