"""The gfx950 kernels against the independent float64 restatement of the shader (tests/shader_ref64.py).

The reference is computed once per frame and reused across every kernel setting: each shipped variant, the ray tables
on and off, the three empty-octant settings, texel and record uploads. Every decided pixel must agree exactly."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, MAPS, room_world, terrain_world
from test_shader_reference64 import (EDGE_CAPS, EDGE_MIN_HITS, EDGE_NAMES, POSES, TERRAIN_WINDOW, UNDECIDED_CAP, Case, check,
                                     edge_cases, light_dir_bits)
import shader_ref64 as R

pytestmark = pytest.mark.gpu

import vrt_import

VARIANTS = vrt_import.vrt().available_variants()


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def worlds(V):
    """scene name -> product World (kept open for records())"""
    out = {}
    for m in ("dragon", "monu9", "nature"):
        w = V.World()
        assert w.load_vox(os.path.join(MAPS, m + ".vox"))
        out[m] = w
    out["terrain"] = terrain_world(V, window=TERRAIN_WINDOW)
    out["room"] = room_world(V)
    yield out
    for w in out.values():
        w.close()


def _params(ctx, c):
    p = ctx.default_params()
    assert list(np.array(p.light_dir, np.float32).view(np.uint32)) == list(light_dir_bits().view(np.uint32))
    p.voxel_scale = c.scale
    p.world_min[:], p.world_max[:] = list(c.wmin), list(c.wmax)
    p.global_light[:] = [float(v) for v in c.gl]
    p.light_dir[:] = [float(v) for v in c.light]
    p.highlighted[:] = list(c.hl)
    ctx.set_params(p)
    ctx.set_camera(*c.cam)


def _settings(ctx, V, c, records=None):
    """configure every kernel setting in turn; yields its name"""
    uploads = [("texels", lambda: ctx.upload_octree(c.tex, c.dim))]
    if records is not None:
        uploads.append(("records", lambda: ctx.upload_records(*records)))
    try:
        for up, do in uploads:
            do()
            _params(ctx, c)
            for v in VARIANTS:
                ctx.set_variant(v)
                for rt in (0, 1):
                    ctx.set_ray_tables(rt)
                    for eo in (0, 1, 2):
                        ctx.set_option(V.OPT_EMPTY_OCTANTS, eo)
                        yield f"{up} variant {v} ray tables {rt} empty octants {eo}"
    finally:
        ctx.set_variant(0)
        ctx.set_ray_tables(1)
        ctx.set_option(V.OPT_EMPTY_OCTANTS, 1)
        ctx.set_params(ctx.default_params())


@pytest.mark.parametrize("scene,pose,W,H,min_hits,cap", [
    ("dragon", "dragon", 256, 144, 16000, UNDECIDED_CAP), ("dragon", "dragon_inside", 101, 67, 6000, UNDECIDED_CAP),
    ("monu9", "monu9", 256, 144, 9400, UNDECIDED_CAP), ("nature", "nature", 123, 71, 4000, UNDECIDED_CAP),
    ("terrain", "terrain", 240, 136, 1700, 0.12), ("room", "room_inside", 256, 144, 15600, UNDECIDED_CAP),
    ("room", "room_outside", 256, 144, 12200, UNDECIDED_CAP), ("room", "room_inside", 83, 49, 1700, UNDECIDED_CAP)])
def test_kernels_match_float64_reference(ctx, V, worlds, scene, pose, W, H, min_hits, cap):
    w = worlds[scene]
    tex, dim = w.flatten()
    c = Case(V, tex, dim, POSES[pose], W, H)
    tr = c.trace(R.World(tex, dim))
    frames = {m: tr.frame(m) for m in (0, 1, 2)}
    n = 0
    for what in _settings(ctx, V, c, records=w.records()):
        for mode, f in frames.items():
            rgba, idd = ctx.dispatch(W, H, mode)
            check(f, rgba, idd, min_hits, f"{scene}/{pose} {W}x{H} mode {mode} {what}", cap)
            n += 1
    assert n >= 2 * len(VARIANTS) * 6 * 3


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_kernels_on_edge_worlds(ctx, V, name):
    c, pin = edge_cases(V)[name]
    tr = c.trace(R.World(c.tex, c.dim, c.wmin, c.wmax))
    frames = {m: tr.frame(m) for m in (0, 1, 2)}
    pin(frames[1])
    for what in _settings(ctx, V, c):
        for mode, f in frames.items():
            rgba, idd = ctx.dispatch(c.W, c.H, mode)
            check(f, rgba, idd, EDGE_MIN_HITS.get(name, 1000), f"{name} mode {mode} {what}", EDGE_CAPS.get(name, UNDECIDED_CAP))


@pytest.mark.parametrize("key,min_hits,cap", [("dragon_1080p", 9000, UNDECIDED_CAP), ("monu9_720p", 2000, UNDECIDED_CAP),
                                              ("terrain_1080p", 9000, 0.12)])
def test_full_size_frames_on_a_sample(ctx, V, golden, product_scenes, key, min_hits, cap):
    """~20k seeded pixels of the frames.json poses at 1920x1080, modes 0 and 1, and the display pass (Context.denoise and
    dispatch_frame's shown frame) against the float64 quad.frag on the same pixels"""
    g = golden["frames"]["frames"][key + "/mode0"]
    tex, dim = product_scenes[g["map"]]
    W, H = 1920, 1080
    c = Case(V, tex, dim, g["pose"], W, H)
    rng = np.random.default_rng(2024)
    xs, ys = rng.integers(0, W, 20000), rng.integers(0, H, 20000)
    tr = R.Trace(R.World(tex, dim), *c.cam, W, H, xs=xs, ys=ys, light_dir=c.light)
    ctx.upload_octree(tex, dim)
    _params(ctx, c)
    try:
        for mode in (0, 1):
            f = tr.frame(mode)
            rgba, idd = ctx.dispatch(W, H, mode)
            check(f, rgba, idd, min_hits, f"{key} mode {mode}", cap)
            want, dec = R.display(rgba, idd, xs, ys)
            assert dec.mean() > 0.9
            got = ctx.denoise(rgba, idd)[ys, xs].astype(np.int64)
            assert np.array_equal(got[:, :3][dec], want[:, :3][dec]) and np.all(got[:, 3] == want[:, 3]), f"{key} mode {mode} denoise"
            shown, rgba2, idd2 = ctx.dispatch_frame(W, H, mode)
            assert np.array_equal(rgba2, rgba) and np.array_equal(idd2, idd)
            got = shown[ys, xs].astype(np.int64)
            assert np.array_equal(got[:, :3][dec], want[:, :3][dec]) and np.all(got[:, 3] == want[:, 3]), f"{key} mode {mode} shown"
    finally:
        ctx.set_params(ctx.default_params())
