"""The gfx950 kernels' VRT_MODE_FULL against the independent float64 restatement of pathTrace (tests/path_ref64.py).

The reference is traced once per frame and reused across every route of the mode: each shipped variant (the v2 / v1
record fall-backs through a tree with an internal unit cell), VRT_OPT_FULL_OPAQUE 0, 1, 5, 6 and 7, ray tables on and off,
texel and record uploads, single accumulation samples at chosen initRNG indices and one 4-sample accumulation through
the looped kernel. Every decided pixel must agree exactly. The det_* routines are measured on the device as well."""
import numpy as np
import pytest

from test_gpu_reference64 import _params, ctx, worlds  # noqa: F401
from test_path_reference64 import SAMPLES, assert_det_bounds, check, det_errors, glass_cases, trace
from test_shader_reference64 import POSES, Case
import path_ref64 as PR
import shader_ref64 as R

pytestmark = pytest.mark.gpu

import vrt_import

VARIANTS = vrt_import.vrt().available_variants()
FORMS = (0, 1, 5, 6, 7)            # VRT_OPT_FULL_OPAQUE


def test_det_routines_on_device_against_float64(ctx):
    f = lambda op: (lambda x, y=None: ctx.debug_math(op, x, x if y is None else y))
    assert_det_bounds(det_errors(f(6), lambda x, y: ctx.debug_math(12, x, y), f(10), f(11)))


# (scene, pose, W, H, min decided hits, undecided cap, opaque)
FRAMES = [("dragon", "dragon", 256, 144, 16700, 0.015, True), ("nature", "nature", 160, 90, 6400, 0.01, True),
          ("room", "room_inside", 256, 144, 32400, 0.04, False), ("room", "room_outside", 160, 90, 5200, 0.01, False)]


@pytest.mark.parametrize("scene,pose,W,H,min_hits,cap,opaque", FRAMES)
def test_full_mode_routes_match_path_reference(ctx, V, worlds, scene, pose, W, H, min_hits, cap, opaque):
    w = worlds[scene]
    tex, dim = w.flatten()
    c = Case(V, tex, dim, POSES[pose], W, H)
    f = trace(c, R.World(tex, dim))
    n = 0
    try:
        for up, do in (("texels", lambda: ctx.upload_octree(tex, dim)), ("records", lambda: ctx.upload_records(*w.records()))):
            do()
            _params(ctx, c)
            for v in VARIANTS:
                ctx.set_variant(v)
                for rt in (0, 1):
                    ctx.set_ray_tables(rt)
                    for form in (FORMS if opaque and v == 0 else (6,)):
                        ctx.set_option(V.OPT_FULL_OPAQUE, form)
                        rgba, idd = ctx.dispatch(W, H, 2)
                        check(f, rgba, idd, min_hits, cap, f"{scene}/{pose} {up} variant {v} ray tables {rt} opaque form {form}")
                        n += 1
    finally:
        ctx.set_variant(0)
        ctx.set_ray_tables(1)
        ctx.set_option(V.OPT_FULL_OPAQUE, 6)
        ctx.set_params(ctx.default_params())
    want = 2 * 2 * (len(VARIANTS) - 1 + (len(FORMS) if opaque else 1))
    assert n == want, (n, want)


def _tx(ptr, mask):
    return [ptr & 255, (ptr >> 8) & 255, (ptr >> 16) & 255, mask]


def test_record_fallbacks_on_a_tree_with_an_internal_unit_cell(ctx, V):
    """test_gpu_parity's world [0,8)^3 whose unit cell [4,5)^3 is an internal node: no wide layout, so the dispatcher takes
    the explicit-box kernels (the v2 / v1 fall-backs) for every variant"""
    leaf = [200, 40, 90, 255, 255, 0, 0, 255]
    tex = np.array(_tx(1, 0x80) + _tx(2, 0) + _tx(3, 0x01) + _tx(4, 0) + _tx(5, 0x01) + _tx(6, 0) + _tx(7, 0x80) +
                   _tx(8 | 0x800000, 0) + leaf, np.uint8)
    c = Case(V, tex, 3, (1.3, 2.1, 0.7, 52.0, 18.0), 64, 48, wmin=(0, 0, 0), wmax=(8, 8, 8))
    f = trace(c, R.World(tex, 3, c.wmin, c.wmax))
    ctx.upload_octree(tex, 3)
    n = 0
    try:
        _params(ctx, c)
        for v in VARIANTS:
            ctx.set_variant(v)
            rgba, idd = ctx.dispatch(c.W, c.H, 2)
            check(f, rgba, idd, 20, 0.1, f"unit-internal variant {v}")
            n += 1
    finally:
        ctx.set_variant(0)
        ctx.set_params(ctx.default_params())
    assert n == len(VARIANTS) and len(VARIANTS) > 1


@pytest.mark.parametrize("name", ["panes", "grazing_exit", "block_scale_2.0", "bounce_only", "eye_in_glass", "pane_order"])
def test_glass_edge_worlds_on_device(ctx, V, name):
    c, pin, min_hits, cap = glass_cases(V)[name]
    f = trace(c, R.World(c.tex, c.dim, c.wmin, c.wmax))
    pin(f)
    ctx.upload_octree(c.tex, c.dim)
    n = 0
    try:
        _params(ctx, c)
        for v in VARIANTS:
            ctx.set_variant(v)
            rgba, idd = ctx.dispatch(c.W, c.H, 2)
            check(f, rgba, idd, min_hits, cap, f"{name} variant {v}")
            n += 1
    finally:
        ctx.set_variant(0)
        ctx.set_params(ctx.default_params())
    assert n == len(VARIANTS)


@pytest.mark.parametrize("scene,pose,W,H,min_hits", [("dragon", "dragon", 97, 55, 2450), ("room", "room_inside", 83, 49, 3580)])
def test_accumulated_samples_match_path_reference(ctx, V, worlds, scene, pose, W, H, min_hits):
    """one sample at a time from accum_begin(first_sample=k), then one 4-sample accum_add through the looped kernel:
    (sum of the four reference bytes + 2) // 4 where all four samples are decided"""
    w = worlds[scene]
    tex, dim = w.flatten()
    c = Case(V, tex, dim, POSES[pose], W, H)
    world = R.World(tex, dim)
    ctx.upload_octree(tex, dim)
    n = 0
    try:
        _params(ctx, c)
        for k in SAMPLES:
            f = trace(c, world, sample=k)
            ctx.accum_begin(W, H, first_sample=k, mode=2)
            assert ctx.accum_add(1) == 1
            rgba, idd, _ = ctx.accum_resolve()
            check(f, rgba, idd, min_hits, 0.04, f"{scene} sample {k}")
            n += 1
        first = 7
        fr = [trace(c, world, sample=first + i) for i in range(4)]
        ctx.accum_begin(W, H, first_sample=first, mode=2)
        assert ctx.accum_add(4) == 4
        rgba, idd, _ = ctx.accum_resolve()
        dec = np.all([f.dec_rgb.all(1) & f.dec_id for f in fr], axis=0)
        want = (sum(f.rgba[:, :3] for f in fr) + 2) // 4
        got = rgba[fr[0].ys, fr[0].xs, :3].astype(np.int64)
        assert dec.sum() > 0.85 * dec.size, dec.mean()
        assert np.array_equal(got[dec], want[dec]), np.argwhere(np.any(got != want, 1) & dec)[:5]
        ok_id = np.all([f.dec_id & f.dec_dist for f in fr], axis=0)
        assert np.array_equal(idd[fr[0].ys, fr[0].xs][ok_id], np.stack([fr[0].id, fr[0].dist], 1)[ok_id])
    finally:
        ctx.set_params(ctx.default_params())
    assert n == len(SAMPLES)


@pytest.mark.parametrize("key,min_hits,cap", [("dragon_1080p_full", 9100, 0.015), ("room_inside_1080p_full", 17600, 0.04)])
def test_full_size_frames_on_a_sample(ctx, V, golden, product_scenes, key, min_hits, cap):
    """~20k seeded pixels of the 1920x1080 mode-2 golden poses"""
    g = golden["frames"]["frames"][key + "/mode2"]
    tex, dim = product_scenes[g["map"]]
    W, H = 1920, 1080
    c = Case(V, tex, dim, g["pose"], W, H)
    rng = np.random.default_rng(2026)
    xs, ys = rng.integers(0, W, 20000), rng.integers(0, H, 20000)
    f = PR.PathTrace(R.World(tex, dim), *c.cam, W, H, xs=xs, ys=ys, light_dir=c.light).frame()
    ctx.upload_octree(tex, dim)
    try:
        _params(ctx, c)
        rgba, idd = ctx.dispatch(W, H, 2)
        check(f, rgba, idd, min_hits, cap, key)
    finally:
        ctx.set_params(ctx.default_params())

