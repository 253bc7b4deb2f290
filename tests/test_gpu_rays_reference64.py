"""vrt_shade_rays, vrt_shade_rays_hdr and the HDR accumulation on the gfx950 kernels against the independent float64
restatements (tests/shader_ref64.py, tests/path_ref64.py), on the batches, caps and bounds of tests/test_rays_reference64.py.

The references are traced once per batch and sample (the Batch objects keep them) and reused across every route: each
shipped variant, texel and record uploads, a patch plus compaction, the host and the device form, caller sums, every batch
shape at which the kernels' lane-to-ray map or launch plan changes, and the accumulation's resolve on the host and on the
device. Decided rays are exact in bytes, ID and dist; floats lie within the reference's bound."""
import numpy as np
import pytest

import oracle_rays
import shader_ref64 as R
from test_gpu_shade_rays import _most_hit_voxels
from test_path_reference64 import SAMPLES
from test_rays_reference64 import (ALL, FRAMES, MEAN_FIRST, MEAN_N, MODES, TONEMAPS, Batch, batch, check_adaptive, check_bytes,
                                   check_floats, check_tonemapped, samples_of)
from test_shader_reference64 import light_dir_bits, scenes  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32

import vrt_import

VARIANTS = vrt_import.vrt().available_variants()


@pytest.fixture(scope="module")
def RR(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_rays_gpu_ref64"))   # o_frame_rays only: a frame's rays


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _params(ctx, b):
    p = ctx.default_params()
    assert list(np.array(p.light_dir, np.float32).view(np.uint32)) == list(light_dir_bits().view(np.uint32))
    p.voxel_scale = b.scale
    p.world_min[:], p.world_max[:] = list(b.wmin), list(b.wmax)
    p.global_light[:] = [float(v) for v in b.gl]
    p.light_dir[:] = [float(v) for v in b.light]
    ctx.set_params(p)
    if b.cam is not None:
        ctx.set_camera(*b.cam)


def _restore(ctx):
    ctx.set_variant(0)
    ctx.set_params(ctx.default_params())


# ---- vrt_shade_rays ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_shade_rays_routes_match_the_references(ctx, V, O, RR, scenes, name):
    """all three modes, every variant, texel and record uploads"""
    b = batch(name, V, O, RR, scenes)
    frames = {(mode, k): b.frame(mode, k) for mode in MODES for k in samples_of(name, mode)}
    w = b.make_world()
    n = 0
    try:
        for up, do in (("texels", lambda: ctx.upload_octree(b.tex, b.dim)), ("records", lambda: ctx.upload_records(*w.records()))):
            do()
            _params(ctx, b)
            for v in (VARIANTS if up == "texels" else VARIANTS[:1]):
                ctx.set_variant(v)
                for (mode, k), f in frames.items():
                    rgba, idd = ctx.shade_rays(b.o, b.d, mode, width=b.width, first_sample=k)
                    check_bytes(f, rgba, idd, name, mode, f"{name} {up} variant {v} mode {mode} sample {k}")
                    n += 1
    finally:
        w.close()
        _restore(ctx)
    assert n == (len(VARIANTS) + 1) * len(frames)


def test_shade_rays_after_a_patch_and_compaction(ctx, V, O, RR, scenes):
    """voxels the rays hit are removed by patches; the reference is retraced on the edited world"""
    b = batch("dragon_mix", V, O, RR, scenes)
    w = b.make_world()
    try:
        ctx.upload_octree(b.tex, b.dim)
        _params(ctx, b)
        before = ctx.shade_rays(b.o, b.d, 1, width=b.width)[0]
        for x, y, z in _most_hit_voxels(ctx, b.o, b.d, 30):
            w.remove(x, y, z)
            if ctx.patch_voxel(w, x, y, z) is None:
                ctx.upload_octree(*w.flatten())
        e = Batch(*w.flatten(), b.o, b.d, b.width)
        assert not np.array_equal(before, ctx.shade_rays(b.o, b.d, 1, width=b.width)[0]), "the edit changed no ray"
        for what in ("after the patches", "after compaction"):
            for mode in MODES:
                rgba, idd = ctx.shade_rays(b.o, b.d, mode, width=b.width, first_sample=1)
                check_bytes(e.frame(mode, 1), rgba, idd, "dragon_mix", mode, f"dragon_mix {what} mode {mode}")
            ctx.compact()
    finally:
        w.close()
        _restore(ctx)


# ---- vrt_shade_rays_hdr -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_shade_rays_hdr_floats_and_means(ctx, V, O, RR, scenes, name):
    b = batch(name, V, O, RR, scenes)
    try:
        ctx.upload_octree(b.tex, b.dim)
        _params(ctx, b)
        for mode in MODES:
            k = samples_of(name, mode)[0]
            rgb, rgba, idd = ctx.shade_rays_hdr(b.o, b.d, mode, width=b.width, first_sample=k)
            want, bound, dec = b.radiance(mode, k)
            check_floats(rgb, want, bound, dec, f"{name} mode {mode} sample {k}")
            check_bytes(b.frame(mode, k), rgba, idd, name, mode, f"{name} hdr bytes mode {mode} sample {k}")
        if name in ("materials_1", "room_mix"):
            for mode in (1, 2):
                mean, bound, dec = b.mean(mode, MEAN_FIRST, MEAN_N)
                for op, e in TONEMAPS:
                    rgb, rgba, _ = ctx.shade_rays_hdr(b.o, b.d, mode, width=b.width, first_sample=MEAN_FIRST, n_samples=MEAN_N,
                                                      tonemap=op, exposure=e)
                    check_floats(rgb, mean, bound, dec, f"{name} mode {mode} mean of {MEAN_N}")
                    check_tonemapped(rgba, mean, bound, dec, op, e, f"{name} mode {mode} {op} x{e}")
    finally:
        _restore(ctx)


def test_device_form_with_caller_sums(ctx, V, O, RR, scenes):
    """3 + 5 samples through d_sums / n_prior: the sums within n x bound of the reference's sum, the mean of the 8"""
    b = batch("materials_1", V, O, RR, scenes)
    n = len(b.d)
    bufs = [ctx.device_alloc(b.o.nbytes), ctx.device_alloc(b.d.nbytes), ctx.device_alloc(n * 24), ctx.device_alloc(n * 12),
            ctx.device_alloc(n * 4)]
    d_o, d_d, d_sums, d_rgb, d_rgba = bufs
    try:
        ctx.upload_octree(b.tex, b.dim)
        _params(ctx, b)
        ctx.device_write(d_o, b.o)
        ctx.device_write(d_d, b.d)
        ctx.device_write(d_sums, np.zeros((n, 3), np.float64))
        kw = dict(mode=2, width=b.width, tonemap="reinhard", exposure=0.25)
        done = 0
        for count in (3, 5):
            ctx.shade_rays_hdr_device(n, d_o, 3, d_d, d_rgb, d_rgba, None, d_sums, done, first_sample=MEAN_FIRST + done, n_samples=count, **kw)
            done += count
            sums = ctx.device_read(d_sums, (n, 3), np.float64)
            mean, bound, dec = b.mean(2, MEAN_FIRST, done)
            assert np.isfinite(sums[dec]).all()
            assert np.all(np.abs(sums - done * mean)[dec] <= done * bound[dec]), f"sums after {done} samples"
        check_floats(ctx.device_read(d_rgb, (n, 3), F), mean, bound, dec, "3 + 5 through the sums")
        check_tonemapped(ctx.device_read(d_rgba, (n, 4), np.uint8), mean, bound, dec, "reinhard", 0.25, "3 + 5 through the sums")
    finally:
        for p in bufs:
            ctx.device_free(p)
        _restore(ctx)


# ---- batch shapes ---------------------------------------------------------------------------------------------------------------
# (n, width): lists of 1, 63, 64 and 65 rays (one wave and its neighbours), width 1 and 7 (lists), 8 wide with two full rows
# plus 3 rays (tiled, a partial last row), 13 wide with 13 * 9 + 5 rays (partial tiles on both edges), a width above n
SHAPES = [(1, 1), (63, 63), (64, 64), (65, 65), (300, 1), (300, 7), (19, 8), (13 * 9 + 5, 13), (300, 5000)]


def test_batch_shapes(ctx, V, O, RR, scenes):
    b = batch("materials_1", V, O, RR, scenes)
    inw = np.nonzero(~b.trace(0).outside)[0][:300]
    o, d = np.ascontiguousarray(b.o[inw]), np.ascontiguousarray(b.d[inw])
    checked = 0
    try:
        ctx.upload_octree(b.tex, b.dim)
        _params(ctx, b)
        plain = {mode: ctx.shade_rays(o, d, mode, width=300) for mode in (0, 1)}
        for n, width in SHAPES:
            for stride in (3, 0):
                oo = o[:n] if stride == 3 else np.ascontiguousarray(np.tile(o[0], (n, 1)))
                for mode in (0, 1):      # no random number: the shape changes nothing
                    got = ctx.shade_rays(oo if stride == 3 else o[0], d[:n], mode, width=width)
                    if stride == 3:
                        assert np.array_equal(got[0], plain[mode][0][:n]) and np.array_equal(got[1], plain[mode][1][:n]), (n, width, mode)
                    else:
                        same = ctx.shade_rays(oo, d[:n], mode, width=width)
                        assert np.array_equal(got[0], same[0]) and np.array_equal(got[1], same[1]), (n, width, mode, "stride 0")
                for mode in (1, 2):      # the reference at the shape's own RNG pixels
                    f = b.frame(mode, 5, o=oo, d=d[:n], width=width)
                    rgba, idd = ctx.shade_rays(oo if stride == 3 else o[0], d[:n], mode, width=width, first_sample=5)
                    r = R.compare(f, rgba, idd)
                    assert r["bad"] == 0, (n, width, stride, mode, r)
                    want, bound, dec = b.radiance(mode, 5, o=oo, d=d[:n], width=width)
                    rgb = ctx.shade_rays_hdr(oo if stride == 3 else o[0], d[:n], mode, width=width, first_sample=5)[0]
                    check_floats(rgb, want, bound, dec, f"shape {n} x {width} stride {stride} mode {mode}", min_decided=0)
                    checked += int(f.all_decided().sum())
    finally:
        _restore(ctx)
    assert checked > 0.85 * 2 * 2 * sum(n for n, _ in SHAPES), checked


# ---- the HDR accumulation (corner source) ------------------------------------------------------------------------------------------
def _resolve_checks(ctx, b, mode, first, n, what):
    """accum_resolve_hdr's floats and tone-mapped bytes against the reference's mean; the device resolve gives the same bits"""
    W = b.width
    H = len(b.d) // W
    mean, bound, dec = b.mean(mode, first, n)
    rgb, rgba, _ = ctx.accum_resolve_hdr("reinhard", 0.25)
    check_floats(rgb.reshape(-1, 3), mean, bound, dec, what)
    check_tonemapped(rgba.reshape(-1, 4), mean, bound, dec, "reinhard", 0.25, what)
    check_tonemapped(ctx.accum_resolve_hdr()[1].reshape(-1, 4), mean, bound, dec, "clamp", 1.0, what)
    d_rgb, d_rgba = ctx.device_alloc(W * H * 12), ctx.device_alloc(W * H * 4)
    try:
        ctx.accum_resolve_hdr_device(d_rgb, d_rgba, None, "reinhard", 0.25)
        assert np.array_equal(ctx.device_read(d_rgb, (H, W, 3), F).view(np.uint32), rgb.view(np.uint32)), what + ": device resolve rgb"
        assert np.array_equal(ctx.device_read(d_rgba, (H, W, 4), np.uint8), rgba), what + ": device resolve rgba8"
    finally:
        ctx.device_free(d_rgb)
        ctx.device_free(d_rgba)


@pytest.mark.parametrize("name,mode", [("dragon_frame", 2), ("room_frame", 2), ("dragon_frame", 1)])
def test_hdr_accumulation_matches_the_references(ctx, V, O, RR, scenes, name, mode):
    """accum_add(1) at each of SAMPLES, one accum_add(4) from sample 7, 3 + 5, then the adaptive form: each pixel's mean
    covers the reference's first n_p samples, n_p read from accum_counts()"""
    _, _, W, H, _, _ = FRAMES[name]
    b = batch(name, V, O, RR, scenes)
    try:
        ctx.upload_octree(b.tex, b.dim)
        _params(ctx, b)
        for k in SAMPLES:
            ctx.accum_begin(W, H, first_sample=k, mode=mode, hdr=True)
            assert ctx.accum_add(1) == 1
            _resolve_checks(ctx, b, mode, k, 1, f"{name} mode {mode} sample {k}")
        ctx.accum_begin(W, H, first_sample=MEAN_FIRST, mode=mode, hdr=True)
        assert ctx.accum_add(4) == 4
        _resolve_checks(ctx, b, mode, MEAN_FIRST, 4, f"{name} mode {mode} 4 samples")
        ctx.accum_begin(W, H, first_sample=MEAN_FIRST, mode=mode, hdr=True)
        assert ctx.accum_add(3) == 3 and ctx.accum_add(5) == 8
        _resolve_checks(ctx, b, mode, MEAN_FIRST, 8, f"{name} mode {mode} 3 + 5 samples")
        if mode == 2:
            rule = (2, 6, 3)
            ctx.accum_begin(W, H, first_sample=MEAN_FIRST, mode=2, adaptive=rule, hdr=True)
            ctx.accum_add(6)
            counts, _ = ctx.accum_counts()
            check_adaptive(b, counts.ravel().astype(np.int64), ctx.accum_resolve_hdr()[0].reshape(-1, 3), rule, f"{name} adaptive")
    finally:
        _restore(ctx)
