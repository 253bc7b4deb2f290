"""The jittered and thin-lens samples of the accumulation on the gfx950 kernels against the float64 restatement of those
samples (tests/lens_ref64.py feeding tests/shader_ref64.py and tests/path_ref64.py), on the cases, caps and minimums of
tests/test_lens_reference64.py.

Each reference is traced once on the host and reused across every route: each shipped variant, VRT_OPT_FULL_OPAQUE 0, 1
and 6 on the opaque cases, texel and record uploads on the dragon, one 4-sample add through the looped kernel, the HDR resolve,
a 1080p frame at the last sample index. Every decided pixel must agree exactly in rgb, and in ID and dist with the
unjittered pinhole frame. The last test involves no reference and leaves no pixel out: the accumulation's sample k against
vrt_shade_rays on the checker's float32 rays of that sample, byte for byte."""
import numpy as np
import pytest

import lens_ref64 as LR
import oracle_lens
import path_ref64 as PR
import shader_ref64 as R
from test_gpu_accum_jitter import _setup
from test_gpu_accum_lens import POSES as LENS_POSES
from test_gpu_reference64 import _params, ctx, worlds  # noqa: F401
from test_lens_reference64 import (KS, MIN_HITS, SOURCES, cap_of, check_sample, lens_case, lens_of, pinhole, radiance,
                                   reference)
from test_rays_reference64 import check_floats
from test_shader_reference64 import Case, scenes  # noqa: F401

pytestmark = pytest.mark.gpu

import vrt_import

VARIANTS = vrt_import.vrt().available_variants()
GPU_CASES = {"dragon": (0, 1, 2), "room_inside": (2,), "medium_per_lane": (0, 1, 2), "opaque_per_lane": (2,)}   # case -> modes
OPAQUE = ("dragon", "opaque_per_lane")
FORMS = (0, 1, 6)                  # VRT_OPT_FULL_OPAQUE on the opaque cases: the general kernel, two kernels, the default


@pytest.fixture(scope="module")
def LL(tmp_path_factory):
    return oracle_lens.build(tmp_path_factory.mktemp("oracle_lens_gpu_ref64"))


def _restore(ctx, V):
    ctx.set_lens(0.0, 1.0)
    ctx.set_variant(0)
    ctx.set_option(V.OPT_FULL_OPAQUE, 6)
    ctx.set_params(ctx.default_params())


def _sample(ctx, lc, source, k, mode, n=1, hdr=False):
    ctx.accum_begin(lc.c.W, lc.c.H, first_sample=k, mode=mode, jitter=SOURCES[source][0], hdr=hdr)
    assert ctx.accum_add(n) == n


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_single_samples_match_the_float64_samples(ctx, V, worlds, scenes, name, source, k):
    lc = lens_case(V, scenes, name)
    modes = GPU_CASES[name]
    fr, pin = reference(lc, source, k, modes), pinhole(lc, modes)
    uploads = [("texels", lambda: ctx.upload_octree(lc.c.tex, lc.c.dim))]
    if name == "dragon":
        uploads.append(("records", lambda: ctx.upload_records(*worlds["dragon"].records())))
    n = 0
    try:
        for up, do in uploads:
            do()
            _params(ctx, lc.c)
            ctx.set_lens(*lens_of(lc, source))
            for v in VARIANTS:
                ctx.set_variant(v)
                for form in (FORMS if name in OPAQUE else (6,)):
                    ctx.set_option(V.OPT_FULL_OPAQUE, form)
                    for mode in modes:
                        _sample(ctx, lc, source, k, mode)
                        rgba, idd, _ = ctx.accum_resolve()
                        check_sample(fr[mode], pin[mode], rgba, idd, MIN_HITS[name][source][mode // 2], cap_of(lc, source),
                                     f"{name} {source} sample {k} mode {mode} {up} variant {v} opaque form {form}")
                        n += 1
    finally:
        _restore(ctx, V)
    assert n == len(uploads) * len(VARIANTS) * (len(FORMS) if name in OPAQUE else 1) * len(modes)


@pytest.mark.parametrize("source", ["jitter", "jitter_lens"])
def test_four_samples_through_the_looped_kernel(ctx, V, scenes, source):
    """(sum of the four reference bytes + 2) // 4 where all four samples are decided"""
    lc = lens_case(V, scenes, "dragon")
    first = 7
    fr = [reference(lc, source, first + i, (2,))[2] for i in range(4)]
    pin = pinhole(lc, (2,))[2]
    ctx.upload_octree(lc.c.tex, lc.c.dim)
    try:
        _params(ctx, lc.c)
        ctx.set_lens(*lens_of(lc, source))
        _sample(ctx, lc, source, first, 2, n=4)
        rgba, idd, _ = ctx.accum_resolve()
    finally:
        _restore(ctx, V)
    dec = np.all([f.dec_rgb.all(1) & f.dec_id for f in fr], axis=0)
    want = (sum(f.rgba[:, :3] for f in fr) + 2) // 4
    got = rgba[pin.ys, pin.xs, :3].astype(np.int64)
    assert dec.sum() > 0.85 * dec.size, dec.mean()
    assert np.array_equal(got[dec], want[dec]), np.argwhere(np.any(got != want, 1) & dec)[:5]
    ok_id = pin.dec_id & pin.dec_dist
    assert np.array_equal(idd[pin.ys, pin.xs][ok_id], np.stack([pin.id, pin.dist], 1)[ok_id])


@pytest.mark.parametrize("name,source", [("dragon", "jitter"), ("room_inside", "jitter_lens")])
def test_hdr_means_lie_within_the_radiance_bound(ctx, V, scenes, name, source):
    """accum_resolve_hdr's float mean of 1 and of 4 samples against radiance() carried through hdr_mean"""
    lc = lens_case(V, scenes, name)
    first = 7
    rad = [radiance(lc, source, first + i, 2) for i in range(4)]
    ctx.upload_octree(lc.c.tex, lc.c.dim)
    try:
        _params(ctx, lc.c)
        ctx.set_lens(*lens_of(lc, source))
        for n in (1, 4):
            mean, bound, dec = R.hdr_mean([r[0] for r in rad[:n]], [r[1] for r in rad[:n]], [r[2] for r in rad[:n]])
            _sample(ctx, lc, source, first, 2, n=n, hdr=True)
            rgb = ctx.accum_resolve_hdr()[0]
            check_floats(rgb.reshape(-1, 3), mean, bound, dec, f"{name} {source} HDR mean of {n}", min_decided=int(0.7 * dec.size))
    finally:
        _restore(ctx, V)


def test_full_size_jittered_frame_at_the_last_sample(ctx, V, golden, product_scenes):
    """~20k seeded pixels of the 1920x1080 dragon, mode 2, jittered sample 2^32 - 1: px up to 1919 drops 11 bits of jx"""
    g = golden["frames"]["frames"]["dragon_1080p_full/mode2"]
    tex, dim = product_scenes[g["map"]]
    W, H = 1920, 1080
    c = Case(V, tex, dim, g["pose"], W, H)
    rng = np.random.default_rng(2027)
    xs, ys = rng.integers(0, W, 20000), rng.integers(0, H, 20000)
    world = R.World(tex, dim)
    k = 2 ** 32 - 1
    f = PR.PathTrace.lens(world, LR.lens_rays(*c.cam, W, H, xs, ys, sample=k, jitter=True), light_dir=c.light).frame()
    pin = PR.PathTrace(world, *c.cam, W, H, xs=xs, ys=ys, light_dir=c.light).frame()
    ctx.upload_octree(tex, dim)
    try:
        _params(ctx, c)
        ctx.accum_begin(W, H, first_sample=k, mode=2, jitter=True)
        assert ctx.accum_add(1) == 1
        rgba, idd, _ = ctx.accum_resolve()
        check_sample(f, pin, rgba, idd, FULL_SIZE_MIN_HITS, 0.015, "dragon 1080p jittered sample 2^32 - 1")
    finally:
        _restore(ctx, V)


FULL_SIZE_MIN_HITS = 9190   # 0.9 of the 10213 decided hits the reference gives against the checker (undecided share 0.0027)


@pytest.mark.parametrize("name", sorted(LENS_POSES))
def test_accumulation_samples_are_shade_rays_of_the_checkers_rays(ctx, V, O, LL, product_scenes, name):
    """include/vrt.h: a lens sample is pathTrace from o along dir with initRNG(pixel, k). The accumulation's sample k -- with
    whatever the dispatcher proved for this lens (eye_shared, first_shared, no_medium, empty) -- against vrt_shade_rays,
    which takes no such shortcut, on the checker's float32 rays: all pixels, all three modes, byte for byte"""
    m, W, H, pose, ap, focus, _ = LENS_POSES[name]
    scene, (_, _, cp) = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    n = 0
    try:
        ctx.set_lens(ap, focus)
        for k in (1, 255):
            for jitter in (False, True):
                o, d = np.zeros((H * W, 3), np.float32), np.zeros((H * W, 3), np.float32)
                for i in range(H * W):
                    _, o[i], d[i] = oracle_lens.ray(LL, scene, W, H, i % W, i // W, k, ap, focus, jitter=jitter)
                assert np.any(o != np.asarray(cp, np.float32)[:3])            # the lens moved the origins
                for mode in (0, 1, 2):
                    ctx.accum_begin(W, H, first_sample=k, mode=mode, jitter=jitter)
                    assert ctx.accum_add(1) == 1
                    rgba, _, _ = ctx.accum_resolve()
                    got, _ = ctx.shade_rays(o, d, mode, width=W, first_sample=k, n_samples=1)
                    diff = np.nonzero(np.any(got.reshape(H, W, 4) != rgba, axis=-1))
                    assert not diff[0].size, (f"{name} sample {k} jitter {jitter} mode {mode}: {diff[0].size} pixels differ, first at "
                                              f"(x={diff[1][0]}, y={diff[0][0]})")
                    n += 1
    finally:
        ctx.set_lens(0.0, 1.0)
    assert n == 12
