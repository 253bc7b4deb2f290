"""vrt_accum_guides, vrt_guide_rays and the filtered resolve's guide state on the gfx950 kernels against the independent float64
restatement (tests/guide_ref64.py) directly, not through the C checkers: on the frames, batches, caps and bounds of
tests/test_guides_reference64.py, which asserts the left-out shares and the floors on the same references.

The references are traced once per input and sample (that module keeps them) and reused across every route: both traversal
variants, the four ray sources at both frame sizes, one sample and three split 1 + 2, the setting on and off, an adaptive
accumulation, ray batches as a list and as an image in the host and the device form, a highlighted voxel, and the planes left
behind by a filtered resolve. Decided pixels are exact bits in normal, albedo and coverage (or the hit byte); the depth lies within
the reference's derived bound."""
import numpy as np
import pytest

import guide_ref64 as GR
import guide_worlds as GW
from test_guides_reference64 import (ALL_BATCHES, BATCH_CAPS, FRAME_CAPS, MEAN_FIRST, MEAN_N, SAMPLES, SIZES, batch_trace, check_planes,
                                     frame_camera, frame_input, frame_trace, lens_of, most_frequent_cell_behind_glass, ray_batch)
from test_shader_reference64 import scenes  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
VARIANTS = (0, 1)          # the default wide traversal and the record-array route
MODE_FULL, MODE_PRIMARY = 2, 0


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(ctx):
    yield
    ctx.set_variant(0)
    ctx.set_lens(0.0, 1.0)
    ctx.set_guide_glass(False)
    ctx.set_params(ctx.default_params())


def _open(ctx, V, name, size, source, first, glass=True, mode=MODE_PRIMARY, **kw):
    tex, dim = frame_input(V, name)[:2]
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    ctx.set_camera(*frame_camera(V, name, size))
    ctx.set_lens(*lens_of(V, name, source))
    ctx.set_guide_glass(glass)
    ctx.accum_begin(size[0], size[1], first, mode=mode, jitter=GW.SOURCES[source][0], **kw)


def _want(V, name, size, source, first, n, glass=True):
    want = GR.resolve([frame_trace(V, name, size, source, k, glass=glass) for k in range(first, first + n)])
    assert want["decided"].mean() >= 1.0 - FRAME_CAPS[name][2 if n > 1 else 0], (name, size, source, first, n)
    return want


# ---- vrt_accum_guides ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=["40x24", "43x21"])
@pytest.mark.parametrize("name", sorted(FRAME_CAPS))
def test_accum_guides_match_the_reference(ctx, V, name, size):
    """variants 0 and 1, four sources: n = 1 at samples 5 and 12, n = 3 split 1 + 2, and the setting off"""
    worst = 0.0
    for variant in VARIANTS:
        ctx.set_variant(variant)
        for source in GW.SOURCES:
            what = f"{name} {size[0]} x {size[1]} {source} variant {variant}"
            for k in SAMPLES:
                _open(ctx, V, name, size, source, k)
                assert ctx.accum_add(1) == 1
                worst = max(worst, check_planes(_want(V, name, size, source, k, 1), ctx.accum_guides(), f"{what} sample {k}"))
            _open(ctx, V, name, size, source, MEAN_FIRST)
            assert ctx.accum_add(1) == 1
            check_planes(_want(V, name, size, source, MEAN_FIRST, 1), ctx.accum_guides(), f"{what} 1 of 1 + 2")
            assert ctx.accum_add(MEAN_N - 1) == MEAN_N
            check_planes(_want(V, name, size, source, MEAN_FIRST, MEAN_N), ctx.accum_guides(), f"{what} 1 + 2")
            _open(ctx, V, name, size, source, SAMPLES[0], glass=False)
            assert ctx.accum_add(1) == 1
            check_planes(_want(V, name, size, source, SAMPLES[0], 1, glass=False), ctx.accum_guides(), f"{what} off")
    print(f"{name} {size}: worst depth err / bound on the device {worst:.3f}")
    assert worst <= GR.MEASURED_RATIOS[name] + 5e-4


def test_an_adaptive_accumulation_takes_every_round(ctx, V):
    name, size, source = "lamp", SIZES[0], "jitter_lens"
    _open(ctx, V, name, size, source, MEAN_FIRST, mode=MODE_FULL, adaptive=(2, 64, 65535))
    assert ctx.accum_add(1) == 1
    ctx.accum_guides()
    assert ctx.accum_add(MEAN_N - 1) == MEAN_N
    counts, _ = ctx.accum_counts()
    assert (counts < MEAN_N).any()
    check_planes(_want(V, name, size, source, MEAN_FIRST, MEAN_N), ctx.accum_guides(), "adaptive")


def test_a_filtered_resolve_leaves_the_references_planes(ctx, V):
    """vrt_accum_resolve_hdr_filtered brings the guide state up to date itself; vrt_accum_guides then adds nothing and returns the
    planes the reference gives for the same three samples"""
    name, size, source = "room_wall", SIZES[1], "jitter"
    _open(ctx, V, name, size, source, MEAN_FIRST, mode=MODE_FULL, hdr=True)
    assert ctx.accum_add(MEAN_N) == MEAN_N
    rgb, _ = ctx.accum_resolve_hdr_filtered()
    assert np.isfinite(rgb).all()
    check_planes(_want(V, name, size, source, MEAN_FIRST, MEAN_N), ctx.accum_guides(), "after a filtered resolve")


# ---- vrt_guide_rays --------------------------------------------------------------------------------------------------------------------
def _params(ctx, b, highlighted=(-1, -1, -1)):
    p = ctx.default_params()
    p.voxel_scale = b.scale
    p.world_min[:], p.world_max[:] = list(b.wmin), list(b.wmax)
    p.global_light[:] = [float(v) for v in b.gl]
    p.light_dir[:] = [float(v) for v in b.light]
    p.highlighted[:] = [int(v) for v in highlighted]
    ctx.set_params(p)


def _device_form(ctx, b, width):
    n = len(b.d)
    bufs = [ctx.device_alloc(m) for m in (b.o.nbytes, b.d.nbytes, n * 12, n * 16, n * 4, n)]
    try:
        ctx.device_write(bufs[0], b.o)
        ctx.device_write(bufs[1], b.d)
        ctx.guide_rays_device(n, bufs[0], 3, bufs[1], *bufs[2:], width=width)
        return {"normal": ctx.device_read(bufs[2], (n, 3), F), "albedo": ctx.device_read(bufs[3], (n, 4), F),
                "depth": ctx.device_read(bufs[4], (n,), F), "hit": ctx.device_read(bufs[5], (n,), np.uint8)}
    finally:
        for p in bufs:
            ctx.device_free(p)


@pytest.mark.parametrize("name", ALL_BATCHES)
def test_guide_rays_match_the_reference(ctx, V, O, scenes, name):
    """as a list (width 7) and as an image (width 64: the 8 x 8 tile route), host and device forms, both variants; the setting off;
    the highlighted voxel"""
    b = ray_batch(name, V, O, scenes)
    assert b.o.shape == b.d.shape
    ctx.upload_octree(b.tex, b.dim)
    on, off = batch_trace(b).planes(), batch_trace(b, glass=False).planes()
    assert on["decided"][~batch_trace(b).outside].mean() >= 1.0 - BATCH_CAPS[name][0]
    worst = 0.0
    for variant in VARIANTS:
        ctx.set_variant(variant)
        _params(ctx, b)
        ctx.set_guide_glass(True)
        for width in (7, 64):
            what = f"{name} variant {variant} width {width}"
            worst = max(worst, check_planes(on, ctx.guide_rays(b.o, b.d, width=width), what, coverage=False))
            check_planes(on, _device_form(ctx, b, width), what + " device form", coverage=False)
        ctx.set_guide_glass(False)
        check_planes(off, ctx.guide_rays(b.o, b.d, width=64), f"{name} variant {variant} off", coverage=False)
    hl = most_frequent_cell_behind_glass(batch_trace(b))
    if hl is not None:
        ctx.set_variant(0)
        _params(ctx, b, hl)
        ctx.set_guide_glass(True)
        marked = batch_trace(b, highlighted=hl).planes()
        assert not np.array_equal(marked["albedo"], on["albedo"])
        for width in (7, 64):
            check_planes(marked, ctx.guide_rays(b.o, b.d, width=width), f"{name} highlighted {hl} width {width}", coverage=False)
    print(f"{name}: worst depth err / bound on the device {worst:.3f}")
    assert worst <= GR.MEASURED_RATIOS[name] + 5e-4
