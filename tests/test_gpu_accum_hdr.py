"""HDR accumulation on the MI355X (vrt_accum_keep_hdr, vrt_accum_resolve_hdr) against the checker (tests/oracle_hdr.c: the oracle's
float colour of every sample, the sequential float64 sums, the mean, the tone maps). Everything is bit for bit: floats are
compared as their uint32 views. Every kernel route -- the opaque dragon (pass 1 + the sample-looped bounce from the corner, the
opaque chain with jitter or a lens), the room (the general full path tracer), the primary modes (the repeat of a frame, the
sample-looped primary kernels), a record-only upload (the record-array kernels) -- crossed with corner / jitter / lens /
jitter + lens and plain / adaptive; the device resolve, chunked adds, the restart rule, the byte side of an HDR accumulation
against the same accumulation without HDR, the error codes and the setter's timing."""
import os

import numpy as np
import pytest

import oracle_hdr
from conftest import MAPS
from test_gpu_accum_jitter import SCENES, _same, _setup

pytestmark = pytest.mark.gpu

SOURCES = {"corner": (False, None), "jitter": (True, None), "lens": (False, True), "jitter_lens": (True, True)}
LENS = {"dragon": (2.0, 60.0), "room_outside": (1.25, 45.0), "nature": (2.5, 90.0)}   # tests/test_gpu_accum_lens.py's
RULE = (2, 6, 24)     # adaptive: some pixels stop at 2, some run to 6
TONEMAPS = (("clamp", 1.0), ("clamp", 0.37), ("reinhard", 1.0), ("reinhard", 2.5))
FIRST, N = 5, 6


@pytest.fixture(scope="module")
def HL(tmp_path_factory):
    return oracle_hdr.build(tmp_path_factory.mktemp("oracle_hdr"))


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, ref, what):
    _same(_bits(got), _bits(ref), what)


def _lens_of(name, source):
    return LENS[name] if SOURCES[source][1] else (0.0, 1.0)


def _reference(HL, scene, W, H, mode, first, n, name, source, rule):
    jitter = SOURCES[source][0]
    ap, focus = _lens_of(name, source)
    acc = oracle_hdr.Accum(HL, H, W, rule)
    for k in range(n):
        acc.add(oracle_hdr.render(HL, scene, W, H, mode, (first + k) & 0xFFFFFFFF, jitter=jitter, aperture=ap, focus=focus))
    _, frame_id = oracle_hdr.render_bytes(HL, scene, W, H, mode, 0)   # the unjittered pinhole frame's
    return acc, frame_id


def _accumulate(ctx, W, H, mode, first, chunks, name, source, rule, hdr=True):
    ctx.set_lens(*_lens_of(name, source))
    ctx.accum_begin(W, H, first, mode=mode, jitter=SOURCES[source][0], adaptive=rule, hdr=hdr)
    total = 0
    for n in chunks:
        total += n
        assert ctx.accum_add(n) == total


def _check(ctx, HL, O, scene, W, H, mode, name, source, rule, what):
    try:
        acc, frame_id = _reference(HL, scene, W, H, mode, FIRST, N, name, source, rule)
        _accumulate(ctx, W, H, mode, FIRST, [N], name, source, rule)
        mean = acc.mean()
        for op, e in TONEMAPS:
            rgb, rgba, shown = ctx.accum_resolve_hdr(op, e)
            tag = f"{what} mode {mode} {source} {'adaptive' if rule else 'plain'} {op} x{e}"
            _same_bits(rgb, mean, f"{tag}: float mean")
            want = oracle_hdr.tonemap(HL, mean, op, e)
            _same(rgba, want, f"{tag}: tone-mapped bytes")
            _same(shown, O.denoise(want, frame_id), f"{tag}: shown")
        # the byte side of the same accumulation is the checker's, and the same accumulation's without HDR
        rgba, idd, shown = ctx.accum_resolve()
        _same(rgba, acc.resolve_bytes(), f"{what} mode {mode} {source}: byte resolve vs the checker")
        counts = ctx.accum_counts()[0] if rule else None
        if rule:
            _same(counts[..., None], acc.counts()[..., None], f"{what} mode {mode} {source}: counts vs the checker")
        _accumulate(ctx, W, H, mode, FIRST, [N], name, source, rule, hdr=False)
        for a, b, w in zip(ctx.accum_resolve(), (rgba, idd, shown), ("rgba8", "id_dist", "shown")):
            _same(a, b, f"{what} mode {mode} {source}: {w} with and without HDR")
        if rule:
            _same(ctx.accum_counts()[0][..., None], counts[..., None], f"{what} mode {mode} {source}: counts with and without HDR")
    finally:
        ctx.set_lens(0.0, 1.0)


@pytest.mark.parametrize("rule", [None, RULE], ids=["plain", "adaptive"])
@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("name,mode", [("dragon", 2), ("room_outside", 2), ("dragon", 0), ("dragon", 1), ("nature", 2)])
def test_hdr_resolve_is_the_checkers(ctx, V, O, HL, product_scenes, name, mode, source, rule):
    m, W, H, pose = SCENES[name]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    _check(ctx, HL, O, scene, W, H, mode, name, source, rule, name)


@pytest.mark.parametrize("rule", [None, RULE], ids=["plain", "adaptive"])
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_record_only_upload(ctx, V, O, HL, product_scenes, source, rule):
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    rec = w.records()
    w.close()
    m, W, H, pose = SCENES["dragon"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose, records=rec)
    for mode in (1, 2):
        _check(ctx, HL, O, scene, W, H, mode, "dragon", source, rule, "records")


def test_every_variant(ctx, V, O, HL, product_scenes):
    m, W, H, pose = SCENES["room_outside"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    try:
        for var in V.available_variants():
            ctx.set_variant(var)
            for mode, source in ((2, "corner"), (2, "jitter_lens"), (1, "jitter"), (0, "corner")):
                _check(ctx, HL, O, scene, W, H, mode, "room_outside", source, None, f"variant {var}")
    finally:
        ctx.set_variant(0)


@pytest.mark.parametrize("rule", [None, RULE], ids=["plain", "adaptive"])
@pytest.mark.parametrize("name,mode,source", [("dragon", 2, "corner"), ("dragon", 2, "jitter"), ("room_outside", 2, "lens"),
                                              ("dragon", 1, "corner"), ("dragon", 0, "jitter_lens")])
def test_three_plus_five_adds_equal_eight(ctx, V, O, product_scenes, name, mode, source, rule):
    m, W, H, pose = SCENES[name]
    _setup(ctx, V, O, product_scenes, m, W, H, pose)
    try:
        _accumulate(ctx, W, H, mode, 11, [8], name, source, rule)
        ref = ctx.accum_resolve_hdr("reinhard", 1.5)
        for chunks in ([3, 5], [1] * 8):
            _accumulate(ctx, W, H, mode, 11, chunks, name, source, rule)
            got = ctx.accum_resolve_hdr("reinhard", 1.5)
            _same_bits(got[0], ref[0], f"{name} mode {mode} {source} {chunks}: float mean")
            _same(got[1], ref[1], f"{name} mode {mode} {source} {chunks}: bytes")
            _same(got[2], ref[2], f"{name} mode {mode} {source} {chunks}: shown")
    finally:
        ctx.set_lens(0.0, 1.0)


def test_device_resolve_is_the_host_resolve(ctx, V, O, product_scenes):
    import torch
    m, W, H, pose = SCENES["room_outside"]
    _setup(ctx, V, O, product_scenes, m, W, H, pose)
    _accumulate(ctx, W, H, 2, 0, [4], "room_outside", "jitter", None)
    d_rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    d_rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    d_shown = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    for stream in (None, side.cuda_stream):
        for op, e in TONEMAPS[1:3]:
            ctx.accum_resolve_hdr_device(d_rgb.data_ptr(), d_rgba.data_ptr(), d_shown.data_ptr(), op, e, stream=stream)
            torch.cuda.synchronize()
            rgb, rgba, shown = ctx.accum_resolve_hdr(op, e)      # (synchronises the context's stream)
            torch.cuda.synchronize()
            _same_bits(d_rgb.cpu().numpy(), rgb, f"{op} x{e}: device float mean")
            _same(d_rgba.cpu().numpy(), rgba, f"{op} x{e}: device bytes")
            _same(d_shown.cpu().numpy(), shown, f"{op} x{e}: device shown")
    d_only = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")      # the float image alone
    ctx.accum_resolve_hdr_device(d_only.data_ptr(), None, None)
    rgb, _, _ = ctx.accum_resolve_hdr()
    torch.cuda.synchronize()
    _same_bits(d_only.cpu().numpy(), rgb, "device float mean alone")


def test_a_camera_change_restarts_the_float_sums(ctx, V, O, HL, product_scenes):
    m, W, H, pose = SCENES["room_outside"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    ctx.accum_begin(W, H, 3, mode=2, jitter=True, hdr=True)
    assert ctx.accum_add(4) == 4
    moved = (pose[0] + 1.0, pose[1], pose[2], pose[3], pose[4])
    ip, iv, cp, _ = V.camera_block(moved[:3], moved[3], moved[4], W, H)
    ctx.set_camera(ip, iv, cp)
    assert ctx.accum_add(2) == 2
    tex, dim = product_scenes[m]
    acc, _ = _reference(HL, O.make_scene(tex, dim, ip, iv, cp), W, H, 2, 3, 2, "room_outside", "jitter", None)
    _same_bits(ctx.accum_resolve_hdr()[0], acc.mean(), "samples 3, 4 from the new camera alone")


def test_keep_hdr_is_read_at_the_begin_only(ctx, V, O, product_scenes):
    m, W, H, pose = SCENES["dragon"]
    _setup(ctx, V, O, product_scenes, m, W, H, pose)
    L, h = ctx._L, ctx._h
    ctx.accum_begin(W, H, 0, mode=2, hdr=True)
    assert ctx.accum_add(2) == 2
    ref = ctx.accum_resolve_hdr()
    assert L.vrt_accum_keep_hdr(h, 0) == 0                 # a running HDR accumulation stays one, and is not restarted
    assert ctx.accum_add(1) == 3
    rgb3 = ctx.accum_resolve_hdr()[0]
    ctx.accum_begin(W, H, 0, mode=2, hdr=True)
    assert ctx.accum_add(3) == 3
    _same_bits(ctx.accum_resolve_hdr()[0], rgb3, "2 + 1 samples across the setter")
    assert not np.array_equal(_bits(ref[0]), _bits(rgb3))
    ctx.accum_begin(W, H, 0, mode=2, hdr=False)
    assert ctx.accum_add(1) == 1
    assert L.vrt_accum_keep_hdr(h, 1) == 0                 # ... and one begun without stays without
    assert ctx.accum_add(1) == 2
    assert L.vrt_accum_resolve_hdr(h, None, None, None, None) == -5
    assert L.vrt_accum_keep_hdr(h, 0) == 0


def test_error_codes(V, product_scenes):
    c = V.Context(0)
    try:
        L, h = c._L, c._h
        T = V.Tonemap
        ref = V.C.byref
        assert L.vrt_accum_keep_hdr(None, 1) == -1
        for bad in (2, -1, 255):
            assert L.vrt_accum_keep_hdr(h, bad) == -1
        assert L.vrt_accum_resolve_hdr(h, None, None, None, None) == -5              # no begin
        assert L.vrt_accum_resolve_hdr_device(h, None, None, None, None, None) == -5
        m, W, H, pose = SCENES["dragon"]
        tex, dim = product_scenes[m]
        c.upload_octree(tex, dim)
        ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
        c.set_camera(ip, iv, cp)
        c.accum_begin(W, H, 0, hdr=True)
        assert L.vrt_accum_resolve_hdr(h, None, None, None, None) == -5              # no sample yet
        assert c.accum_add(1) == 1
        assert L.vrt_accum_resolve_hdr(h, None, None, None, None) == 0
        for op, e in ((2, 1.0), (-1, 1.0), (0, 0.0), (0, -1.0), (1, float("nan")), (1, float("inf")), (0, -float("inf"))):
            assert L.vrt_accum_resolve_hdr(h, None, ref(T(op, e)), None, None) == -1, (op, e)
            assert L.vrt_accum_resolve_hdr_device(h, None, ref(T(op, e)), None, None, None) == -1, (op, e)
        assert L.vrt_accum_resolve_hdr(h, None, ref(T(1, 1e-30)), None, None) == 0
        assert L.vrt_accum_resolve_hdr_device(h, None, None, None, 1, None) == -1    # the display pass needs d_rgba8
        c.accum_begin(W, H, 0, hdr=False)
        assert c.accum_add(1) == 1
        assert L.vrt_accum_resolve_hdr(h, None, None, None, None) == -5              # begun without HDR
        assert L.vrt_accum_resolve_hdr_device(h, None, None, None, None, None) == -5
        for flags in (2, 0x80000001):                                                # HDR is no flag of the begin
            assert L.vrt_accum_begin_ex(h, W, H, 2, 0, flags) == -1
    finally:
        c.close()
