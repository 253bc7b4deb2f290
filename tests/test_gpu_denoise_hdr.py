"""The HDR display pass on the MI355X (vrt_denoise_hdr, vrt_accum_resolve_hdr_shown; include/vrt.h) against the checker
(tests/oracle_denoise_hdr.c, which tests/test_denoise_hdr.py holds to the byte pass and to float64). Bit for bit: floats are
compared as their uint32 views. Every case runs under the three VRT_OPT_DISPLAY_KERNEL values and three tone maps."""
import ctypes as C

import numpy as np
import pytest

import oracle_denoise_hdr as D
import oracle_hdr
from test_gpu_accum_jitter import _same, _setup

pytestmark = pytest.mark.gpu

KERNELS = (0, 2, 3)
TONEMAPS = (("clamp", 1.0), ("clamp", 0.37), ("reinhard", 2.5))
DRAGON = (63.5, 60.5, 140.5, -90.0, -10.0)
DRAGON_CLOSE = (60.3, 64.7, 75.2, -100.0, -25.0)
RULE = (2, 6, 24)


@pytest.fixture(scope="module")
def DL(tmp_path_factory):
    return D.build(tmp_path_factory.mktemp("oracle_denoise_hdr"))


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, ref, what):
    _same(_bits(got), _bits(ref), what)


def _check(ctx, DL, rgb, idd, what):
    """host form, every kernel and tone map, floats and bytes against the checker -> the checker's floats"""
    ref, _ = D.denoise(DL, rgb, idd)
    try:
        for dv in KERNELS:
            ctx.set_denoise_variant(dv)
            for op, e in TONEMAPS:
                got, got8 = ctx.denoise_hdr(rgb, idd, op, e)
                _same_bits(got, ref, f"{what} kernel {dv} {op} x{e}: floats")
                _same(got8, oracle_hdr.tonemap(DL, ref, op, e), f"{what} kernel {dv} {op} x{e}: bytes")
    finally:
        ctx.set_denoise_variant(0)
    return ref


def _colours(rng, W, H, specials=True):
    rgb = np.exp2(rng.uniform(-20, 16, size=(H, W, 3))).astype(np.float32)      # up to 65536: some exceed 65504
    if specials:
        for v in (np.nan, np.inf, -np.inf, -3.5, -0.0, 1e-41, 3e-39):
            rgb[rng.random((H, W, 3)) < 0.01] = np.float32(v)
    return rgb


def _device(ctx, rgb, idd, op, e, offset=0, stream=None):
    """the device form -> (floats, bytes); offset: bytes the float image's base is moved off its allocation"""
    import torch
    H, W = idd.shape[:2]
    n = H * W * 3
    buf = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    buf[offset // 4: offset // 4 + n] = torch.from_numpy(np.ascontiguousarray(rgb, np.float32).reshape(-1))
    d_id = torch.from_numpy(np.ascontiguousarray(idd, np.int32)).cuda()
    out = torch.zeros(n, dtype=torch.float32, device="cuda")
    out8 = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.denoise_hdr_device(W, H, buf.data_ptr() + offset, d_id.data_ptr(), out.data_ptr(), out8.data_ptr(), op, e, stream)
    ctx.synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(H, W, 3), out8.cpu().numpy().view(np.uint8).reshape(H, W, 4)


def test_synthetic_ids_and_every_distance_class(ctx, DL):
    rng = np.random.default_rng(9)
    W, H = 150, 90
    idd = np.zeros((H, W, 2), np.int32)
    idd[..., 0] = rng.integers(-3, 4, size=(H, W))
    idd[..., 1] = rng.choice([0, 1, 2, 50, 99, 100, 101, 400, 2047, 40000], size=(H, W))
    rgb = _colours(rng, W, H)
    assert np.any(rgb > 65504) and np.any(np.isnan(rgb)) and np.any(rgb < 0)
    ref = _check(ctx, DL, rgb, idd, "synthetic")
    assert np.all(np.isfinite(ref)) and np.all(ref >= 0)


@pytest.mark.parametrize("size", [(131, 83), (132, 84)], ids=["tap_by_tap", "16_byte_loads"])
def test_id_table_cases(ctx, DL, size):
    """every pixel its own id (the table overflows), ~100 ids per tile, forty ids in one hash slot, one id far apart within a
    window, ids only in a tile's halo"""
    W, H = size
    rng = np.random.default_rng(10)
    yy, xx = np.mgrid[0:H, 0:W]
    slot = lambda v: ((int(v) * 2654435761) & 0xffffffff) >> 25
    same_slot = [v for v in range(1, 400000) if slot(v) == 5][:40]
    fields = [1 + yy * W + xx, 1 + (yy // 2) * 16 + (xx // 3) % 16 + 1000 * (xx // 48), np.array(same_slot)[(yy // 4 * 7 + xx // 5) % 40],
              np.where((xx % 37 < 2) | (yy % 29 < 2), 9, 1 + (xx // 9 + 11 * (yy // 7)) % 60), np.where(xx % 32 < 20, 0, 3 + yy // 6)]
    for k, ids in enumerate(fields):
        idd = np.zeros((H, W, 2), np.int32)
        idd[..., 0] = ids
        idd[..., 1] = rng.choice([60, 100, 120, 400], size=(H, W)) if k % 2 else 100
        _check(ctx, DL, _colours(rng, W, H), idd, f"id table case {k} {W}x{H}")


@pytest.mark.parametrize("size", [(67, 35), (130, 50), (128, 48), (5, 3)])
def test_radii_spread_inside_a_wave(ctx, DL, size):
    W, H = size
    rng = np.random.default_rng(11)
    idd = np.zeros((H, W, 2), np.int32)
    idd[..., 0] = 7
    idd[H // 3, W // 2, 0] = 0
    yy, xx = np.mgrid[0:H, 0:W]
    for dist in (100 + (xx + yy) // 3, 100 + 60 * ((xx // 5 + yy // 3) % 4), 90 + (xx * 37 + yy * 11) % 400):
        idd[..., 1] = dist
        _check(ctx, DL, _colours(rng, W, H), idd, f"radii {W}x{H}")


def test_unaligned_base_pointer_stages_tap_by_tap(ctx, DL):
    """a width that is a multiple of four with the float image 4 bytes off a 16-byte boundary: no 16-byte loads, same result"""
    rng = np.random.default_rng(12)
    W, H = 132, 84
    yy, xx = np.mgrid[0:H, 0:W]
    idd = np.zeros((H, W, 2), np.int32)
    idd[..., 0] = np.where(xx % 32 < 3, 0, 1 + (xx // 9 + 11 * (yy // 7)) % 60)
    idd[..., 1] = rng.choice([60, 100, 120, 400], size=(H, W))
    rgb = _colours(rng, W, H)
    ref, _ = D.denoise(DL, rgb, idd)
    try:
        for dv in KERNELS:
            ctx.set_denoise_variant(dv)
            for op, e in TONEMAPS:
                want8 = oracle_hdr.tonemap(DL, ref, op, e)
                for offset in (0, 4):
                    got, got8 = _device(ctx, rgb, idd, op, e, offset)
                    _same_bits(got, ref, f"device form, base + {offset}, kernel {dv}: floats")
                    _same(got8, want8, f"device form, base + {offset}, kernel {dv} {op} x{e}: bytes")
    finally:
        ctx.set_denoise_variant(0)


def test_all_65504_at_radius_20(ctx, DL):
    W, H = 70, 45
    rgb = np.full((H, W, 3), 1e30, np.float32)        # h() brings every float to 65504
    idd = np.zeros((H, W, 2), np.int32)
    idd[..., 0] = 3
    idd[..., 1] = 100
    ref = _check(ctx, DL, rgb, idd, "all 65504")
    assert np.all(np.isfinite(ref)) and ref.max() <= 65504.0 * (1 + 1681 * 2.0 ** -24)
    assert np.array_equal(ref[H // 2, W // 2], np.full(3, 65504.0, np.float32))     # every partial sum k * 65504 = k * 2047 * 32 is a float


def test_sky_only_image_passes_h_through(ctx, DL):
    rng = np.random.default_rng(13)
    W, H = 96, 40
    rgb = _colours(rng, W, H)
    idd = np.zeros((H, W, 2), np.int32)
    idd[..., 1] = rng.choice([0, 100, 40000], size=(H, W))
    ref = _check(ctx, DL, rgb, idd, "sky only")
    _same_bits(ref, D.h_of(DL, rgb), "sky only: the checker is h(c)")


def test_identity_with_the_byte_pass(ctx, V, O, product_scenes):
    """contract point 4: byte / 255.0f in, the NULL tone map -> vrt_denoise's bytes"""
    W, H = 256, 144
    _setup(ctx, V, O, product_scenes, "dragon", W, H, DRAGON)
    rgba, idd = ctx.dispatch(W, H, 2)
    rgb = rgba[..., :3].astype(np.float32) / np.float32(255.0)
    try:
        for dv in KERNELS:
            ctx.set_denoise_variant(dv)
            want = ctx.denoise(rgba, idd)
            _same(ctx.denoise_hdr(rgb, idd, None)[1], want, f"byte identity kernel {dv}")
    finally:
        ctx.set_denoise_variant(0)
    assert np.any(want != rgba)


def _accumulate(ctx, W, H, chunks, adaptive, hdr=True):
    ctx.accum_begin(W, H, 5, mode=2, jitter=adaptive, adaptive=RULE if adaptive else None, hdr=hdr)
    for n in chunks:
        ctx.accum_add(n)


@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "adaptive_jitter"])
def test_accumulation_shown(ctx, V, O, DL, product_scenes, adaptive):
    import torch
    W, H, N = 96, 54, 5
    scene, _ = _setup(ctx, V, O, product_scenes, "dragon", W, H, DRAGON)
    acc = oracle_hdr.Accum(DL, H, W, RULE if adaptive else None)
    for k in range(N):
        acc.add(oracle_hdr.render(DL, scene, W, H, 2, 5 + k, jitter=adaptive))
    _accumulate(ctx, W, H, [N], adaptive)
    before = ctx.accum_resolve_hdr("reinhard", 2.5)
    idd = ctx.accum_resolve()[1]
    _same_bits(before[0], acc.mean(), "the accumulation's mean is the checker's")
    want_rgb = D.denoise(DL, acc.mean(), idd)[0]
    try:
        for dv in KERNELS:
            ctx.set_denoise_variant(dv)
            for op, e in TONEMAPS:
                tag = f"kernel {dv} {op} x{e}"
                mean = ctx.accum_resolve_hdr(op, e)[0]
                rgb, rgba = ctx.accum_resolve_hdr_shown(op, e)
                two_rgb, two_rgba = ctx.denoise_hdr(mean, idd, op, e)
                _same_bits(rgb, two_rgb, f"{tag}: shown floats vs denoise_hdr(resolve)")
                _same(rgba, two_rgba, f"{tag}: shown bytes vs denoise_hdr(resolve)")
                _same_bits(rgb, want_rgb, f"{tag}: shown floats vs the checker")
                _same(rgba, oracle_hdr.tonemap(DL, want_rgb, op, e), f"{tag}: shown bytes vs the checker")
                for stream in (None, torch.cuda.Stream()):
                    d_rgb = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
                    d_rgba = torch.zeros(H * W, dtype=torch.int32, device="cuda")
                    torch.cuda.synchronize()
                    ctx.accum_resolve_hdr_shown_device(d_rgb.data_ptr(), d_rgba.data_ptr(), op, e, stream.cuda_stream if stream else None)
                    if stream:
                        stream.synchronize()
                    ctx.synchronize()
                    _same_bits(d_rgb.cpu().numpy().reshape(H, W, 3), rgb, f"{tag}: device form floats")
                    _same(d_rgba.cpu().numpy().view(np.uint8).reshape(H, W, 4), rgba, f"{tag}: device form bytes")
    finally:
        ctx.set_denoise_variant(0)
    after = ctx.accum_resolve_hdr("reinhard", 2.5)
    _same_bits(after[0], before[0], "accum_resolve_hdr's mean after the shown resolves")
    _same(after[1], before[1], "accum_resolve_hdr's bytes after the shown resolves")
    _same(after[2], before[2], "accum_resolve_hdr's shown after the shown resolves")
    # 3 + 2 adds equal 5
    ref = ctx.accum_resolve_hdr_shown("reinhard", 2.5)
    _accumulate(ctx, W, H, [3, 2], adaptive)
    got = ctx.accum_resolve_hdr_shown("reinhard", 2.5)
    _same_bits(got[0], ref[0], "3 + 2 adds: floats")
    _same(got[1], ref[1], "3 + 2 adds: bytes")


def test_accumulation_state_errors(ctx, V, O, product_scenes):
    W, H = 96, 54
    _setup(ctx, V, O, product_scenes, "dragon", W, H, DRAGON)
    ctx.accum_begin(W, H, 0, mode=2, hdr=True)
    with pytest.raises(V.VrtError, match="vrt error -5"):      # before a sample
        ctx.accum_resolve_hdr_shown()
    ctx.accum_begin(W, H, 0, mode=2, hdr=False)
    ctx.accum_add(1)
    with pytest.raises(V.VrtError, match="vrt error -5"):      # without HDR
        ctx.accum_resolve_hdr_shown()
    with pytest.raises(V.VrtError, match="vrt error -5"):
        ctx.accum_resolve_hdr_shown_device(1, 1)
    ctx.accum_begin(W, H, 0, mode=2, hdr=True)
    ctx.accum_add(1)
    L, h = ctx._L, ctx._h
    out = np.zeros((H, W, 4), np.uint8)
    assert L.vrt_accum_resolve_hdr_shown(h, None, None, None) == -1                      # both outputs NULL
    assert L.vrt_accum_resolve_hdr_shown_device(h, None, None, None, None) == -1
    assert L.vrt_accum_resolve_hdr_shown(h, C.byref(V.Tonemap(7, 1.0)), None, out.ctypes.data) == -1
    assert L.vrt_accum_resolve_hdr_shown(h, C.byref(V.Tonemap(0, 0.0)), None, out.ctypes.data) == -1
    assert L.vrt_accum_resolve_hdr_shown(h, None, None, out.ctypes.data) == 0            # bytes alone, the NULL tone map
    assert np.all(out[..., 3] == 255)


def _emitter_world(V):
    """a grey floor with lights standing on it: floor pixels whose bounce finds a light take samples far above 1"""
    w = V.World()
    for x in range(24):
        for z in range(24):
            w.insert(x, 0, z, 0xa0a0a0ff)
    rng = np.random.default_rng(5)
    for _ in range(40):
        x, z = (int(v) for v in rng.integers(2, 22, size=2))
        w.insert(x, 1, z, 0xffd2d2ff, 3.0, 1.0, 0.0)        # emissive
    return w


def test_the_order_matters(ctx, V):
    """blur(tonemap(x)) != tonemap(blur(x)): on a world with emitters the new shown image is not accum_resolve_hdr's"""
    W, H = 96, 54
    w = _emitter_world(V)
    tex, dim = w.flatten()
    w.close()
    ctx.upload_octree(tex, dim)
    ip, iv, cp, _ = V.camera_block((12.5, 14.5, 34.5), -90.0, -40.0, W, H)
    ctx.set_camera(ip, iv, cp)
    ctx.set_params(ctx.default_params())
    ctx.accum_begin(W, H, 0, mode=2, hdr=True)
    ctx.accum_add(5)
    for op, e in (("clamp", 1.0), ("reinhard", 1.0)):
        mean, _, old_shown = ctx.accum_resolve_hdr(op, e)
        idd = ctx.accum_resolve()[1]
        assert np.any(mean[idd[..., 0] != 0] > 1.0), "no sample above 1 on a surface: the world shows no emitter"
        new_rgb, new_shown = ctx.accum_resolve_hdr_shown(op, e)
        diff = np.abs(new_shown[..., :3].astype(int) - old_shown[..., :3].astype(int))
        print(f"{op}: {int(np.sum(np.any(diff > 0, axis=-1)))} pixels differ, by up to {int(diff.max())} levels")
        assert np.any(new_shown != old_shown)
        assert np.array_equal(new_shown[idd[..., 0] == 0], old_shown[idd[..., 0] == 0])     # sky passes through either way


def _sched_frames(ctx, V, O, product_scenes, W, H):
    """two poses' frames as float images (an HDR range made from the bytes) and as bytes"""
    frames = []
    for pose in (DRAGON, DRAGON_CLOSE):
        _setup(ctx, V, O, product_scenes, "dragon", W, H, pose)
        rgba, idd = ctx.dispatch(W, H, 2)
        x = rgba[..., :3].astype(np.float32) / np.float32(255.0)
        frames.append((rgba, (x * x * np.float32(12.0)).astype(np.float32), idd))
    return frames


def test_feedback_scheduling(V, O, DL, product_scenes):
    """1056 x 544 (1,122 tiles): the scheduled HDR pass equals the unscheduled one (and that the checker) while its order is
    re-derived every one or two launches and goes stale when the image changes; byte launches interleaved on the same shape keep
    their result, their launch counter and their order."""
    W, H = 1056, 544
    c = V.Context(0)
    try:
        c.set_tile_scheduling(0)
        frames = _sched_frames(c, V, O, product_scenes, W, H)
        op, e = "reinhard", 2.5
        plain = [c.denoise_hdr(rgb, idd, op, e) for _, rgb, idd in frames]
        plain8 = [c.denoise(rgba, idd) for rgba, _, idd in frames]
        ref = D.denoise(DL, frames[0][1], frames[0][2])[0]
        _same_bits(plain[0][0], ref, "unscheduled HDR pass vs the checker: floats")
        _same(plain[0][1], oracle_hdr.tonemap(DL, ref, op, e), "unscheduled HDR pass vs the checker: bytes")
        for period in (1, 2):
            c.set_tile_scheduling(period)
            for k in range(9):
                i = (k // 2) % 2                     # same shape, the image changes every other call
                got = c.denoise_hdr(frames[i][1], frames[i][2], op, e)
                _same_bits(got[0], plain[i][0], f"scheduled HDR pass period {period} call {k}: floats")
                _same(got[1], plain[i][1], f"scheduled HDR pass period {period} call {k}: bytes")
                _same(c.denoise(frames[i][0], frames[i][2]), plain8[i], f"byte pass between HDR launches, period {period} call {k}")
            assert c.sched_order().size > 0
    finally:
        c.close()
    # the byte pass's state is its own: with period 2 its second launch measures and derives an order, its third does not. HDR
    # launches in between must not move that counter (a shared one would make the third byte launch measure, or skip the second)
    c = V.Context(0)
    try:
        c.set_tile_scheduling(2)
        rgba, rgb, idd = frames[0]
        c.denoise(rgba, idd)
        assert c.sched_order().size == 0             # launch 0 of the byte pass: nothing measured yet
        c.denoise_hdr(rgb, idd)                      # launch 0 of the HDR pass
        assert c.sched_order().size == 0
        c.denoise(rgba, idd)                         # launch 1 of the byte pass: measures
        order = c.sched_order()
        assert order.size > 0 and sorted(order.tolist()) == list(range(order.size))
        for _ in range(3):
            c.denoise_hdr(frames[1][1], frames[1][2])     # launches 1-3 of the HDR pass, another image: measures twice
        _same(c.denoise(rgba, idd), plain8[0], "byte pass after HDR launches")   # launch 2 of the byte pass: does not measure
        assert np.array_equal(c.sched_order(), order), "HDR launches changed the byte pass's order"
    finally:
        c.close()


def test_refusals(ctx, V):
    import torch
    W, H = 64, 32
    d_rgb = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    d_id = torch.zeros(H * W * 2, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    d_out8 = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L, h = ctx._L, ctx._h
    rgb, idd, out, out8 = d_rgb.data_ptr(), d_id.data_ptr(), d_out.data_ptr(), d_out8.data_ptr()
    ok = C.byref(V.Tonemap(1, 2.0))
    assert L.vrt_denoise_hdr(h, W, H, None, idd, ok, out, out8, None) == -1           # null inputs
    assert L.vrt_denoise_hdr(h, W, H, rgb, None, ok, out, out8, None) == -1
    assert L.vrt_denoise_hdr(h, W, H, rgb, idd, ok, None, None, None) == -1           # both outputs null
    assert L.vrt_denoise_hdr(h, W, H, rgb, idd, ok, rgb, out8, None) == -1            # d_out_rgb == d_rgb
    for op, e in ((2, 1.0), (-1, 1.0), (0, 0.0), (0, -1.0), (1, float("inf")), (1, float("nan"))):
        assert L.vrt_denoise_hdr(h, W, H, rgb, idd, C.byref(V.Tonemap(op, e)), out, out8, None) == -1, (op, e)
    for w, hh in ((0, H), (W, 0), (-1, H), (1 << 16, 1 << 16)):                       # a bad frame size
        assert L.vrt_denoise_hdr(h, w, hh, rgb, idd, ok, out, out8, None) == -1, (w, hh)
    assert L.vrt_denoise_hdr(h, W, H, rgb, idd, ok, out, None, None) == 0             # either output alone, the NULL tone map
    assert L.vrt_denoise_hdr(h, W, H, rgb, idd, None, None, out8, None) == 0
    ctx.synchronize()
    a = np.zeros((H, W, 3), np.float32)
    b = np.zeros((H, W, 2), np.int32)
    o8 = np.zeros((H, W, 4), np.uint8)
    assert L.vrt_denoise_hdr_host(h, W, H, None, b.ctypes.data, None, a.ctypes.data, o8.ctypes.data) == -1
    assert L.vrt_denoise_hdr_host(h, W, H, a.ctypes.data, None, None, a.ctypes.data, o8.ctypes.data) == -1
    assert L.vrt_denoise_hdr_host(h, W, H, a.ctypes.data, b.ctypes.data, None, None, None) == -1
    assert L.vrt_denoise_hdr_host(h, W, H, a.ctypes.data, b.ctypes.data, C.byref(V.Tonemap(3, 1.0)), None, o8.ctypes.data) == -1
    assert L.vrt_denoise_hdr_host(h, W, H, a.ctypes.data, b.ctypes.data, None, None, o8.ctypes.data) == 0
    with pytest.raises(ValueError):
        ctx.denoise_hdr(a, b, "filmic")
    with pytest.raises(ValueError):
        ctx.denoise_hdr(a[..., :2], b)
