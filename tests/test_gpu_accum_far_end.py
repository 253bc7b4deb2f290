"""The accumulators at the sample cap on the MI355X: include/vrt.h allows 2^24 samples per accumulation and per ray batch, and the
routes on which every sample of a pixel is the same one reach it in constant time -- a primary mode from the corner (repeat_kernel,
repeat_adaptive_kernel, repeat_mom_kernel), the corner guide, the primary-mode ray batches, and the sky and emissive pixels of the
opaque bounce route. There the byte sums stand 2^23 below 2^32 (255 * 2^24 + 2^23), the float64 sums rely on (double)c * k being
exact, and M3 on m1f * m1f reproducing q. The counts are 2^24 and 2^24 - 1, reached as (2^24 - 1) + 1 and as 3 + (2^24 - 3). 2^24 - 1
has 24 significant bits: its product with a colour rounds in float32, where 2^24's is exact, so a float multiply shows in a caller's
sums, which are compared as float64 (the float32 mean rounds a sum that is off by one part in 2^24 back to the same float; and the
count itself is a float32, as every integer up to 2^24 is: converting it alone changes nothing). Every expectation is exact: Python integers, numpy float64, or the one-sample result, which the
other device modules hold to the checkers."""
import numpy as np
import pytest

import guide_worlds as GW
import oracle_hdr
import oracle_rays_hdr
from test_gpu_shade_rays import _materials_world, _oracle_scene, _ray_mix
from test_gpu_shade_rays_hdr import Checker

pytestmark = pytest.mark.gpu

CAP = 1 << 24
SIZES = ((GW.W, GW.H), GW.RAGGED)                                               # 40 x 24 and 43 x 21
VIEWS = ("outside", "room")                                                     # sky around the room: a channel at 255; the room from inside
SPLITS = ([CAP - 1, 1], [3, CAP - 3], [3, CAP - 4])                             # checked after every chunk that ends at 2^24 - 1 or 2^24
TONEMAPS = (("clamp", 1.0), ("reinhard", 2.5))
VAR_UNKNOWN = np.float32(65504.0) * np.float32(65504.0)
# the opaque bounce route's sky and emissive pixels: the launch is constant in the sample count (measured, see the test), so the cap
BOUNCE_N = CAP


@pytest.fixture(scope="module")
def HL(tmp_path_factory):
    return oracle_hdr.build(tmp_path_factory.mktemp("oracle_hdr"))


@pytest.fixture(scope="module")
def RH(tmp_path_factory):
    return oracle_rays_hdr.build(tmp_path_factory.mktemp("oracle_rays_hdr"))


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def worlds(V):
    """(name, size) -> (texels, tex_dim, camera block)"""
    out = {}
    for name in VIEWS:
        w = GW.world(V, name)
        tex, dim = w.flatten()
        w.close()
        for size in SIZES:
            out[name, size] = (tex, dim, GW.camera(V, name, size))
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert not len(bad), f"{what}: {len(bad)} entries differ; first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


def _open(ctx, worlds, name, size, mode, **kw):
    tex, dim, cam = worlds[name, size]
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    ctx.set_camera(*cam)
    ctx.set_lens(0.0, 1.0)
    ctx.accum_begin(size[0], size[1], 0, mode=mode, jitter=False, **kw)


def _resolves(ctx, hdr, moments):
    """everything the accumulation resolves to, as a dict of arrays"""
    out = dict(zip(("rgba8", "id_dist", "shown"), ctx.accum_resolve()))
    if hdr:
        for op, e in TONEMAPS:
            out.update(zip((f"{op} mean", f"{op} bytes", f"{op} shown"), ctx.accum_resolve_hdr(op, e)))
    if moments:
        out["variance"] = ctx.accum_variance()
    return out


def _walk(ctx, chunks):
    """adds the chunks; yields the total after each chunk that ends at 2^24 - 1 or 2^24"""
    total = 0
    for n in chunks:
        total += n
        assert ctx.accum_add(n) == total
        if total in (CAP - 1, CAP):
            yield total


# ---- a primary mode from the corner: repeat_kernel, repeat_mom_kernel ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "hdr", "moments"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", VIEWS)
@pytest.mark.parametrize("size", SIZES, ids=["40x24", "43x21"])
def test_a_corner_accumulation_at_the_cap_is_its_frame(ctx, worlds, size, name, mode, kind):
    hdr, moments = kind != "plain", kind == "moments"
    kw = dict(hdr=hdr, moments=moments)
    _open(ctx, worlds, name, size, mode, **kw)
    frame = ctx.dispatch(size[0], size[1], mode)
    if name == "outside":                                                       # sky: the byte sums reach 255 * n
        assert (frame[0][..., :3] == 255).any(), "the view holds a channel at 255"
    else:                                                                       # several byte values, all below it
        assert len(np.unique(frame[0][..., :3])) >= 4
    _open(ctx, worlds, name, size, mode, **kw)
    assert ctx.accum_add(1) == 1
    one = _resolves(ctx, hdr, moments)
    _same(one["rgba8"], frame[0], "one sample: the frame's bytes")
    _same(one["id_dist"], frame[1], "one sample: the frame's id_dist")
    if moments:
        assert (_bits(one["variance"]) == _bits(VAR_UNKNOWN)).all(), "n = 1: 65504^2"
    for chunks in SPLITS:
        _open(ctx, worlds, name, size, mode, **kw)
        for total in _walk(ctx, chunks):
            got = _resolves(ctx, hdr, moments)
            for key, want in one.items():
                if key == "variance":
                    assert not _bits(got[key]).any(), f"{chunks} n {total}: the variance is +0 in every bit"
                else:
                    _same(got[key], want, f"{name} {size} mode {mode} {kind} {chunks} n {total}: {key}")


# ---- adaptive: repeat_adaptive_kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hdr", [False, True], ids=["plain", "hdr"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("size", SIZES, ids=["40x24", "43x21"])
def test_adaptive_rounds_to_the_cap(ctx, V, worlds, size, mode, hdr):
    name = "outside"
    _open(ctx, worlds, name, size, mode, hdr=hdr)
    assert ctx.accum_add(1) == 1
    one = _resolves(ctx, hdr, False)
    for rule, stop in (((CAP, CAP, 0), CAP), ((2, CAP, 0), 2)):
        for chunks in SPLITS[:2]:
            _open(ctx, worlds, name, size, mode, hdr=hdr, adaptive=rule)
            for total in _walk(ctx, chunks):
                counts, active = ctx.accum_counts()
                want = min(total, stop)
                assert counts.dtype == np.uint32 and (counts == want).all(), f"{rule} {chunks} round {total}: counts {counts.min()}..{counts.max()}, want {want}"
                assert active == (0 if total >= stop else counts.size), (rule, chunks, total, active)
                got = _resolves(ctx, hdr, False)
                for key, w_ in one.items():
                    _same(got[key], w_, f"{size} mode {mode} rule {rule} {chunks} round {total}: {key}")
            assert total == CAP
            with pytest.raises(V.VrtError, match="vrt error -1"):               # VRT_E_INVALID: the cap counts rounds
                ctx.accum_add(1)
            counts, active = ctx.accum_counts()
            assert (counts == stop).all() and active == 0, "the refused add changed nothing"


# ---- the corner guide ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", VIEWS)
@pytest.mark.parametrize("size", SIZES, ids=["40x24", "43x21"])
def test_corner_guides_at_the_cap_are_one_samples(ctx, worlds, size, name, mode):
    _open(ctx, worlds, name, size, mode)
    assert ctx.accum_add(1) == 1
    one = ctx.accum_guides()
    assert 0 < float(one["coverage"].mean()) and (one["depth"] > 0).any()
    for chunks in SPLITS:
        _open(ctx, worlds, name, size, mode)
        for total in _walk(ctx, chunks):
            got = ctx.accum_guides()
            for key in one:
                _same(got[key], one[key], f"{name} {size} mode {mode} {chunks} n {total}: {key}")
    # ... and brought up to date in two steps: a guide call at 3 samples, then at the cap
    _open(ctx, worlds, name, size, mode)
    assert ctx.accum_add(3) == 3
    ctx.accum_guides()
    assert ctx.accum_add(CAP - 3) == CAP
    got = ctx.accum_guides()
    for key in one:
        _same(got[key], one[key], f"{name} {size} mode {mode} guides at 3 and at 2^24: {key}")


# ---- ray batches in the primary modes ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(V, O):
    """the materials world (emitters, water, glass) and 1250 rays of every kind, as an image 50 wide"""
    w = _materials_world(V)
    tex, dim = w.flatten()
    w.close()
    o, d = _ray_mix(np.random.default_rng(41), 1250, (0, 0, 0), (50, 24, 24), ((30, 2, 8), (36, 8, 14)), ((30, 2, 16), (36, 8, 22)))
    return tex, dim, o, d, _oracle_scene(O, V, tex, dim)


@pytest.mark.parametrize("mode", [0, 1])
def test_primary_ray_batches_at_the_cap_are_one_samples(ctx, batch, mode):
    tex, dim, o, d, _ = batch
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    one = ctx.shade_rays(o, d, mode, width=50, n_samples=1)
    one_hdr = ctx.shade_rays_hdr(o, d, mode, width=50, n_samples=1, tonemap="reinhard", exposure=2.5)
    assert (one[0][:, :3] == 255).any() and float(one_hdr[0].max()) > 1.0
    for n in (CAP - 1, CAP):
        for first in (0, 2 ** 32 - 2):
            got = ctx.shade_rays(o, d, mode, width=50, first_sample=first, n_samples=n)
            for a, b, what in zip(got, one, ("rgba8", "id_dist")):
                _same(a, b, f"vrt_shade_rays mode {mode} n {n} first {first}: {what}")
            got = ctx.shade_rays_hdr(o, d, mode, width=50, first_sample=first, n_samples=n, tonemap="reinhard", exposure=2.5)
            for a, b, what in zip(got, one_hdr, ("rgb", "rgba8", "id_dist")):
                _same(a, b, f"vrt_shade_rays_hdr mode {mode} n {n} first {first}: {what}")


def test_a_callers_sums_at_the_cap(V, O, RH, batch):
    """vrt_shade_rays_hdr_device: 2^24 - 3 samples and then 3 in modes 0 and 1 leave float64(h(c)) * 2^24 in d_sums, exactly; 8
    samples of mode 2 on those sums at n_prior = 2^24 - 8 leave the checker's sequential float64 adds, and their mean over 2^24"""
    tex, dim, o, d, scene = batch
    n = len(d)
    c = V.Context(0)
    bufs = [c.device_alloc(o.nbytes), c.device_alloc(d.nbytes), c.device_alloc(n * 24), c.device_alloc(n * 12), c.device_alloc(n * 4),
            c.device_alloc(n * 8)]
    d_o, d_d, d_sums, d_rgb, d_rgba, d_id = bufs
    try:
        c.upload_octree(tex, dim)
        c.device_write(d_o, o)
        c.device_write(d_d, d)
        ck = Checker(RH, scene, o, d, 50)
        for mode in (0, 1):
            kw = dict(width=50, tonemap="reinhard", exposure=2.5)
            hc, one_rgba, one_id = c.shade_rays_hdr(o, d, mode, n_samples=1, **kw)      # h(c): the one-sample mean
            _same(hc, ck.call(mode, 0, 1)[1], f"mode {mode}: one sample is the checker's")
            c.device_write(d_sums, np.zeros((n, 3), np.float64))
            c.shade_rays_hdr_device(n, d_o, 3, d_d, None, None, None, d_sums, 0, mode=mode, n_samples=CAP - 3, **kw)
            _same(c.device_read(d_sums, (n, 3), np.float64), hc.astype(np.float64) * float(CAP - 3), f"mode {mode}: the sums after 2^24 - 3")
            c.shade_rays_hdr_device(n, d_o, 3, d_d, d_rgb, d_rgba, d_id, d_sums, CAP - 3, mode=mode, first_sample=CAP - 3, n_samples=3, **kw)
            prior = c.device_read(d_sums, (n, 3), np.float64)
            _same(prior, hc.astype(np.float64) * float(CAP), f"mode {mode}: the sums after 2^24 - 3 and 3")
            assert float(prior.max()) > float(CAP), "some colour above 1: the sums are no integers' worth"
            _same(c.device_read(d_rgb, (n, 3), np.float32), hc, f"mode {mode}: the mean over 2^24")
            _same(c.device_read(d_rgba, (n, 4), np.uint8), one_rgba, f"mode {mode}: its bytes")
            _same(c.device_read(d_id, (n, 2), np.int32), one_id, f"mode {mode}: id_dist")
            # mode 2 on those sums
            first = 11
            c.shade_rays_hdr_device(n, d_o, 3, d_d, d_rgb, d_rgba, d_id, d_sums, CAP - 8, mode=2, first_sample=first, n_samples=8, **kw)
            s8, m8, _ = ck.call(2, first, 8, sums=prior, n_prior=CAP - 8)
            assert (_bits(s8) != _bits(prior)).any()
            _same(c.device_read(d_sums, (n, 3), np.float64), s8, f"mode 2 on mode {mode}'s sums: the checker's float64 adds")
            _same(c.device_read(d_rgb, (n, 3), np.float32), m8, f"mode 2 on mode {mode}'s sums: the mean over 2^24")
            _same(c.device_read(d_rgba, (n, 4), np.uint8), oracle_rays_hdr.tonemap(RH, m8, "reinhard", 2.5), f"mode 2 on mode {mode}'s sums: bytes")
    finally:
        for p in bufs:
            c.device_free(p)
        c.close()


# ---- the opaque bounce route's sky and emissive pixels -------------------------------------------------------------------------------
LAMP_POSE = (8.3, 8.7, 12.5, -90.0, 0.0)                                       # four voxels in front of the one voxel, a little off its axis


def _one_lamp(V, size):
    w = V.World()
    w.insert(8, 8, 8, 0xffd2d2ff, 3.0, 1.0, 0.0)                              # opaque (alpha 255, a surface's refraction byte) and emissive
    tex, dim = w.flatten()
    w.close()
    return tex, dim, V.camera_block(LAMP_POSE[:3], LAMP_POSE[3], LAMP_POSE[4], size[0], size[1])[:3]


@pytest.mark.parametrize("kind", ["plain", "hdr", "moments"])
@pytest.mark.parametrize("size", SIZES, ids=["40x24", "43x21"])
def test_sky_and_emissive_pixels_of_the_opaque_route_at_the_cap(ctx, V, O, HL, size, kind):
    """VRT_MODE_FULL from the corner on an opaque tree: pass 1 once, then bounce_accum_kernel. A world of one opaque emissive voxel
    leaves no pixel a diffuse bounce (pass 1 sets the seed's valid bit on an opaque first hit that does not emit, and on nothing
    else), so every lane takes the branch that multiplies pass 1's bytes and float colour by the sample count; the checker's samples
    0, 1 and 7 are the same image. The launch does not loop: an add of 2^12 samples with its resolve and one of 2^18 both measured
    0.08-0.09 ms on the MI355X at both frame sizes, plain, HDR and with moments, so the case runs at the cap."""
    hdr, moments = kind != "plain", kind == "moments"
    W, H = size
    tex, dim, cam = _one_lamp(V, size)
    assert V.tree_is_opaque(tex)
    scene = O.make_scene(tex, dim, *cam)
    samples = [oracle_hdr.render(HL, scene, W, H, 2, k) for k in (0, 1, 7)]
    _same(samples[1], samples[0], "the checker's sample 1 is sample 0")
    _same(samples[2], samples[0], "the checker's sample 7 is sample 0")
    lamp = samples[0].max(axis=2) > 5.0
    assert 40 < lamp.sum() < W * H // 2, "the voxel and sky around it"
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    ctx.set_camera(*cam)
    ctx.set_lens(0.0, 1.0)
    kw = dict(mode=2, jitter=False, hdr=hdr, moments=moments)
    ctx.accum_begin(W, H, 0, **kw)
    assert ctx.accum_add(1) == 1
    one = _resolves(ctx, hdr, moments)
    _same(one["rgba8"], oracle_hdr.rgba_of(HL, samples[0]), "one sample: the checker's bytes")
    assert (one["rgba8"][..., :3] == 255).any()
    if hdr:
        _same(one["clamp mean"], _h(HL, samples[0]), "one sample: the checker's h(c)")
    for chunks in ([BOUNCE_N - 1, 1], [3, BOUNCE_N - 3]):
        ctx.accum_begin(W, H, 0, **kw)
        total = 0
        for n in chunks:
            total += n
            assert ctx.accum_add(n) == total
            if total < BOUNCE_N - 1:
                continue
            got = _resolves(ctx, hdr, moments)
            for key, want in one.items():
                if key == "variance":
                    assert not _bits(got[key]).any(), f"{chunks} n {total}: the variance is +0 in every bit"
                else:
                    _same(got[key], want, f"{size} {kind} {chunks} n {total}: {key}")


def _h(HL, rgb):
    return np.array([oracle_hdr.value(HL, v) for v in rgb.ravel()], np.float32).reshape(rgb.shape)
