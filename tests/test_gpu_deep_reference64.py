"""The path depth, the sun disc and the emitter rules on the gfx950 kernels against the independent float64 restatement
(tests/path_ref64.py with depth=, tan_radius=, emit= and mis=), on the batches, settings, caps and floors of
tests/test_deep_reference64.py -- against the reference, not against the checkers.

The reference is traced once per batch, setting and sample (the batches keep the traces) and reused across routes: vrt_shade_rays
and vrt_shade_rays_hdr, means with tone maps, the HDR accumulation from the corner and from the jittered lens, every shipped
variant, texel and record uploads, and the batch shapes at which the kernels' lane-to-ray map changes. Decided rays are exact in
bytes, ID and dist; floats lie within the reference's bound; the host's emitter list and thresholds are the reference's. Every
test puts the context back to depth 1, radius 0, sampling off, the uniform rule and MIS off."""
import numpy as np
import pytest

import deep_ref64 as DR
import emit_worlds as ew
import lens_ref64 as LR
import oracle_rays
import path_ref64 as PR
import shader_ref64 as R
from test_deep_reference64 import (BATCH_SAMPLES, CAPS, CASE_IDS, CASES, CEILING, MIN_BRANCH, MIS, OFF, POWER, UNIFORM,
                                   DeepBatch, batch, branch_rays, ref_args, sid)
from test_gpu_rays_reference64 import SHAPES, VARIANTS, _params, _resolve_checks
from test_path_reference64 import SAMPLES
from test_rays_reference64 import MEAN_FIRST, MEAN_N, MIN_DECIDED, MIN_DECIDED_HITS, check_floats, check_tonemapped
from test_rays_reference64 import batch as rays_batch
from test_shader_reference64 import scenes  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def RR(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_rays_gpu_deep64"))   # o_frame_rays only: a frame's rays


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _settings(ctx, V, setting):
    D, rad, rule = setting
    ctx.set_path_depth(D)
    ctx.set_sun_disc(rad)
    ctx.set_emitter_sampling(int(rule != OFF))
    ctx.set_emitter_importance(V.EMIT_UNIFORM if rule in (OFF, UNIFORM) else V.EMIT_POWER)
    ctx.set_emitter_mis(int(rule == MIS))


def _restore(ctx, V):
    ctx.set_variant(0)
    ctx.set_params(ctx.default_params())
    ctx.set_path_depth(1)
    ctx.set_sun_disc(0.0)
    ctx.set_emitter_sampling(0)
    ctx.set_emitter_importance(V.EMIT_UNIFORM)
    ctx.set_emitter_mis(0)
    ctx.set_lens(0.0, 1.0)


def _check_list(ctx, b):
    """vrt_emitters and vrt_emitter_cdf of the uploaded tree are the reference's list and table"""
    E = DR.Emitters(b.world)
    assert np.array_equal(ctx.emitters(), E.entries()), "vrt_emitters"
    assert [int(t) for t in ctx.emitter_cdf()] == E.T, "vrt_emitter_cdf"


def _check_bytes(t, rgba, idd, name, setting, what, floors=True):
    f = t.frame()
    r = R.compare(f, rgba, idd)
    dec = f.all_decided()
    share = f.in_world_undecided_share()
    print(f"{what}: in-world {int((~f.outside).sum())} decided {int(dec.sum())} decided hits {int((dec & f.hit).sum())} "
          f"undecided share {share:.4f}")
    assert r["bad"] == 0, (what, r)
    if not floors:
        return dec
    assert dec.sum() >= MIN_DECIDED and (dec & f.hit).sum() >= MIN_DECIDED_HITS, (what, int(dec.sum()), int((dec & f.hit).sum()))
    for branch, rays in branch_rays(t, setting, dec, name).items():
        assert rays.sum() >= MIN_BRANCH, (what, branch, int(rays.sum()))
    cap = CAPS[(name, setting)]
    assert cap <= CEILING[setting[0]] and share <= cap, (what, share, cap)
    return dec


# ---- bytes and floats of every batch and setting -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,setting", CASES, ids=CASE_IDS)
def test_shade_rays_bytes_and_floats(ctx, V, O, RR, scenes, name, setting):
    b = batch(name, V, O, RR, scenes)
    try:
        ctx.upload_octree(b.tex, b.dim)
        _params(ctx, b)
        _settings(ctx, V, setting)
        if setting[2] != OFF:
            _check_list(ctx, b)
        for k in BATCH_SAMPLES[name]:
            what = f"{name} {sid(setting)} sample {k}"
            t = b.deep(setting, k)
            rgba, idd = ctx.shade_rays(b.o, b.d, 2, width=b.width, first_sample=k)
            _check_bytes(t, rgba, idd, name, setting, what)
            rgb, rgba_h, idd_h = ctx.shade_rays_hdr(b.o, b.d, 2, width=b.width, first_sample=k)
            want, bound, dec = t.radiance()
            check_floats(rgb, want, bound, dec, what)
            assert np.array_equal(rgba_h, rgba) and np.array_equal(idd_h, idd), what + ": the HDR form's bytes"
    finally:
        _restore(ctx, V)


MEANS = [("dragon_mix", (3, 0.05, OFF)), ("lamp_room", (3, 0.05, POWER)), ("lamp_room", (3, 0.05, MIS))]
N_MEAN_RAYS = 2000   # a prefix of the batch: eight traces of it stay within a few seconds


@pytest.mark.parametrize("name,setting", MEANS, ids=[f"{n}-{sid(s)}" for n, s in MEANS])
def test_means_and_tone_maps(ctx, V, O, RR, scenes, name, setting):
    b = batch(name, V, O, RR, scenes).prefix(N_MEAN_RAYS)
    try:
        ctx.upload_octree(b.tex, b.dim)
        _params(ctx, b)
        _settings(ctx, V, setting)
        mean, bound, dec = b.mean(setting, MEAN_FIRST, MEAN_N)
        for op, e in (("clamp", 1.0), ("reinhard", 0.25)):
            what = f"{name} {sid(setting)} mean of {MEAN_N} {op} x{e}"
            rgb, rgba, _ = ctx.shade_rays_hdr(b.o, b.d, 2, width=b.width, first_sample=MEAN_FIRST, n_samples=MEAN_N, tonemap=op, exposure=e)
            check_floats(rgb, mean, bound, dec, what)
            check_tonemapped(rgba, mean, bound, dec, op, e, what)
    finally:
        _restore(ctx, V)


# ---- the HDR accumulation ---------------------------------------------------------------------------------------------------------
ACCUM_SETTINGS = [(3, 0.0, OFF), (3, 0.05, OFF), (3, 0.05, UNIFORM), (3, 0.05, MIS)]
_frames = {}


def _frame_batch(name, V, O, RR, scenes):
    """the lamp room's 72 x 44 frame at POSE, or test_rays_reference64's 97 x 55 dragon frame, as the batch of their rays"""
    if name not in _frames:
        if name == "lamp_frame":
            w = ew.lamp_room(V)
            tex, dim = w.flatten()
            rec = np.array(w.records()[0], np.uint32).copy()
            w.close()
            cam = V.camera_block(ew.POSE[:3], ew.POSE[3], ew.POSE[4], ew.W, ew.H)[:3]
            o, d = oracle_rays.frame_rays(RR, O.make_scene(tex, dim, *cam), ew.W, ew.H)
            _frames[name] = DeepBatch(tex, dim, o, d, ew.W, cam=cam, records=rec)
        else:
            src = rays_batch("dragon_frame", V, O, RR, scenes)
            b = DeepBatch(src.tex, src.dim, src.o, src.d, src.width, cam=src.cam)
            b._world = src.world
            _frames[name] = b
    return _frames[name]


class _AtSetting:
    """a frame batch seen by test_gpu_rays_reference64._resolve_checks: mean(mode, first, n) at one setting"""

    def __init__(self, b, setting):
        self.b, self.setting, self.width, self.d = b, setting, b.width, b.d

    def mean(self, mode, first, n):
        assert mode == 2
        return self.b.mean(self.setting, first, n)


@pytest.mark.parametrize("setting", ACCUM_SETTINGS, ids=[sid(s) for s in ACCUM_SETTINGS])
@pytest.mark.parametrize("name", ["lamp_frame", "dragon_frame"])
def test_hdr_accumulation_from_the_corner(ctx, V, O, RR, scenes, name, setting):
    """one accum_add(1) at two sample indices, then 3 + 5 from MEAN_FIRST: floats, two tone maps, host and device resolve"""
    b = _frame_batch(name, V, O, RR, scenes)
    W, H = b.width, len(b.d) // b.width
    view = _AtSetting(b, setting)
    try:
        ctx.upload_octree(b.tex, b.dim)
        _params(ctx, b)
        _settings(ctx, V, setting)
        for k in (SAMPLES[3], MEAN_FIRST + 1):
            ctx.accum_begin(W, H, first_sample=k, mode=2, hdr=True)
            assert ctx.accum_add(1) == 1
            _resolve_checks(ctx, view, 2, k, 1, f"{name} {sid(setting)} sample {k}")
        ctx.accum_begin(W, H, first_sample=MEAN_FIRST, mode=2, hdr=True)
        assert ctx.accum_add(3) == 3 and ctx.accum_add(5) == 8
        _resolve_checks(ctx, view, 2, MEAN_FIRST, 8, f"{name} {sid(setting)} 3 + 5 samples")
    finally:
        _restore(ctx, V)


def test_hdr_accumulation_from_the_jittered_lens(ctx, V, O, RR, scenes):
    """the lens + jitter source at (3, 0.05, mis) on the lamp room, through PathTrace.lens"""
    setting = (3, 0.05, MIS)
    b = _frame_batch("lamp_frame", V, O, RR, scenes)
    W, H = ew.W, ew.H
    try:
        ctx.upload_octree(b.tex, b.dim)
        _params(ctx, b)
        _settings(ctx, V, setting)
        ctx.set_lens(*ew.LENS)
        for k in (SAMPLES[1], MEAN_FIRST):
            what = f"lamp room lens + jitter {sid(setting)} sample {k}"
            rays = LR.lens_rays(*b.cam, W, H, sample=k, jitter=True, aperture=ew.LENS[0], focus=ew.LENS[1])
            assert rays.moved.any()
            t = PR.PathTrace.lens(b.world, rays, voxel_scale=b.scale, global_light=b.gl, light_dir=b.light, **ref_args(setting))
            want, bound, dec = t.radiance()
            ctx.accum_begin(W, H, first_sample=k, mode=2, jitter=True, hdr=True)
            assert ctx.accum_add(1) == 1
            rgb, rgba, _ = ctx.accum_resolve_hdr("reinhard", 0.25)
            print(f"{what}: undecided share {1.0 - dec.mean():.4f} connections {int((dec & (t.stats['conn_contributing'] > 0)).sum())}")
            assert (dec & (t.stats["conn_contributing"] > 0)).sum() >= MIN_BRANCH
            check_floats(rgb.reshape(-1, 3), want, bound, dec, what)
            check_tonemapped(rgba.reshape(-1, 4), want, bound, dec, "reinhard", 0.25, what)
    finally:
        _restore(ctx, V)


# ---- uploads and variants ---------------------------------------------------------------------------------------------------------
ROUTES = [("lamp_room", (3, 0.05, MIS)), ("dragon_mix", (8, 0.0, OFF))]


@pytest.mark.parametrize("name,setting", ROUTES, ids=[f"{n}-{sid(s)}" for n, s in ROUTES])
def test_every_variant_and_a_record_upload(ctx, V, O, RR, scenes, name, setting):
    b = batch(name, V, O, RR, scenes)
    k = BATCH_SAMPLES[name][0]
    t = b.deep(setting, k)
    want, bound, dec = t.radiance()
    w = b.make_world()
    n = 0
    try:
        for up, do in (("texels", lambda: ctx.upload_octree(b.tex, b.dim)), ("records", lambda: ctx.upload_records(*w.records()))):
            do()
            _params(ctx, b)
            _settings(ctx, V, setting)
            if setting[2] != OFF:
                _check_list(ctx, b)
            for v in (VARIANTS if up == "texels" else VARIANTS[:1]):
                ctx.set_variant(v)
                what = f"{name} {sid(setting)} {up} variant {v} sample {k}"
                rgb, rgba, idd = ctx.shade_rays_hdr(b.o, b.d, 2, width=b.width, first_sample=k)
                _check_bytes(t, rgba, idd, name, setting, what)
                check_floats(rgb, want, bound, dec, what)
                n += 1
    finally:
        w.close()
        _restore(ctx, V)
    assert n == len(VARIANTS) + 1


# ---- batch shapes -----------------------------------------------------------------------------------------------------------------
def test_batch_shapes(ctx, V, O, RR, scenes):
    """test_gpu_rays_reference64's SHAPES at (3, 0.05, mis) on the lamp room: the reference at the shape's own RNG pixels"""
    setting = (3, 0.05, MIS)
    b = batch("lamp_room", V, O, RR, scenes)
    o, d = np.ascontiguousarray(b.o[:300]), np.ascontiguousarray(b.d[:300])
    checked = 0
    try:
        ctx.upload_octree(b.tex, b.dim)
        _params(ctx, b)
        _settings(ctx, V, setting)
        for n, width in SHAPES:
            for stride in (3, 0):
                oo = o[:n] if stride == 3 else np.ascontiguousarray(np.tile(o[0], (n, 1)))
                what = f"shape {n} x {width} stride {stride}"
                t = b.deep_at(setting, 5, oo, d[:n], width)
                rgb, rgba, idd = ctx.shade_rays_hdr(oo if stride == 3 else o[0], d[:n], 2, width=width, first_sample=5)
                r = R.compare(t.frame(), rgba, idd)
                assert r["bad"] == 0, (what, r)
                want, bound, dec = t.radiance()
                check_floats(rgb, want, bound, dec, what, min_decided=0)
                checked += int(t.frame().all_decided().sum())
    finally:
        _restore(ctx, V)
    assert checked > 0.85 * 2 * sum(n for n, _ in SHAPES), checked
