"""The ray-batch and HDR checkers (tests/oracle_rays.c, oracle_hdr.c, oracle_rays_hdr.c) against the independent float64
restatements (tests/shader_ref64.py for modes 0 and 1, tests/path_ref64.py for mode 2).

A batch is a frame's rays or test_gpu_shade_rays's mix of origins and directions. Every decided ray must agree exactly in
bytes, voxel ID and dist, and its unclamped float colour must lie within the reference's float32 bound; means over samples
and both tone maps carry that bound through. Rays whose origin is outside the world are not restated (the GLSL leaves the
node box undefined there) and are compared nowhere. Each batch states its measured undecided share beside its cap, and
planted misreadings of the entry and of the HDR arithmetic show that the comparison fails when it should."""
import os

import numpy as np
import pytest

import oracle_adaptive
import oracle_hdr
import oracle_rays
import oracle_rays_hdr
import path_ref64 as PR
import shader_ref64 as R
from conftest import MAPS, random_voxels, room_world
from test_gpu_shade_rays import _materials_world, _ray_mix
from test_path_reference64 import SAMPLES
from test_path_reference64 import check as check_path
from test_shader_reference64 import POSES, UNDECIDED_CAP, _slab, _world, light_dir_bits, scenes  # noqa: F401
from test_shader_reference64 import check as check_shader

F = np.float32
MODES = (0, 1, 2)
MIN_DECIDED, MIN_DECIDED_HITS = 1000, 300
MEAN_FIRST, MEAN_N = 7, 8
TONEMAPS = [(op, e) for op in ("clamp", "reinhard") for e in (0.25, 1.0, 4.0)]
DRAGON_MIX = ((0, 0, 0), (126, 95, 60), ((40, 2, 20), (80, 6, 40)), ((50, 1, 25), (70, 4, 35)))
ROOM_MIX = ((0, 0, 0), (120, 64, 120), ((10, 20, 10), (20, 40, 20)), ((0, 0, 0), (120, 1, 120)))
MATERIALS_MIX = ((0, 0, 0), (50, 24, 24), ((30, 2, 8), (36, 8, 14)), ((30, 2, 16), (36, 8, 22)))
BOUNDS = ((-64,) * 3, (192,) * 3)
BOUNDS_MIX = ((-60, -60, -60), (70, 70, 70), ((-10, -10, -10), (10, 10, 10)), ((-30, -30, -30), (-20, -20, -20)))
# rays per mix for ~2,000 in-world ones: an eighth starts outside the world, and another eighth (the other octants) is outside
# the custom bounds; the room's sparse content takes more rays to 300 decided hits
N_MIX = {"dragon_mix": 2300, "room_mix": 2800, "materials_1": 2300, "materials_0.5": 2300, "materials_2": 2300, "bounds_mix": 3300}

# Undecided share of the in-world rays (any field of the ray undecided), measured on the reference alone, per mode; the cap
# is that share plus a quarter of itself, rounded up to the next 0.005. Frames keep the caps of their scenes
# (test_shader_reference64 / test_path_reference64, of the hit pixels).
# name: (cap mode 0, cap mode 1, cap mode 2)            measured mode 0 / 1 / 2 (the worse of the batch's two samples)
MIX_CAPS = {
    "dragon_mix":    (0.015, 0.015, 0.010),            # 0.94 % / 0.94 % / 0.74 %
    "room_mix":      (0.005, 0.005, 0.010),            # 0.28 % / 0.28 % / 0.77 %
    "materials_1":   (0.010, 0.010, 0.040),            # 0.45 % / 0.45 % / 3.04 %
    "materials_0.5": (0.010, 0.010, 0.040),            # 0.45 % / 0.45 % / 2.84 %
    "materials_2":   (0.005, 0.005, 0.035),            # 0.40 % / 0.40 % / 2.69 %
    "bounds_mix":    (0.055, 0.060, 0.110),            # 4.20 % / 4.45 % / 8.70 % (unit voxels scattered in air: many grazing steps)
}
FRAMES = {"dragon_frame": ("dragon", "dragon", 97, 55, 2400, 2450), "room_frame": ("room", "room_inside", 83, 49, 1700, 3580)}
# the mode-2 samples of each batch, from SAMPLES: every index on the frames, two per mix so that each index is met
MIX_SAMPLES = {name: (SAMPLES[k % 5], SAMPLES[(k + 2) % 5]) for k, name in enumerate(MIX_CAPS)}
ALL = sorted(FRAMES) + sorted(MIX_CAPS)


@pytest.fixture(scope="module")
def RR(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_rays_ref64"))


@pytest.fixture(scope="module")
def RH(tmp_path_factory):
    return oracle_rays_hdr.build(tmp_path_factory.mktemp("oracle_rays_hdr_ref64"))


@pytest.fixture(scope="module")
def HD(tmp_path_factory):
    return oracle_hdr.build(tmp_path_factory.mktemp("oracle_hdr_ref64"))


class Batch:
    """rays + texels + uniforms: shaded by the checkers, traced by the references (each trace made once and kept)"""

    def __init__(self, tex, dim, o, d, width, scale=1.0, wmin=(-1023,) * 3, wmax=(1024,) * 3, gl=(1, 1, 1, 1), cam=None):
        self.tex, self.dim, self.o, self.d, self.width = tex, dim, np.ascontiguousarray(o, F), np.ascontiguousarray(d, F), width
        self.scale, self.wmin, self.wmax, self.gl, self.light, self.cam = scale, wmin, wmax, gl, light_dir_bits(), cam
        self._world = None
        self._traces = {}
        self.make_world = None    # -> an open product World of the same content (for record uploads and edits)

    @property
    def world(self):
        if self._world is None:
            self._world = R.World(self.tex, self.dim, self.wmin, self.wmax)
        return self._world

    def scene(self, O, V):
        cam = self.cam if self.cam is not None else V.camera_block((63.5, 60.5, 140.5), -90.0, -10.0, 64, 64)[:3]
        s = O.make_scene(self.tex, self.dim, *cam)
        s.voxel_scale = self.scale
        s.bounds_min[:], s.bounds_max[:] = list(self.wmin), list(self.wmax)
        s.global_light[:] = [float(v) for v in self.gl]
        s.light_dir[:] = [float(v) for v in self.light]
        return s

    def trace(self, mode, sample=0, flaws=(), o=None, d=None, width=None):
        """the reference's trace for the mode: shader_ref64.Trace (0, 1: no random number, one trace) or PathTrace (2)"""
        key = (2, sample & 0xFFFFFFFF) if mode == 2 else (0, 0)
        fresh = bool(flaws) or o is not None or d is not None or width is not None
        if fresh or key not in self._traces:
            cls = PR.PathTrace if mode == 2 else R.Trace
            t = cls.rays(self.world, self.o if o is None else o, self.d if d is None else d, self.width if width is None else width,
                         sample=sample, voxel_scale=self.scale, global_light=self.gl, light_dir=self.light, flaws=flaws)
            if fresh:
                return t
            self._traces[key] = t
        return self._traces[key]

    def frame(self, mode, sample=0, **kw):
        t = self.trace(mode, sample, **kw)
        return t.frame() if mode == 2 else t.frame(mode)

    def radiance(self, mode, sample=0, **kw):
        t = self.trace(mode, sample, **kw)
        return t.radiance() if mode == 2 else t.radiance(mode)

    def mean(self, mode, first, n, flaws=()):
        """(mean, bound, decided) of samples first .. first + n - 1 (modes 0 and 1: every sample is the same)"""
        rad = [self.radiance(mode, first + k if mode == 2 else 0) for k in range(n if mode == 2 else 1)]
        return R.hdr_mean([r[0] for r in rad], [r[1] for r in rad], [r[2] for r in rad], flaws)


_batches = {}


def vox_world(V, name):
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, name + ".vox"))
    return w


def batch(name, V, O, RR, scenes):
    if name in _batches:
        return _batches[name]
    if name in FRAMES:
        scene, pose, W, H, _, _ = FRAMES[name]
        tex, dim = scenes[scene]
        cam = V.camera_block(POSES[pose][:3], POSES[pose][3], POSES[pose][4], W, H)[:3]
        o, d = oracle_rays.frame_rays(RR, O.make_scene(tex, dim, *cam), W, H)
        b = Batch(tex, dim, o, d, W, cam=cam)
        b.make_world = (lambda: room_world(V)) if scene == "room" else (lambda: vox_world(V, scene))
    elif name in ("dragon_mix", "room_mix"):
        tex, dim = scenes[name[:-4]]
        o, d = _ray_mix(np.random.default_rng(51 if name == "dragon_mix" else 52), N_MIX[name], *(DRAGON_MIX if name == "dragon_mix" else ROOM_MIX))
        b = Batch(tex, dim, o, d, 64 if name == "dragon_mix" else 7)
        b.make_world = (lambda: room_world(V)) if name == "room_mix" else (lambda: vox_world(V, "dragon"))
    elif name.startswith("materials_"):
        scale = float(name.split("_")[1])
        w = _materials_world(V)
        tex, dim = w.flatten()
        w.close()
        o, d = _ray_mix(np.random.default_rng(53), N_MIX[name], *MATERIALS_MIX)
        b = Batch(tex, dim, o / F(scale), d, 64, scale=scale, gl=(1, 1, 1, 1) if scale == 1.0 else (0.9, 0.8, 0.6, 1.0))
        b.make_world = lambda: _materials_world(V)
    else:
        assert name == "bounds_mix", name
        xyz, rgba = random_voxels(np.random.default_rng(4), 20000, -60, 70, n_colors=7)
        w = V.World(world_min=BOUNDS[0], world_max=BOUNDS[1])
        w.insert_many(xyz, rgba)
        tex, dim = w.flatten()
        w.close()
        o, d = _ray_mix(np.random.default_rng(54), N_MIX[name], *BOUNDS_MIX)
        b = Batch(tex, dim, o, d, 13, wmin=BOUNDS[0], wmax=BOUNDS[1])

        def bounds_world():
            w = V.World(world_min=BOUNDS[0], world_max=BOUNDS[1])
            w.insert_many(xyz, rgba)
            return w
        b.make_world = bounds_world
    _batches[name] = b
    return b


def samples_of(name, mode):
    return (0,) if mode != 2 else (SAMPLES if name in FRAMES else MIX_SAMPLES[name])


def check_bytes(f, rgba, idd, name, mode, what):
    """every decided ray exact in bytes, ID and dist; the batch's floor of decided rays and its cap"""
    if name in FRAMES:
        _, _, _, _, hits01, hits2 = FRAMES[name]
        if mode == 2:
            return check_path(f, rgba, idd, hits2, 0.04, what)
        return check_shader(f, rgba, idd, hits01, what, UNDECIDED_CAP)
    r = R.compare(f, rgba, idd)
    dec = f.all_decided()
    share = f.in_world_undecided_share()
    print(f"{what}: in-world {int((~f.outside).sum())} decided {int(dec.sum())} decided hits {int((dec & f.hit).sum())} "
          f"undecided share {share:.4f}")
    assert r["bad"] == 0, (what, r)
    assert not (f.outside & (f.dec_id | f.dec_dist | f.dec_rgb.any(1))).any()
    assert dec.sum() >= MIN_DECIDED and (dec & f.hit).sum() >= MIN_DECIDED_HITS, (what, int(dec.sum()), int((dec & f.hit).sum()))
    cap = MIX_CAPS[name][mode]
    assert cap <= 0.15 and share <= cap, (what, share, cap)
    return r


def check_floats(got, want, bound, dec, what, min_decided=MIN_DECIDED):
    """|got - want| <= bound on the decided rays (got: the checker's or the device's float32[n, 3], through h already)"""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got[dec]).all(), f"{what}: NaN or infinity in a decided ray"
    err = np.abs(R.hdr_value(got) - want)
    bad = dec & (err > bound).any(1)
    print(f"{what}: decided {int(dec.sum())} peak {want[dec].max() if dec.any() else 0:.3f} worst err / bound "
          f"{np.max(np.where(bound[dec] > 0, err[dec] / np.where(bound[dec] > 0, bound[dec], 1), err[dec] > 0), initial=0):.3f}")
    assert dec.sum() >= min_decided, (what, int(dec.sum()))
    assert not bad.any(), (what, int(bad.sum()), int(np.nonzero(bad)[0][0]), got[bad][0], want[bad][0], bound[bad][0])


def check_tonemapped(rgba, mean, bound, dec, op, e, what):
    """decided bytes of the tone-mapped mean equal the reference's; alpha 255"""
    want, dec_b, _, _ = R.tonemap(mean, bound, op, e)
    ok = dec[:, None] & dec_b
    got = np.asarray(rgba)[:, :3].astype(np.int64)
    assert ok.sum() >= 3 * MIN_DECIDED * 0.8, (what, int(ok.sum()))
    assert np.array_equal(got[ok], want[ok]), (what, np.argwhere(ok & (got != want))[:5])
    assert np.all(np.asarray(rgba)[:, 3] == 255), what


# ---- bytes, ID and dist ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_ray_batches_match_the_references(V, O, RR, scenes, name):
    """a frame's rays (o_frame_rays) and arbitrary rays in modes 0, 1 and 2: every decided ray exact"""
    b = batch(name, V, O, RR, scenes)
    s = b.scene(O, V)
    seen = set()
    for mode in MODES:
        for k in samples_of(name, mode):
            rgba, idd = oracle_rays.shade(RR, s, b.o, b.d, mode, b.width, k)
            check_bytes(b.frame(mode, k), rgba, idd, name, mode, f"{name} mode {mode} sample {k}")
            seen.add((mode, rgba.tobytes()))
    assert len(seen) == sum(len(samples_of(name, m)) for m in MODES)


def test_a_frames_rays_are_the_frame(V, O, RR, scenes):
    """the refactor's other half: the batch entry on a frame's rays decides what the camera constructor decides"""
    for name in FRAMES:
        scene, pose, W, H, _, _ = FRAMES[name]
        b = batch(name, V, O, RR, scenes)
        f = PR.PathTrace(b.world, *b.cam, W, H, sample=1, light_dir=b.light).frame()
        g = b.frame(2, 1)
        both = f.all_decided() & g.all_decided()
        assert both.mean() > 0.9
        assert np.array_equal(f.rgba[both], g.rgba[both]) and np.array_equal(f.id[both], g.id[both])
        assert np.array_equal(f.dist[both], g.dist[both])


# ---- HDR floats of one sample ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_hdr_floats_of_one_sample(V, O, RR, RH, scenes, name):
    b = batch(name, V, O, RR, scenes)
    s = b.scene(O, V)
    for mode in MODES:
        k = samples_of(name, mode)[0]
        rgb, _ = oracle_rays_hdr.shade(RH, s, b.o, b.d, mode, b.width, k)
        want, bound, dec = b.radiance(mode, k)
        assert np.isfinite(rgb[~b.trace(mode, k).outside]).all(), "NaN or infinity on the checker's side"
        check_floats(rgb, want, bound, dec, f"{name} mode {mode} sample {k}")


# ---- HDR means and tone maps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["materials_1", "room_mix"])
def test_hdr_means_and_tone_maps(V, O, RR, RH, scenes, name):
    b = batch(name, V, O, RR, scenes)
    s = b.scene(O, V)
    for mode in (1, 2):
        got = oracle_rays_hdr.Batch(RH, s, b.o, b.d, mode, b.width).add(MEAN_FIRST, MEAN_N).mean()
        mean, bound, dec = b.mean(mode, MEAN_FIRST, MEAN_N)
        check_floats(got, mean, bound, dec, f"{name} mode {mode} mean of {MEAN_N}")
        if name == "materials_1":
            assert mean[dec].max() > 4.0, "the emitters give no mean far above 1"
        for op, e in TONEMAPS:
            check_tonemapped(oracle_rays_hdr.tonemap(RH, got, op, e), mean, bound, dec, op, e, f"{name} mode {mode} {op} x{e}")


def test_tone_map_bounds_by_hand():
    """clamp scales the bound by the exposure; Reinhard's never exceeds e * b + 3u (its slope and value are <= 1)"""
    mean = np.array([[0.0, 0.5, 2.0], [10.0, 65504.0, 1e-3]])
    bound = np.full_like(mean, 1e-6)
    for e in (0.25, 1.0, 4.0):
        _, _, y, b = R.tonemap(mean, bound, "clamp", e)
        assert np.array_equal(y, e * mean) and np.array_equal(b, e * bound)
        _, _, y, b = R.tonemap(mean, bound, "reinhard", e)
        assert np.allclose(y, e * mean / (1 + e * mean)) and np.all(b <= e * bound + 3 * R.U) and np.all(b >= e * bound)
    bytes_, dec, _, _ = R.tonemap(np.array([[0.5 / 255, 1.5 / 255 + 1e-5, 3.0]]), np.full((1, 3), 1e-6), "clamp", 1.0)
    assert dec.tolist() == [[False, True, True]] and bytes_[0, 1:].tolist() == [2, 255]
    m, b, d = R.hdr_mean([np.array([[2.0, -1.0, 1e9]]), np.array([[4.0, 1.0, 0.0]])], [np.full((1, 3), 1e-6)] * 2,
                         [np.array([True]), np.array([False])])
    assert m.tolist() == [[3.0, 0.5, 32752.0]] and not d[0] and np.allclose(b, 1e-6 + R.U * m)


# ---- the adaptive HDR accumulation ------------------------------------------------------------------------------------------
def test_adaptive_hdr_means_cover_each_pixels_own_samples(V, O, RR, HD, scenes):
    """oracle_hdr.Accum under the adaptive rule (oracle_adaptive): a pixel with count n_p holds the reference's mean over
    samples first .. first + n_p - 1"""
    name = "dragon_frame"
    _, _, W, H, _, _ = FRAMES[name]
    b = batch(name, V, O, RR, scenes)
    s = b.scene(O, V)
    rule, rounds = (2, 6, 3), 6
    acc = oracle_hdr.Accum(HD, H, W, rule)
    for r in range(rounds):
        acc.add(oracle_hdr.render(HD, s, W, H, 2, MEAN_FIRST + r))
    check_adaptive(b, acc.counts().ravel(), acc.mean().reshape(-1, 3), rule, "dragon adaptive")


def check_adaptive(b, counts, got, rule, what):
    assert counts.min() >= rule[0] and counts.max() <= rule[1] and len(np.unique(counts)) > 1, np.unique(counts)
    checked = 0
    for n in np.unique(counts):
        mean, bound, dec = b.mean(2, MEAN_FIRST, int(n))
        sel = dec & (counts == n)
        assert np.isfinite(got[sel]).all()
        bad = sel & (np.abs(R.hdr_value(got.astype(np.float64)) - mean) > bound).any(1)
        assert not bad.any(), (what, int(n), int(bad.sum()))
        checked += int(sel.sum())
    assert checked > 0.85 * counts.size, (what, checked)


# ---- the comparison can fail: one planted misreading at a time ----------------------------------------------------------------
def emitter_world(V):
    """a floor and a WHITE emitter of illumination 1: rgb * illumination is 1.0 with or without the * 10, so its bytes are
    255 either way"""
    vox = _slab(0, 24, 0, 1, 0, 24) + _slab(8, 16, 4, 12, 8, 16, c=0xFFFFFFFF, r=3.0, i=1.0)
    return _world(V, vox)


def emitter_batch(V):
    tex, dim = emitter_world(V)
    rng = np.random.default_rng(55)
    o = np.array([12.0, 8.0, 40.0]) + rng.random((1500, 3)) * 4.0
    d = np.array([8.0, 4.0, 8.0]) + rng.random((1500, 3)) * 8.0 - o
    d *= 10.0 ** rng.uniform(-3.0, 3.0, size=(1500, 1))
    return Batch(tex, dim, o, d, 64)


RAY_MUTATIONS = {"rays_shared_medium": ("materials_1", (0, 2)), "rays_dist_from_first_origin": ("dragon_mix", (0, 2)),
                 "rays_rng_linear": ("dragon_mix", (2,)), "rays_dir_length": ("materials_1", (0, 2)),
                 "hdr_deep_sky_no_sun": ("dragon_mix", (2,))}


@pytest.mark.parametrize("flaw", sorted(R.RAY_FLAWS))
def test_each_planted_ray_flaw_is_detected(V, O, RR, RH, scenes, flaw):
    assert set(RAY_MUTATIONS) | {"hdr_clamp_before_mean", "hdr_emission_x1"} == set(R.RAY_FLAWS)
    if flaw == "hdr_emission_x1":
        # invisible to the bytes, visible to the floats
        b = emitter_batch(V)
        s = b.scene(O, V)
        for mode in (0, 2):
            rgba, idd = oracle_rays.shade(RR, s, b.o, b.d, mode, b.width, 0)
            rgb, _ = oracle_rays_hdr.shade(RH, s, b.o, b.d, mode, b.width, 0)
            good, flawed = b.frame(mode), b.frame(mode, flaws=(flaw,))
            emitter = flawed.all_decided() & (rgb.min(1) > 5.0)
            assert emitter.sum() > 300, int(emitter.sum())
            assert R.compare(good, rgba, idd)["bad"] == 0 and R.compare(flawed, rgba, idd)["bad"] == 0   # bytes: 255 either way
            want, bound, dec = b.radiance(mode)
            assert not (dec & (np.abs(rgb - want) > bound).any(1)).any()
            want, bound, dec = b.radiance(mode, flaws=(flaw,))
            assert (dec & (np.abs(rgb - want) > bound).any(1)).sum() >= emitter.sum()                     # floats: 10 against 1
        return
    if flaw == "hdr_clamp_before_mean":
        b = batch("materials_1", V, O, RR, scenes)
        got = oracle_rays_hdr.Batch(RH, b.scene(O, V), b.o, b.d, 2, b.width).add(MEAN_FIRST, MEAN_N).mean()
        mean, bound, dec = b.mean(2, MEAN_FIRST, MEAN_N, flaws=(flaw,))
        assert (dec & (np.abs(got - mean) > bound).any(1)).sum() > 50
        return
    name, modes = RAY_MUTATIONS[flaw]
    b = batch(name, V, O, RR, scenes)
    s = b.scene(O, V)
    bad = 0
    for mode in modes:
        k = samples_of(name, mode)[0]
        rgba, idd = oracle_rays.shade(RR, s, b.o, b.d, mode, b.width, k)
        bad += R.compare(b.frame(mode, k, flaws=(flaw,)), rgba, idd)["bad"]
    assert bad > 0, flaw
