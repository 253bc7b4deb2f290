"""The CPU oracle's VRT_MODE_FULL against the independent float64 restatement of pathTrace (tests/path_ref64.py).

Every decided pixel must agree exactly (rgb bytes, voxel ID, dist); each frame states how many decided hit pixels it
checked and caps the undecided share, so no frame passes by deciding nothing. Glass edge worlds pin that the cases they
are built for (a full stack, TIR, absorption, light only a bounce finds, an eye in glass, the ID-0 re-entry) occur in
decided pixels, and planted misreadings show that the comparison fails when the ray tree is read differently. The det_*
routines that stand in for exp, pow, sin and cos are measured against float64 here; path_ref64's error model uses the
same bounds."""
import numpy as np
import pytest

import oracle_samples
import path_ref64 as PR
import shader_ref64 as R
from test_shader_reference64 import GREY, OPAQUE, POSES, Case, _slab, _world, edge_cases, ref_world, scenes  # noqa: F401

# the sample indices of initRNG checked: 0, 1, a middle one, 2^24 - 1, and 54435, the first whose sampleIndex * 78901 wraps 2^32
SAMPLES = (0, 1, 1000, (1 << 24) - 1, 54435)


def trace(c, world, sample=0, flaws=()):
    return PR.PathTrace(world, *c.cam, c.W, c.H, sample=sample, voxel_scale=c.scale, global_light=c.gl, light_dir=c.light,
                        highlighted=c.hl, flaws=flaws).frame()


def check(f, rgba, idd, min_decided_hits, cap, what):
    r = R.compare(f, rgba, idd)
    assert r["bad"] == 0, (what, r)
    assert r["decided_hits"] >= min_decided_hits, (what, r)
    assert r["undecided_share"] <= cap, (what, r)
    return r


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    return oracle_samples.build(tmp_path_factory.mktemp("oracle_samples_path"))


def oracle_sample(S, O, c, sample):
    s = O.make_scene(c.tex, c.dim, *c.cam, highlighted=c.hl)
    s.voxel_scale = c.scale
    s.bounds_min[:], s.bounds_max[:] = list(c.wmin), list(c.wmax)
    s.global_light[:] = [float(v) for v in c.gl]
    s.light_dir[:] = [float(v) for v in c.light]
    return oracle_samples.render_sample(S, s, c.W, c.H, O.MODE_FULL, sample)


# ---- the det_* routines against float64, on the domains the shader feeds them ---------------------------------------------
def det_errors(exp, pw, sin, cos):
    """-> measured maxima: exp relative on [-87, 0], its absolute error below, pow(x, 5) relative on [0, 1] where
    x^5 >= 1.7e-38 and absolute below, sin / cos absolute on [0, 2 pi)"""
    x = np.concatenate([np.linspace(-87.0, 0.0, 400001), -np.logspace(-8, 0, 20001)]).astype(np.float32)
    got, want = exp(x).astype(np.float64), np.exp(x.astype(np.float64))
    lo = np.linspace(-88.0, -87.0, 1001).astype(np.float32)[:-1]
    e_lo = np.abs(exp(lo).astype(np.float64) - np.exp(lo.astype(np.float64))).max()
    out = {"exp": (np.abs(got - want) / want).max(), "exp_underflow_abs": e_lo}
    x = np.concatenate([np.linspace(0.0, 1.0, 400001), np.logspace(-9, 0, 40001)]).astype(np.float32)
    got, want = pw(x, np.full_like(x, 5.0)).astype(np.float64), x.astype(np.float64) ** 5
    ok = want >= 1.7e-38
    out["pow"] = (np.abs(got[ok] - want[ok]) / want[ok]).max()
    out["pow_abs_below"] = np.abs(got[~ok] - want[~ok]).max()
    x = np.linspace(0.0, 2 * np.pi, 400001).astype(np.float32)
    x = x[x < 2 * np.pi]
    out["sin"] = np.abs(sin(x).astype(np.float64) - np.sin(x.astype(np.float64))).max()
    out["cos"] = np.abs(cos(x).astype(np.float64) - np.cos(x.astype(np.float64))).max()
    return out


def assert_det_bounds(e):
    """each stated bound holds and is no looser than twice what is measured"""
    assert e["exp"] <= PR.E_EXP <= 2 * e["exp"], e
    assert e["exp_underflow_abs"] <= 1.7e-38, e
    assert e["pow"] <= PR.E_POW <= 2 * e["pow"], e
    assert e["pow_abs_below"] <= PR.E_POW_ABS, e
    assert max(e["sin"], e["cos"]) <= PR.E_SINCOS <= 2 * min(e["sin"], e["cos"]), e


def test_det_routines_against_float64(O):
    L = O.lib()
    vec = lambda fn: np.vectorize(lambda *a: fn(*(float(v) for v in a)), otypes=[np.float32])
    assert_det_bounds(det_errors(vec(L.o_det_expf), vec(L.o_det_powf), vec(L.o_det_sinf), vec(L.o_det_cosf)))


def test_rng_and_hemisphere_restatement():
    """initRNG / rand in uint32 arithmetic: a few states by hand, the wrap of sampleIndex * 78901, the float32 conversion that
    can give 1.0, and cosineSampleHemisphere returning unit vectors on the normal's side"""
    st = PR.init_rng(np.array([0, 5]), np.array([0, 7]), 0)
    seed = (np.array([0, 5 + 7 * 1920]) + 123456) & 0xFFFFFFFF
    s1 = (seed * 747796405 + 2891336453) & 0xFFFFFFFF
    word = (((s1 >> ((s1 >> 28) + 4)) ^ s1) * 277803737) & 0xFFFFFFFF
    assert np.array_equal(st, (word >> 22) ^ word)
    assert np.array_equal(PR.init_rng([3], [4], 54435), PR.init_rng([3], [4], 54435 - (1 << 32)))
    assert (54435 * 78901) >> 32 == 1 and (54434 * 78901) >> 32 == 0
    _, v = PR.rand(np.arange(1 << 16, dtype=np.int64) * 65537)
    assert v.min() >= 0.0 and v.max() <= 1.0
    assert np.float32(np.float64(0xFFFFFFFF)) / np.float32(4294967296.0) == 1.0   # C10: float(uint) may round up to 2^32
    rng = np.random.default_rng(4)
    for ax in range(3):
        for s in (1.0, -1.0):
            n = np.zeros((2000, 3))
            n[:, ax] = s
            d = PR.cosine_hemisphere(n, rng.random(2000), rng.random(2000))
            assert np.allclose(np.linalg.norm(d, axis=1), 1.0) and np.all((d * n).sum(1) >= 0)


# ---- the model scenes and the room ----------------------------------------------------------------------------------------
# min_hits: decided hit pixels (~90 % of what was measured). Measured undecided shares of the hit pixels: dragon 0.3 %,
# dragon_inside 0.2 %, monu9 0.3 %, nature 0.5 %, room_inside 3.3 %, room_outside 0.6 %, terrain 2.5 %; every frame
# decides more than 96 % of its pixels.
SCENES = [("dragon", "dragon", 256, 144, 16700, 0.015), ("dragon", "dragon_inside", 101, 67, 6000, 0.015),
          ("monu9", "monu9", 256, 144, 9400, 0.015), ("nature", "nature", 256, 144, 16400, 0.015),
          ("room", "room_inside", 256, 144, 32400, 0.04), ("room", "room_outside", 256, 144, 13200, 0.01),
          ("terrain", "terrain", 240, 136, 1780, 0.03)]


@pytest.mark.parametrize("scene,pose,W,H,min_hits,cap", SCENES)
def test_oracle_full_mode_matches_path_reference(V, O, scenes, scene, pose, W, H, min_hits, cap):
    tex, dim = scenes[scene]
    c = Case(V, tex, dim, POSES[pose], W, H)
    f = trace(c, ref_world(scenes, scene))
    rgba, idd = c.oracle(O, 2)
    check(f, rgba, idd, min_hits, cap, f"{scene}/{pose} {W}x{H}")
    assert f.undecided_share() <= 0.04, f.undecided_share()                 # >= 96 % of all pixels decided


@pytest.mark.parametrize("scene,pose,W,H,min_hits", [("dragon", "dragon", 97, 55, 2450), ("room", "room_inside", 83, 49, 3580)])
def test_sample_indices(V, O, S, scenes, scene, pose, W, H, min_hits):
    """the oracle at initRNG sample k (tests/oracle_samples.c) against the reference at the same k; the colours must
    actually differ between samples"""
    tex, dim = scenes[scene]
    c = Case(V, tex, dim, POSES[pose], W, H)
    world = ref_world(scenes, scene)
    seen = set()
    for k in SAMPLES:
        f = trace(c, world, sample=k)
        rgba, idd = oracle_sample(S, O, c, k)
        check(f, rgba, idd, min_hits, 0.04, f"{scene} sample {k}")
        seen.add(rgba.tobytes())
    assert len(seen) == len(SAMPLES)


# ---- the edge worlds of test_shader_reference64, in mode 2 ----------------------------------------------------------------
# ~90 % of the decided hit pixels measured; undecided shares measured: highlight_glass 27 % (reflections off its glass
# voxel's faces seen from air, after approach steps too long for the landing to be decided: see path_ref64's error
# model), shadow_cap 3.7 %, materials 3.4 %, the rest <= 2.8 %
EDGE_MIN_HITS = {"origin_plus_x": 30, "shadow_cap": 3500, "zero_direction": 150, "negative_planes": 2900,
                 "negative_planes_far": 3700, "materials": 10900, "highlight_glass": 2100, "custom_bounds": 5500,
                 "scale_half": 3600, "scale_two": 3600}
EDGE_CAP = {"shadow_cap": 0.045, "highlight_glass": 0.29, "materials": 0.045}


@pytest.fixture(scope="module")
def edges(V):
    return edge_cases(V)


@pytest.mark.parametrize("name", sorted(EDGE_MIN_HITS))
def test_edge_worlds_in_full_mode(O, edges, name):
    c, _ = edges[name]
    f = trace(c, R.World(c.tex, c.dim, c.wmin, c.wmax))
    rgba, idd = c.oracle(O, 2)
    check(f, rgba, idd, EDGE_MIN_HITS[name], EDGE_CAP.get(name, 0.03), name)


# ---- glass edge worlds --------------------------------------------------------------------------------------------------
def _pixels(f, key, sel=None):
    m = f.dec_id & f.dec_dist & f.dec_rgb.all(1)
    return m & (f.stats[key] > 0) if sel is None else m & sel


def glass_cases(V):
    """name -> (Case, pin(frame), min decided hits)"""
    cases = {}
    # (a) ten parallel panes with distinct refraction bytes, head-on: every face pushes a reflected ray, the stack fills
    vox = []
    for i in range(10):
        vox += _slab(92, 109, 92, 109, 94 - 3 * i, 95 - 3 * i, c=0x80C0FF60, r=1.1 + 0.15 * i)
    vox += _slab(88, 113, 88, 113, 60, 61)
    tex, dim = _world(V, vox)
    def panes(f):
        assert _pixels(f, "dropped_refract", (f.stats["peak_stack"] == PR.MAX_RAYS) & (f.stats["dropped_refract"] > 0)).sum() > 100
    cases["panes"] = (Case(V, tex, dim, (100.5, 100.5, 96.5, -90.0, 0.0), 48, 32), panes, 130, 0.92)

    # (b) an eye in dense glass looking up at its top face: TIR at grazing incidence, exits where it is steep
    vox = _slab(76, 124, 92, 100, 76, 124, c=0x6080A040, r=2.5) + _slab(76, 124, 110, 111, 76, 124)
    tex, dim = _world(V, vox)
    def tir(f):
        assert _pixels(f, "tir").sum() > 200 and _pixels(f, "exit_glass").sum() > 200
    cases["grazing_exit"] = (Case(V, tex, dim, (100.5, 96.5, 100.5, -90.0, 35.0), 64, 48), tir, 2700, 0.01)

    # (c) a long tinted dense glass block in front of an opaque wall, at three voxel scales (the same grid view)
    vox = _slab(84, 116, 96, 108, 64, 98, c=0xC04020B0, r=1.5) + _slab(76, 124, 92, 116, 60, 61)
    tex, dim = _world(V, vox)
    for sc in (0.5, 1.0, 2.0):
        def absorb(f):
            assert _pixels(f, "hit_absorbed").sum() > 500
        eye = np.array([100.5, 102.5, 98.3]) / sc
        cases[f"block_scale_{sc}"] = (Case(V, tex, dim, (*eye, -90.0, -5.0), 48, 32, scale=sc), absorb, 1350, 0.01)

    # (d) a floor lit by an emissive ceiling it cannot see directly (behind the eye) and by sky through a gap
    vox = _slab(-16, 17, -1, 0, -16, 17) + _slab(-16, 17, 8, 9, 0, 17, c=0xFFE0A0FF, r=3.0, i=0.6)
    vox += _slab(-16, 17, 0, 8, 16, 17)
    tex, dim = _world(V, vox)
    def bounce(f):
        assert _pixels(f, "deep_emission").sum() > 100 and _pixels(f, "deep_sky").sum() > 100
        assert _pixels(f, "deep_ambient").sum() > 50
    cases["bounce_only"] = (Case(V, tex, dim, (0.5, 4.5, 6.5, -90.0, -70.0), 48, 32), bounce, 1350, 0.01)

    # (e) an eye in tinted glass that reaches the world's bounds: startIOF, the eye's medium, and reflected rays that leave
    # the world still in the medium (absorption on a miss)
    vox = _slab(0, 32, 0, 8, 0, 32, c=0x40A0C070, r=1.8) + _slab(4, 10, 12, 16, 4, 10)
    tex, dim = _world(V, vox, (0, 0, 0), (32, 32, 32))
    def eye_glass(f):
        assert _pixels(f, "hit_absorbed").sum() > 300 and _pixels(f, "miss_absorbed").sum() > 50
    cases["eye_in_glass"] = (Case(V, tex, dim, (16.5, 4.5, 16.5, -135.0, 40.0), 48, 32, wmin=(0, 0, 0), wmax=(32, 32, 32)),
                             eye_glass, 1350, 0.03)

    # (f) a pane between two opaque walls: the refracted ray (popped first) finds the far wall or the origin voxel's +X
    # face (ID 0, which leaves primaryVoxelID open for a later ray: the reflected one's wall behind the eye)
    vox = _slab(2, 3, -6, 7, -6, 7, c=0xA0C0E080, r=1.5) + [(0, 0, 0, OPAQUE, 3.0, 0.0)]
    vox += _slab(-3, -2, -8, 9, -8, 9, c=GREY) + _slab(11, 12, -12, 13, -12, 13, c=0x30A050FF)
    tex, dim = _world(V, vox)
    def order(f):
        dec = f.dec_id & f.dec_dist & f.dec_rgb.all(1)
        reentry = dec & (f.stats["id_zero_hit"] > 0) & (f.id != 0)               # an ID-0 hit, then the ID of a later ray
        assert reentry.sum() > 400 and np.array_equal(reentry, dec & (f.stats["id_reentry"] > 0))
        assert (dec & (f.stats["glass_hits"] > 0) & (f.stats["id_zero_hit"] == 0) & (f.id != 0)).sum() > 700
    cases["pane_order"] = (Case(V, tex, dim, (3.1, 0.5, 0.5, 180.0, 0.0), 48, 32), order, 1250, 0.05)
    return cases


@pytest.fixture(scope="module")
def glass(V, O):
    """name -> (Case, pin, min hits, undecided cap, oracle frame)"""
    return {k: (c, pin, mh, cap, c.oracle(O, 2)) for k, (c, pin, mh, cap) in glass_cases(V).items()}


@pytest.mark.parametrize("name", ["panes", "grazing_exit", "block_scale_0.5", "block_scale_1.0", "block_scale_2.0",
                                  "bounce_only", "eye_in_glass", "pane_order"])
def test_glass_edge_worlds(glass, name):
    c, pin, min_hits, cap, (rgba, idd) = glass[name]
    f = trace(c, R.World(c.tex, c.dim, c.wmin, c.wmax))
    check(f, rgba, idd, min_hits, cap, name)
    pin(f)


def test_exit_side_swap_never_runs(glass):
    """hitMarching's normal faces the ray, so comp:523's cosi > 0 never holds: n1 is the medium left on both sides of
    glass (shown by the exits counted in grazing_exit, whose n1 > n2 without any swap)"""
    c = glass["grazing_exit"][0]
    f = trace(c, R.World(c.tex, c.dim, c.wmin, c.wmax))
    assert (f.stats["exit_glass"] > 0).sum() > 200


# ---- the comparison can fail: one planted misreading of pathTrace at a time -------------------------------------------------
# "exit_swap" swaps n1 / n2 on leaving the denser medium (a reading of comp:522-526 as Snell's bookkeeping); the literal
# swap never runs (test_exit_side_swap_never_runs), so leaving it out could not be detected.
PATH_MUTATIONS = {"fifo": ["pane_order", "panes"], "exit_swap": ["grazing_exit"], "dim_no_scale": ["scale_half", "scale_two"],
                  "bounce_offset": ["materials", "bounce_only"], "no_pi_deep": ["bounce_only"], "rng_row": ["bounce_only"],
                  "no_miss_absorption": ["eye_in_glass"], "id_reflect_first": ["pane_order"], "id_zero_locks": ["pane_order"]}


@pytest.mark.parametrize("flaw", sorted(PATH_MUTATIONS))
def test_each_planted_path_flaw_is_detected(O, glass, edges, flaw):
    assert set(PATH_MUTATIONS) == set(PR.FLAWS)
    bad = 0
    for name in PATH_MUTATIONS[flaw]:
        if name in glass:
            c, rgba, idd = glass[name][0], *glass[name][4]
        else:
            c = edges[name][0]
            rgba, idd = c.oracle(O, 2)
        bad += R.compare(trace(c, R.World(c.tex, c.dim, c.wmin, c.wmax), flaws=(flaw,)), rgba, idd)["bad"]
    assert bad > 0, flaw
