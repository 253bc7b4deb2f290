"""The checkers of the jittered and thin-lens samples (tests/oracle_jitter.c, tests/oracle_lens.c) against the float64
restatement of those samples (tests/lens_ref64.py feeding tests/shader_ref64.py and tests/path_ref64.py).

The sequences are compared exactly, the checker's float32 rays against the float64 rays within the derived per-ray bounds
(the observed-over-bound ratios are printed and must not exceed 1), whole frames with the references' check() -- every
decided pixel equal in rgb, ID and dist, the undecided share capped, a minimum of decided hits -- and every planted
misreading of the header's two paragraphs must show."""
import numpy as np
import pytest

import lens_ref64 as LR
import oracle_jitter
import oracle_lens
import path_ref64 as PR
import shader_ref64 as R
from test_accum_lens import _focus_world
from test_path_reference64 import check, glass_cases
from test_shader_reference64 import POSES, Case, edge_cases, ref_world, scenes  # noqa: F401

EDGE_K = (2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1)
SOURCES = {"jitter": (True, False), "lens": (False, True), "jitter_lens": (True, True)}
KS = (1, 7, 2 ** 32 - 1)
CPU_K = {"jitter": 2 ** 32 - 1, "lens": 7, "jitter_lens": 1}        # the sample each source is traced at on the CPU
# include/vrt.h: the first eight points of each sequence
FIRST_JITTER = [(0, 0), (1 / 2, 1 / 2), (1 / 4, 3 / 4), (3 / 4, 1 / 4), (1 / 8, 5 / 8), (5 / 8, 1 / 8), (3 / 8, 3 / 8), (7 / 8, 7 / 8)]
FIRST_LENS = [(1 / 2, 1 / 2), (0, 0), (3 / 4, 1 / 4), (1 / 4, 3 / 4), (1 / 8, 5 / 8), (5 / 8, 1 / 8), (3 / 8, 3 / 8), (7 / 8, 7 / 8)]


@pytest.fixture(scope="module")
def LL(tmp_path_factory):
    return oracle_lens.build(tmp_path_factory.mktemp("oracle_lens_ref64"))


@pytest.fixture(scope="module")
def J(tmp_path_factory):
    return oracle_jitter.build(tmp_path_factory.mktemp("oracle_jitter_ref64"))


# ---- the cases ----------------------------------------------------------------------------------------------------------------
# name -> (scene or None, pose, W, H, aperture, focus, undecided cap of a jittered frame; a lens frame gets twice that)
# The lens of dragon and room_inside is tests/test_gpu_accum_lens.py's LENS, medium_per_lane and opaque_per_lane are its poses.
# POSES["dragon"] looks straight down -z from half-integer coordinates: the rays of a jittered sample run along grid planes
# and 2.6 % of its hit pixels are undecided at k = 7, 1.7 times the scene's cap; the view is turned by one degree and half a
# degree from the same eye (largest share / cap over the sources and KS: 0.58). room_inside keeps its eye and looks 3 degrees
# further right and 4 further down, where the lens samples stay within twice the room's cap (0.91; 1.01 at POSES's view).
CASES = {"dragon": ("dragon", POSES["dragon"][:3] + (-91.0, -10.5), 97, 55, 2.0, 60.0, 0.015),
         "room_inside": ("room", POSES["room_inside"][:3] + (35.0, -14.0), 83, 49, 0.75, 20.0, 0.04),
         "medium_per_lane": ("room", (31.5, 26.5, 31.5, 32.0, -10.0), 72, 45, 3.0, 12.0, 0.04),
         "opaque_per_lane": (None, (20.3, 15.2, 2.1, -90.0, -40.0), 72, 45, 3.0, 1.7, 0.03),
         "eye_in_glass": (None, None, 48, 32, 0.5, 8.0, 0.03),
         # the planted-flaw test only: medium_per_lane's eye (in the red glass) with a lens wide enough to leave it -- at
         # aperture 3 every origin still has the eye's medium; at 8 sample 7 starts in air, sample 1 in another solid
         "medium_edge": ("room", (31.5, 26.5, 31.5, 32.0, -10.0), 72, 45, 8.0, 12.0, 0.04),
         "zero_direction": (None, None, 64, 32, 0.0, 1.0, 0.05)}


class LCase:
    pass


_cases = {}


def lens_case(V, scenes, name):
    """-> LCase: .c (test_shader_reference64.Case), .world (the float64 reference's), .ap, .focus, .cap"""
    if name in _cases:
        return _cases[name]
    scene, pose, W, H, ap, focus, cap = CASES[name]
    lc = LCase()
    if scene is not None:
        tex, dim = scenes[scene]
        lc.c = Case(V, tex, dim, pose, W, H)
        lc.world = ref_world(scenes, scene)
    elif name == "opaque_per_lane":
        tex, dim = _focus_world(V)
        lc.c = Case(V, tex, dim, pose, W, H)
        lc.world = R.World(tex, dim)
    else:
        lc.c = edge_cases(V)[name][0] if name == "zero_direction" else glass_cases(V)[name][0]
        lc.world = R.World(lc.c.tex, lc.c.dim, lc.c.wmin, lc.c.wmax)
    lc.name, lc.ap, lc.focus, lc.cap = name, ap, focus, cap
    _cases[name] = lc
    return lc


def lens_of(lc, source):
    return (lc.ap, lc.focus) if SOURCES[source][1] else (0.0, 1.0)


def cap_of(lc, source):
    return lc.cap * (2 if SOURCES[source][1] else 1)


_refs = {}


def reference(lc, source, k, modes=(0, 1, 2), flaws=()):
    """the float64 sample: mode -> Frame, traced once per (case, source, sample) and kept"""
    key = (lc.name, source, k, tuple(flaws))
    have = _refs.setdefault(key, {})
    c = lc.c
    uni = dict(voxel_scale=c.scale, global_light=c.gl, light_dir=c.light, highlighted=c.hl)
    if any(m not in have for m in modes):
        ap, focus = lens_of(lc, source)
        ry = LR.lens_rays(*c.cam, c.W, c.H, sample=k, jitter=SOURCES[source][0], aperture=ap, focus=focus, flaws=flaws)
        if any(m in modes and m not in have for m in (0, 1)):
            tr = R.Trace.lens(lc.world, ry, **uni)
            have[0], have[1], have["trace"] = tr.frame(0), tr.frame(1), tr
        if 2 in modes and 2 not in have:
            have["path"] = PR.PathTrace.lens(lc.world, ry, **uni)
            have[2] = have["path"].frame()
    return have


def radiance(lc, source, k, mode):
    """-> (h(c), bound, decided) of the sample's unclamped colour"""
    have = reference(lc, source, k, (mode,))
    return have["path"].radiance() if mode == 2 else have["trace"].radiance(mode)


def pinhole(lc, modes=(0, 1, 2)):
    """the unjittered pinhole frame (point 6's id_dist), from the existing frame constructors"""
    have = _refs.setdefault((lc.name, "frame"), {})
    c = lc.c
    uni = dict(voxel_scale=c.scale, global_light=c.gl, light_dir=c.light, highlighted=c.hl)
    if any(m in modes and m not in have for m in (0, 1)):
        tr = R.Trace(lc.world, *c.cam, c.W, c.H, **uni)
        have[0], have[1] = tr.frame(0), tr.frame(1)
    if 2 in modes and 2 not in have:
        have[2] = PR.PathTrace(lc.world, *c.cam, c.W, c.H, **uni).frame()
    return have


def checker_scene(O, c):
    s = O.make_scene(c.tex, c.dim, *c.cam, highlighted=c.hl)
    s.voxel_scale = c.scale
    s.bounds_min[:], s.bounds_max[:] = list(c.wmin), list(c.wmax)
    s.global_light[:] = [float(v) for v in c.gl]
    s.light_dir[:] = [float(v) for v in c.light]
    return s


def checker(LL, J, s, lc, source, k, mode):
    jitter, lens = SOURCES[source]
    if lens:
        return oracle_lens.render(LL, s, lc.c.W, lc.c.H, mode, k, lc.ap, lc.focus, jitter=jitter)
    return oracle_jitter.render(J, s, lc.c.W, lc.c.H, mode, k, jitter=True)


# ---- the sequences ------------------------------------------------------------------------------------------------------------
def test_sequences_are_the_headers_and_the_checkers(LL, J):
    for k in range(8):
        assert (LR.jx(k), LR.jy(k)) == FIRST_JITTER[k] and (LR.lu(k), LR.lv(k)) == FIRST_LENS[k], k
    worst = 0.0
    for k in list(range(4096)) + list(EDGE_K):
        u, v = oracle_lens.uv(LL, k)
        assert (float(u), float(v)) == (LR.lu(k), LR.lv(k)), k
        a, b = oracle_jitter.offsets(J, k)
        assert (float(a), float(b)) == (LR.jx(k), LR.jy(k)), k
        x, y = oracle_lens.point(LL, k)
        lx, ly, ex, ey, centre = LR.disc(k)
        if centre:
            assert k == 0 and x == 0 and y == 0
            continue
        worst = max(worst, abs(float(x) - lx) / ex, abs(float(y) - ly) / ey)
    print(f"lens point: largest float32 error over its bound {worst:.3f}")
    assert worst <= 1.0, worst
    assert worst == pytest.approx(LR.MEASURED_RATIOS["disc"], abs=0.01)


def test_jittered_positions_at_the_last_sample():
    """k = 2^32 - 1: jx = 1 - 2^-24; exact at px = 0, the float32 tie at px = 1 goes to the even 2, px + 1 from px = 2 on"""
    assert LR.jx(2 ** 32 - 1) == 1 - 2.0 ** -24
    fx, _ = LR.pixel_positions(np.arange(5), np.zeros(5, int), 2 ** 32 - 1, True)
    assert fx.tolist() == [1 - 2.0 ** -24, 2.0, 3.0, 4.0, 5.0]
    ex, _ = LR.pixel_positions(np.arange(5), np.zeros(5, int), 2 ** 32 - 1, True, flaws=("jitter_exact_add",))
    assert np.all(ex[1:] < fx[1:])
    fx, fy = LR.pixel_positions(np.array([1919]), np.array([1079]), 5, True)          # 11 bits of jx are dropped at px = 1919
    assert fx[0] == float(np.float32(1919) + np.float32(0.625)) and fy[0] == 1079.125


# ---- the rays -------------------------------------------------------------------------------------------------------------------
RAY_SCENES = {"dragon": ("dragon", POSES["dragon"], 2.0, 60.0), "room_inside": ("room", POSES["room_inside"], 0.75, 20.0),
              "terrain": ("terrain", POSES["terrain"], 6.0, 400.0)}


def ray_ratios(LL, s, cam, W, H, ap, focus, k, jitter):
    """largest observed float32 error over its bound -> (origin, moved direction, pinhole direction)"""
    ry = LR.lens_rays(*cam, W, H, sample=k, jitter=jitter, aperture=ap, focus=focus)
    ro = rd = rp = 0.0
    for i in range(W * H):
        moved, o, d = oracle_lens.ray(LL, s, W, H, int(ry.xs[i]), int(ry.ys[i]), k, ap, focus, jitter=jitter)
        if ry.amb[i]:
            continue
        assert moved == ry.moved[i], (k, i)
        eo = np.abs(o.astype(np.float64) - ry.o[i])
        ed = np.abs(d.astype(np.float64) - ry.d[i]).max() / ry.dir_bound[i]
        if moved:
            ro, rd = max(ro, (eo / ry.err_o[i]).max()), max(rd, ed)
        else:
            assert eo.max() == 0.0
            rp = max(rp, ed)
    return ro, rd, rp


@pytest.mark.parametrize("name", sorted(RAY_SCENES))
def test_checker_rays_lie_within_the_derived_bounds(LL, O, V, scenes, name):
    """every pixel of a 32x24 frame, k in (1, 2, 7, 255, 2^32 - 1), with and without jitter, lens on and off (the pinhole
    ray's ~6u): the ratios are printed; the largest are recorded in lens_ref64.MEASURED_RATIOS"""
    scene, pose, ap, focus = RAY_SCENES[name]
    tex, dim = scenes[scene]
    W, H = 32, 24
    c = Case(V, tex, dim, pose, W, H)
    s = checker_scene(O, c)
    worst = np.zeros(3)
    for k in (1, 2, 7, 255, 2 ** 32 - 1):
        for jitter in (False, True):
            worst = np.maximum(worst, ray_ratios(LL, s, c.cam, W, H, ap, focus, k, jitter))
            worst = np.maximum(worst, ray_ratios(LL, s, c.cam, W, H, 0.0, 1.0, k, jitter))
    print(f"{name}: largest float32 error over its bound: origin {worst[0]:.3f} direction {worst[1]:.3f} pinhole direction {worst[2]:.3f}")
    assert np.all(worst <= 1.0), worst
    m = LR.MEASURED_RATIOS
    assert np.all(worst <= np.array([m["origin"], m["direction"], m["pinhole_direction"]]) + 0.01), worst


# ---- whole frames ---------------------------------------------------------------------------------------------------------------
# MIN_HITS[case][source] = (modes 0 and 1, mode 2): 0.9 of the fewest decided hit pixels the reference gives against the
# checkers over k in KS (measured, in the comment: fewest decided hits modes 0/1, mode 2; largest undecided share / cap).
MIN_HITS = {
    "dragon": {
        "jitter": (2451, 2453),   # measured 2724, 2726; undecided share 0.0069 of 0.015
        "jitter_lens": (2441, 2448),   # measured 2713, 2720; undecided share 0.0175 of 0.03
        "lens": (2432, 2438),   # measured 2703, 2709; undecided share 0.0175 of 0.03
    },
    "room_inside": {
        "jitter": (3655, 3571),   # measured 4062, 3968; undecided share 0.0332 of 0.04
        "jitter_lens": (3647, 3497),   # measured 4053, 3886; undecided share 0.0698 of 0.08
        "lens": (3647, 3492),   # measured 4053, 3881; undecided share 0.073 of 0.08
    },
    "medium_per_lane": {
        "jitter": (2915, 2861),   # measured 3239, 3179; undecided share 0.021 of 0.04
        "jitter_lens": (2915, 2754),   # measured 3239, 3060; undecided share 0.0617 of 0.08
        "lens": (2915, 2755),   # measured 3239, 3062; undecided share 0.0593 of 0.08
    },
    "opaque_per_lane": {
        "jitter": (2875, 2874),   # measured 3195, 3194; undecided share 0.0075 of 0.03
        "jitter_lens": (2332, 2329),   # measured 2592, 2588; undecided share 0.0015 of 0.06
        "lens": (2268, 2266),   # measured 2520, 2518; undecided share 0.0009 of 0.06
    },
    "eye_in_glass": {
        "jitter": (1353, 1353),   # measured 1504, 1504; undecided share 0.0208 of 0.03
        "jitter_lens": (1382, 1382),   # measured 1536, 1536; undecided share 0.0007 of 0.06
        "lens": (1382, 1381),   # measured 1536, 1535; undecided share 0.0007 of 0.06
    },
}
FRAME_CASES = ["dragon", "room_inside", "medium_per_lane", "opaque_per_lane", "eye_in_glass"]


def check_sample(f, pin, rgba, idd, min_hits, cap, what):
    """check()'s three conditions for a resolved accumulation sample: every decided pixel equal in rgb (the sample's) and in
    ID and dist (the unjittered pinhole frame's, point 6); the sample's own decided hits and undecided share"""
    r = R.compare(LR.with_frame_ids(f, pin), rgba, idd)
    assert r["bad"] == 0, (what, r)
    hits = int((f.hit & f.dec_id & f.dec_dist).sum())
    assert hits >= min_hits, (what, hits)
    assert f.hit_undecided_share() <= cap, (what, f.hit_undecided_share())
    return r


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("name", FRAME_CASES)
def test_checker_frames_match_the_float64_samples(LL, J, O, V, scenes, name, source):
    """modes 0, 1 and 2 at the source's sample CPU_K: the checker's own frame of the sample (its rgb, and the ID and dist of
    the sample's ray) with the references' check(), then its rgb beside the unjittered frame's id_dist (point 6)"""
    lc = lens_case(V, scenes, name)
    s = checker_scene(O, lc.c)
    k = CPU_K[source]
    fr, pin = reference(lc, source, k), pinhole(lc)
    for mode in (0, 1, 2):
        rgba, idd = checker(LL, J, s, lc, source, k, mode)
        what = f"{name} {source} sample {k} mode {mode}"
        r = check(fr[mode], rgba, idd, MIN_HITS[name][source][mode // 2], cap_of(lc, source), what)
        print(what, "decided hits", r["decided_hits"], "undecided share", round(r["undecided_share"], 4))
        _, idd0 = oracle_jitter.render(J, s, lc.c.W, lc.c.H, mode, 0, jitter=False)
        check_sample(fr[mode], pin[mode], rgba, idd0, MIN_HITS[name][source][mode // 2], cap_of(lc, source), what + " + frame id_dist")


# ---- the comparison can fail: one planted misreading of the header at a time -------------------------------------------------------
# flaw -> (case, source, sample, modes). k = 7 uses direction numbers 0..2 only, which no polynomial enters: 255 for the swap;
# (jx, jy)(1) and (7) are symmetric: 2 for the axes.
LENS_MUTATIONS = {"jitter_axes_swapped": ("dragon", "jitter", 2, (0, 1)), "jitter_pixel_centre": ("dragon", "jitter", 2 ** 32 - 1, (0, 1)),
                  "lens_no_shift": ("dragon", "lens", 7, (0, 1)), "lens_polys_swapped": ("dragon", "lens", 255, (0, 1)),
                  "lens_square": ("dragon", "lens", 7, (0, 1)), "lens_focus_along_ray": ("dragon", "lens", 7, (0, 1)),
                  "lens_origin_only": ("dragon", "lens", 7, (0, 1)), "lens_medium_at_eye": ("medium_edge", "lens", 7, (0, 1, 2)),
                  "lens_dim_from_eye": ("medium_per_lane", "lens", 7, (0, 1, 2)), "lens_rng_sample0": ("dragon", "lens", 7, (2,))}


@pytest.mark.parametrize("flaw", sorted(LENS_MUTATIONS))
def test_each_planted_lens_flaw_is_detected(LL, J, O, V, scenes, flaw):
    assert set(LENS_MUTATIONS) | {"jitter_exact_add"} == set(LR.LENS_FLAWS)
    name, source, k, modes = LENS_MUTATIONS[flaw]
    lc = lens_case(V, scenes, name)
    s = checker_scene(O, lc.c)
    good, flawed = reference(lc, source, k, modes), reference(lc, source, k, modes, flaws=(flaw,))
    bad = 0
    for mode in modes:
        rgba, idd = checker(LL, J, s, lc, source, k, mode)
        assert R.compare(good[mode], rgba, idd)["bad"] == 0
        bad += R.compare(flawed[mode], rgba, idd)["bad"]
    assert bad > 0, flaw


def test_exact_add_flaw_at_the_last_sample(J, O, V, scenes):
    """jitter_exact_add moves a position by less than 2^-18 pixel at these widths -- below the frame's own ~6u direction
    error, so no decided pixel of any frame can differ, by the error model's construction. It shows where the float32 sum
    is structurally exact: the identity camera of zero_direction at k = 2^32 - 1, where column W/2 - 1 lands on
    px + 1 = W/2, u == 0 and d.x == 0 exactly. The reference decides that column (an exactly-zero component never hits:
    sky) and agrees with the checker; with the addition done in float64 d.x is ~ -2e-9, which no float32 model can decide."""
    lc = lens_case(V, scenes, "zero_direction")
    k = 2 ** 32 - 1
    f = reference(lc, "jitter", k, (0, 1))[0]
    rgba, idd = checker(None, J, checker_scene(O, lc.c), lc, "jitter", k, 0)
    r = R.compare(f, rgba, idd)
    col = f.xs == lc.c.W // 2 - 1
    assert r["bad"] == 0 and f.dec_id[col].all() and (f.kind[col] == R.KIND_SKY).all() and r["decided_hits"] > 100, r
    g = reference(lc, "jitter", k, (0, 1), flaws=("jitter_exact_add",))[0]
    assert not g.dec_id[col].any()
