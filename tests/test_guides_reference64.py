"""The guide planes' checkers (tests/oracle_guides.c, tests/oracle_guides_glass.c) against the independent float64 restatement
(tests/guide_ref64.py), plain and past glass: frames over the four ray sources, means of three samples, the ray mixes of
tests/test_rays_reference64.py, a fourth materials batch at voxel scale 3, and hand-built worlds (tests/glass_worlds.py) that reach
the endings no other input reaches in decided rays. Decided rays are exact in hit, normal, RGB, A0 and S, the class of the ending
and (where the cell's own rule decides it) the final cell; the depth lies within the reference's derived bound. Every planted
misreading of the reference, and each of the checker's four plants, is caught on a named input.

What a comparison leaves out is capped as tests/test_rays_reference64.py caps it: the share measured on the reference alone plus a
quarter of itself, rounded up to the next 0.005, never above 0.15; once over the in-world rays and once over the rays whose
segment-0 hit is decided and translucent. tests/test_gpu_guides_reference64.py compares the device with the same references."""
import math

import numpy as np
import pytest

import glass_worlds as GL
import guide_ref64 as GR
import guide_worlds as GW
import oracle_guides as G
import oracle_guides_glass as GG
import shader_ref64 as R
from test_gpu_shade_rays import _materials_world, _ray_mix
from test_rays_reference64 import MATERIALS_MIX, MIX_CAPS, N_MIX, Batch, batch
from test_shader_reference64 import scenes  # noqa: F401

F = np.float32
SIZES = ((GW.W, GW.H), GW.RAGGED)
SAMPLES = (5, 12)
MEAN_FIRST, MEAN_N = 5, 3
MIN_THROUGH = 100           # decided through-glass rays every glass input keeps

# ---- the inputs --------------------------------------------------------------------------------------------------------------------
# Frames. name: (cap over all pixels, cap over through-glass pixels, the same two for the means of 3, glass input)
#                                                            measured: the worst of 2 sizes x 4 sources x samples 5, 12 | means of 3
FRAME_CAPS = {
    "room":      (0.005, 0.010, 0.020, 0.025, True),        # 0.33 % / 0.48 %  |  1.33 % / 1.81 %
    "lamp":      (0.010, 0.010, 0.015, 0.015, True),        # 0.63 % / 0.65 %  |  1.15 % / 1.18 %
    "outside":   (0.010, 0.060, 0.010, 0.050, False),       # 0.44 % / 4.76 %  |  0.73 % / 3.85 % (20 to 42 through-glass pixels: the floor
                                                            #                     of 100 cannot hold; the room's glass is in the frames beside it)
    "room_wall": (0.035, 0.010, 0.045, 0.045, True),        # 2.66 % / 0.55 %  |  3.21 % / 3.21 %
    "panes_30":  (0.080, 0.080, 0.110, 0.110, True),        # 6.04 % / 6.04 %  |  8.54 % / 8.54 % (the lens sources: eight surfaces per ray)
}
# Ray batches, the worst of the setting on, off, and on with the highlighted voxel.
# name: (cap over the in-world rays, cap over the through-glass rays, glass input)                               measured
BATCH_CAPS = {
    "dragon_mix":    (0.010, 0.005, False),                  # 0.69 % / no through-glass ray
    "room_mix":      (0.010, 0.055, False),                  # 0.41 % / 4.17 % (69 decided through-glass rays of 2,800: below the floor
                                                             #                  of 100; the room and room_wall frames hold that glass)
    "materials_1":   (0.015, 0.070, True),                   # 1.20 % / 5.60 %
    "materials_0.5": (0.015, 0.070, True),                   # 1.20 % / 5.60 %
    "materials_2":   (0.015, 0.070, True),                   # 1.20 % / 5.60 %
    "scale_3":       (0.015, 0.070, True),                   # 1.20 % / 5.60 %
    "bounds_mix":    (0.055, 0.060, True),                   # 4.40 % / 4.78 %
    "near_index":    (0.005, 0.005, False),                  # 0 / 0 (80 rays: floors of 20 per kind instead of the 100)
    "alpha0":        (0.005, 0.005, False),                  # 0 / 0 (80 rays)
    "grazing":       (0.065, 0.005, False),                  # 5.00 % / 0 (60 rays; the three left out land within the floor margin)
}
HAND_BUILT = ("near_index", "alpha0", "grazing")
ALL_BATCHES = sorted(BATCH_CAPS)
RATIOS = GR.MEASURED_RATIOS     # the largest depth error over its bound per input: asserted <= 1, and no larger than recorded there


def cap_rule(measured):
    """the share measured on the reference alone plus a quarter of itself, rounded up to the next 0.005"""
    return max(0.005, math.ceil(measured * 1.25 / 0.005 - 1e-9) * 0.005)


# the measured shares of the comments above as numbers: the caps are the rule applied to them, and nothing else
FRAME_MEASURED = {"room": (0.0033, 0.0048, 0.0133, 0.0181), "lamp": (0.0063, 0.0065, 0.0115, 0.0118), "outside": (0.0044, 0.0476, 0.0073, 0.0385),
                  "room_wall": (0.0266, 0.0055, 0.0321, 0.0321), "panes_30": (0.0604, 0.0604, 0.0854, 0.0854)}
BATCH_MEASURED = {"dragon_mix": (0.0069, 0.0), "room_mix": (0.0041, 0.0417), "materials_1": (0.0120, 0.0560), "materials_0.5": (0.0120, 0.0560),
                  "materials_2": (0.0120, 0.0560), "scale_3": (0.0120, 0.0560), "bounds_mix": (0.0440, 0.0478), "near_index": (0.0, 0.0),
                  "alpha0": (0.0, 0.0), "grazing": (0.0500, 0.0)}


def test_every_cap_is_the_rule_applied_to_its_measured_share():
    for caps, measured in ((FRAME_CAPS, FRAME_MEASURED), (BATCH_CAPS, BATCH_MEASURED)):
        assert set(caps) == set(measured)
        for name, m in measured.items():
            for cap, share in zip(caps[name], m):
                assert abs(cap - cap_rule(share)) < 1e-9 and cap <= 0.15, (name, cap, share)


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return GG.build(tmp_path_factory.mktemp("oracle_guides_ref64"))


_cache = {}


def frame_input(V, name):
    """-> (texels, tex_dim, reference world, pose, (aperture, focus)), built once"""
    key = ("frame", name)
    if key not in _cache:
        if name == "panes_30":
            tex, dim = GL.build(V, GL.ten_panes(*GL.PANES_WIDE))
            pose, lens = GL.PANES_POSE, GL.PANES_LENS
        else:
            w = GW.world(V, "room" if name == "room_wall" else name)
            tex, dim = w.flatten()
            w.close()
            pose, lens = (GL.ROOM_THROUGH_WALL, GW.FRAMES["room"][1]) if name == "room_wall" else GW.FRAMES[name]
        _cache[key] = (tex, dim, R.World(tex, dim), pose, lens)
    return _cache[key]


def frame_camera(V, name, size):
    pose = frame_input(V, name)[3]
    return V.camera_block(pose[:3], pose[3], pose[4], size[0], size[1])[:3]


def lens_of(V, name, source):
    return frame_input(V, name)[4] if GW.SOURCES[source][1] else (0.0, 1.0)


def frame_trace(V, name, size, source, k, glass=True, flaws=()):
    """the reference's guide of sample k, traced once (a corner sample does not depend on k)"""
    jitter, lens = GW.SOURCES[source]
    key = ("trace", name, size, source, k if (jitter or lens) else 0, glass, tuple(flaws))
    if key not in _cache:
        ap, fo = lens_of(V, name, source)
        _cache[key] = GR.GuideTrace.sample(frame_input(V, name)[2], *frame_camera(V, name, size), size[0], size[1], k, jitter, ap, fo,
                                           glass=glass, flaws=flaws)
    return _cache[key]


def frame_scene(V, O, name, size):
    key = ("scene", name, size)
    if key not in _cache:
        tex, dim = frame_input(V, name)[:2]
        _cache[key] = O.make_scene(tex, dim, *frame_camera(V, name, size))
    return _cache[key]


def ray_batch(name, V, O, scenes):
    """-> test_rays_reference64.Batch: the six mixes as that module builds them, the materials mix at voxel scale 3, and the
    hand-built worlds with their rays"""
    key = ("batch", name)
    if key in _cache:
        return _cache[key]
    if name in MIX_CAPS:
        b = batch(name, V, O, None, scenes)
    elif name == "scale_3":
        w = _materials_world(V)
        tex, dim = w.flatten()
        w.close()
        o, d = _ray_mix(np.random.default_rng(53), N_MIX["materials_1"], *MATERIALS_MIX)
        b = Batch(tex, dim, o / F(3.0), d, 64, scale=3.0)
    else:
        voxels, rays = {"near_index": (GL.near_index, GL.near_index_rays), "alpha0": (GL.alpha0_beside_glass, GL.alpha0_rays),
                        "grazing": (GL.grazing_pane, GL.grazing_rays)}[name]
        o, d, kind = rays()
        b = Batch(*GL.build(V, voxels()), np.broadcast_to(o, d.shape), d, 7)
        b.kind = kind
    _cache[key] = b
    return b


def batch_trace(b, glass=True, highlighted=(-1, -1, -1), flaws=()):
    key = ("guide", glass, tuple(highlighted), tuple(flaws))
    if key not in b._traces:
        b._traces[key] = GR.GuideTrace.rays(b.world, b.o, b.d, voxel_scale=b.scale, highlighted=highlighted, glass=glass, flaws=flaws)
    return b._traces[key]


def batch_scene(b, O, V, highlighted=(-1, -1, -1)):
    s = b.scene(O, V)
    s.highlighted[:] = [int(v) for v in highlighted]
    return s


def most_frequent_cell_behind_glass(t):
    """the most frequent final cell of the decided rays that ended on an opaque surface behind glass, its own floor decided"""
    sel = t.decided & t.through & (t.end == GR.OPAQUE) & (t.S >= 2) & ~t.cell_near
    if not sel.any():
        return None
    cells, counts = np.unique(t.cell[sel], axis=0, return_counts=True)
    return tuple(int(v) for v in cells[np.argmax(counts)])


# ---- the comparisons ---------------------------------------------------------------------------------------------------------------
def ending_class(final_alpha, surfaces, hit):
    """what the checker's plant="alpha_of_final" tells of how a chain ended: the final surface's own alpha is 255 exactly on an
    opaque ending; below 255 the chain stopped for G4 where S == 8, for G5 (TIR or a share) where S < 8 -> 0 miss, 1 opaque, 2 cap,
    3 a G5 stop"""
    return np.where(hit == 0, 0, np.where(final_alpha == 255, 1, np.where(surfaces == GR.MAX_SURFACES, 2, 3)))


REF_CLASS = np.array([0, 1, 2, 3, 3, 3, 1])     # of guide_ref64.ENDINGS; "first" (the plain guide) is compared through its alpha


def mismatches(t, g, final=None):
    """the reference's sample t against a checker's Guide g (and its alpha_of_final twin) -> {field: bool[n] of decided rays that
    differ}, the depth's err / bound"""
    dec = t.decided
    hit = g.hit.ravel() != 0
    both = dec & hit & t.hit
    out = {"hit": dec & (hit != t.hit)}
    out["normal"] = both & (g.normal.reshape(-1, 3).astype(np.int64) != t.normal).any(1)
    out["albedo"] = both & (g.albedo.reshape(-1, 4).astype(np.int64) != t.bytes4()).any(1)
    out["cell"] = both & ~t.cell_near & (g.cell.reshape(-1, 3).astype(np.int64) != t.cell).any(1)
    if hasattr(g, "surfaces"):
        out["S"] = dec & (g.surfaces.ravel() != t.S)
    if final is not None:
        cls = ending_class(final.albedo.reshape(-1, 4)[:, 3], g.surfaces.ravel(), g.hit.ravel())
        want = np.where(t.hit, np.where((t.end == GR.FIRST) & (t.a_final < 255), 3, REF_CLASS[t.end]), 0)
        out["ending"] = dec & (cls != want)
    depth, bound = t.depth()
    err = np.abs(g.depth.ravel().astype(np.float64) - depth)
    out["depth"] = both & (err > bound)
    ratio = float((err[both] / bound[both]).max()) if both.any() else 0.0
    return out, ratio


def check_sample(t, g, final, what, caps, min_through=0, ratio_cap=None):
    """every decided ray exact, the depth within its bound, both left-out shares under their caps; prints the input's line"""
    bad, ratio = mismatches(t, g, final)
    a, b = t.left_out()
    n_through = int((t.through & t.decided).sum())
    print(f"{what}: in-world {int((~t.outside).sum())} decided {int(t.decided.sum())} through glass {n_through} left out {a:.4f} (cap {caps[0]}) "
          f"/ {b:.4f} (cap {caps[1]}) endings {t.endings()} depth err / bound {ratio:.3f}")
    for f, m in bad.items():
        assert not m.any(), (what, f, int(m.sum()), int(np.nonzero(m)[0][0]))
    assert not (t.outside & t.hit).any()
    assert caps[0] <= 0.15 and caps[1] <= 0.15 and a <= caps[0] and b <= caps[1], (what, a, b, caps)
    assert n_through >= min_through, (what, n_through)
    assert ratio <= 1.0 and (ratio_cap is None or ratio <= ratio_cap + 5e-4), (what, ratio)
    return ratio


def check_planes(want, got, what, coverage=True):
    """a resolve of the reference (guide_ref64.resolve, or GuideTrace.planes for a batch) against planes of the checker or the
    device: exact bits of normal, albedo and coverage (or the hit bytes) on decided pixels, the depth within its bound"""
    dec = want["decided"]
    n = dec.size
    for k, c in (("normal", 3), ("albedo", 4)):
        a, b = np.asarray(got[k], F).reshape(n, c), want[k].reshape(n, c)
        bad = dec & (a.view(np.uint32) != b.view(np.uint32)).any(1)
        assert not bad.any(), (what, k, int(bad.sum()), int(np.nonzero(bad)[0][0]), a[bad][0], b[bad][0])
    if coverage:
        a = np.asarray(got["coverage"], F).ravel()
        assert np.array_equal(a[dec].view(np.uint32), want["coverage"][dec].view(np.uint32)), (what, "coverage")
    else:
        assert np.array_equal(np.asarray(got["hit"]).ravel()[dec] != 0, want["hit"][dec]), (what, "hit")
    d = np.asarray(got["depth"], np.float64).ravel()
    assert np.isfinite(d[dec]).all(), what
    err = np.abs(d - want["depth"])
    bad = dec & (err > want["depth_bound"])
    assert not bad.any(), (what, "depth", int(bad.sum()), int(np.nonzero(bad)[0][0]), float(err[bad][0]), float(want["depth_bound"][bad][0]))
    pos = dec & (want["depth_bound"] > 0)
    return float((err[pos] / want["depth_bound"][pos]).max()) if pos.any() else 0.0


def left_out_of_mean(samples):
    """-> the two left-out shares of a mean: a pixel is left out when any of its samples is undecided"""
    amb = np.any([s.amb for s in samples], axis=0)
    through = np.all([s.through | ~s.first_translucent for s in samples], axis=0) & np.any([s.through for s in samples], axis=0)
    return float(amb.mean()), float(amb[through].mean()) if through.any() else 0.0


# ---- frames ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=["40x24", "43x21"])
@pytest.mark.parametrize("name", sorted(FRAME_CAPS))
def test_frames_match_the_reference_sample_by_sample(V, O, L, name, size):
    """all four sources at samples 5 and 12: the past-glass checker against the reference, and the plain checker against the
    reference stopped after one surface"""
    scene = frame_scene(V, O, name, size)
    caps = FRAME_CAPS[name]
    worst = 0.0
    for source, (jitter, _) in GW.SOURCES.items():
        ap, fo = lens_of(V, name, source)
        for k in SAMPLES:
            what = f"{name} {size[0]} x {size[1]} {source} sample {k}"
            t = frame_trace(V, name, size, source, k)
            g = GG.sample(L, scene, size[0], size[1], k, jitter, ap, fo)
            final = GG.sample(L, scene, size[0], size[1], k, jitter, ap, fo, plant="alpha_of_final")
            worst = max(worst, check_sample(t, g, final, what, caps, MIN_THROUGH if caps[4] else 0, RATIOS[name]))
            if k == SAMPLES[0]:
                plain = frame_trace(V, name, size, source, k, glass=False)
                check_sample(plain, G.sample(L, scene, size[0], size[1], k, jitter, ap, fo), None, what + " plain", caps)
    print(f"{name} {size}: worst depth err / bound {worst:.3f} (recorded {RATIOS[name]})")


@pytest.mark.parametrize("name", sorted(FRAME_CAPS))
def test_means_of_three_samples(V, O, L, name):
    """samples 5 to 7 through the header's resolve: exact bits of normal, albedo and coverage where all three are decided, the depth
    within the mean of the samples' bounds plus one float32 rounding"""
    caps = FRAME_CAPS[name]
    for size in SIZES:
        scene = frame_scene(V, O, name, size)
        for source, (jitter, _) in GW.SOURCES.items():
            ap, fo = lens_of(V, name, source)
            samples = [frame_trace(V, name, size, source, k) for k in range(MEAN_FIRST, MEAN_FIRST + MEAN_N)]
            want = GR.resolve(samples)
            got = GG.planes(L, scene, size[0], size[1], MEAN_FIRST, MEAN_N, jitter, ap, fo)[0]
            a, b = left_out_of_mean(samples)
            ratio = check_planes(want, got, f"{name} {size} {source} mean of {MEAN_N}")
            print(f"{name} {size} {source} mean of {MEAN_N}: decided {int(want['decided'].sum())} left out {a:.4f} (cap {caps[2]}) / {b:.4f} "
                  f"(cap {caps[3]}) depth err / bound {ratio:.3f}")
            assert caps[2] <= 0.15 and caps[3] <= 0.15 and a <= caps[2] and b <= caps[3], (name, size, source, a, b)


# ---- ray batches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_BATCHES)
def test_ray_batches_match_the_reference(V, O, L, scenes, name):
    """the setting on and off, and on with a highlighted voxel: the most frequent decided final cell behind glass"""
    b = ray_batch(name, V, O, scenes)
    caps = BATCH_CAPS[name]
    s = batch_scene(b, O, V)
    t = batch_trace(b)
    check_sample(t, GG.rays(L, s, b.o, b.d), GG.rays(L, s, b.o, b.d, plant="alpha_of_final"), name, caps, MIN_THROUGH if caps[2] else 0,
                 RATIOS[name])
    check_sample(batch_trace(b, glass=False), G.rays(L, s, b.o, b.d), None, name + " plain", caps)
    hl = most_frequent_cell_behind_glass(t)
    if caps[2] or name in HAND_BUILT:
        assert hl is not None, name
    if hl is not None:
        th = batch_trace(b, highlighted=hl)
        sh = batch_scene(b, O, V, hl)
        marked = th.decided & th.hit & np.all(th.cell == np.array(hl), 1)
        assert marked.sum() >= 1 and (th.bytes4()[marked, :3] != t.bytes4()[marked, :3]).any(), (name, hl)
        # the inversion takes alpha 255: behind glass A stays A0, and a marked pane ends its chain as an opaque surface would
        check_sample(th, GG.rays(L, sh, b.o, b.d), GG.rays(L, sh, b.o, b.d, plant="alpha_of_final"), f"{name} highlighted {hl}",
                     caps)


def test_the_new_inputs_reach_their_rules_in_decided_rays(V, O, scenes):
    """asserted on the reference alone: every ending kind but one has an input whose decided rays reach it (the cap through a frame
    too), the voxel scale 3 rounds its divisions, and both alpha-0 branches of G5 are met"""
    b = ray_batch("near_index", V, O, scenes)
    assert GL.NEAR_BYTE in set(b.world.p[b.world.a > 0, 0].tolist())
    t = batch_trace(b)
    near, steep = t.decided & ~b.kind, t.decided & b.kind
    assert ((t.end == GR.REFLECT) & (t.S == 1))[near].all() and near.sum() >= 20, t.endings(~b.kind)
    assert ((t.end == GR.OPAQUE) & (t.S == 3))[steep].all() and steep.sum() >= 20, t.endings(b.kind)
    b = ray_batch("grazing", V, O, scenes)
    t = batch_trace(b)
    below, above = t.decided & b.kind, t.decided & ~b.kind
    assert ((t.end == GR.REFRACT) & (t.S == 1))[below].all() and below.sum() >= 20, t.endings(b.kind)
    assert ((t.end == GR.OPAQUE) & (t.S == 2))[above].all() and above.sum() >= 20, t.endings(~b.kind)
    b = ray_batch("alpha0", V, O, scenes)
    t = batch_trace(b)
    w = b.world
    assert (w.a == 0)[w.isleaf & (w.p[:, 0] == int(GL.PHANTOM_REFR / 3.0 * 255))].any()       # alpha-0 leaves that store 2.0
    eye, inside = t.decided & ~b.kind, t.decided & b.kind
    assert ((t.end == GR.OPAQUE) & (t.S == 3))[eye].all() and eye.sum() >= 20          # previous voxel alpha 0, then hit leaf alpha 0
    assert (t.end == GR.OPAQUE)[inside].all() and (t.S[inside] >= 3).all() and inside.sum() >= 20   # the same from a medium of 2.0
    b = ray_batch("scale_3", V, O, scenes)
    t = batch_trace(b)
    assert (t.through & t.decided).sum() >= 50
    assert (b.o.astype(np.float64) * 3.0 != (b.o * F(3.0)).astype(np.float64)).any()          # origin * scale rounds
    size = SIZES[0]
    caps = 0
    for source in GW.SOURCES:
        t = frame_trace(V, "panes_30", size, source, SAMPLES[0])
        caps = int((t.decided & (t.end == GR.CAP) & (t.S == GR.MAX_SURFACES)).sum())
        assert caps >= 100, (source, caps)
    total = {k: 0 for k in GR.ENDINGS}
    for name in ALL_BATCHES:
        for k, v in batch_trace(ray_batch(name, V, O, scenes)).endings().items():
            total[k] += v
    print(f"endings of the decided rays of all batches: {total}; panes_30 corner: {caps} at the cap")
    assert all(total[k] >= 20 for k in ("miss", "opaque", "tir", "reflect", "refract")), total


def test_the_share_thresholds_by_hand():
    """reflect_i and refract_i on hand-picked (n1, n2, cos) triples on either side of 0.001, in the reference's formula: R0 alone
    decides near the normal, Schlick's term at grazing incidence, and TIR zeroes the refract share"""
    n_near = GL.NEAR_BYTE * 3.0 / 255.0
    n_glass = GL.GLASS_REFR_STORED
    for n1, n2, c, refl_below, refr_below in ((1.0, n_near, 1.0, True, False), (1.0, n_near, 0.5, False, False), (1.0, n_glass, 1.0, False, False),
                                              (1.0, n_glass, 1.9e-4, False, True), (1.0, n_glass, 2.2e-4, False, False),
                                              (n_glass, 1.0, 0.5, False, True), (n_near, 1.0, 1.0, True, False)):
        refl, refr, k, _ = GR.fresnel_shares(n1, n2, c)
        assert (refl <= 0.001) == refl_below and (refr <= 0.001) == refr_below, (n1, n2, c, float(refl), float(refr), float(k))
    assert GR.fresnel_shares(n_glass, 1.0, 0.5)[2] < 0 < GR.fresnel_shares(n_glass, 1.0, 0.8)[2]   # beyond and within the critical angle


# ---- the setting off, or nothing translucent ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["materials_1", "scale_3", "room_mix", "bounds_mix"])
def test_reference_past_glass_is_its_plain_guide_where_nothing_is_translucent(V, O, scenes, name):
    b = ray_batch(name, V, O, scenes)
    on, off = batch_trace(b), batch_trace(b, glass=False)
    same = on.decided & off.decided & ~off.first_translucent
    assert same.sum() >= 40 and (off.decided & off.first_translucent).sum() >= 40
    for f in ("hit", "cell", "normal", "rgb", "a0", "S", "L", "bound"):
        assert np.array_equal(getattr(on, f)[same], getattr(off, f)[same]), (name, f)
    assert ((off.end == GR.FIRST) == (off.hit & off.first_translucent))[off.decided].all()
    assert (off.S[off.decided] == off.hit[off.decided]).all()


# ---- planted misreadings -----------------------------------------------------------------------------------------------------------
FLAW_INPUTS = {"ratio_inverted": "materials_1", "depth_straight": "materials_1", "alpha_of_final": "room_mix", "nudge_outwards": "materials_1",
               "miss_is_glass": "materials_1", "cap_9": "panes_30", "grid_origin": "scale_3", "n1_ray_medium": "alpha0"}
PLANT_INPUTS = {"ratio_inverted": "materials_1", "depth_straight": "room_mix", "alpha_of_final": "room_mix", "nudge_outwards": "materials_1"}


def _flawed_count(V, O, L, scenes, name, flaws=(), plant=None):
    if name == "panes_30":
        size, source, k = SIZES[0], "corner", SAMPLES[0]
        t = frame_trace(V, name, size, source, k, flaws=flaws)
        g = GG.sample(L, frame_scene(V, O, name, size), size[0], size[1], k, plant=plant)
    else:
        b = ray_batch(name, V, O, scenes)
        t = batch_trace(b, flaws=flaws)
        g = GG.rays(L, batch_scene(b, O, V), b.o, b.d, plant=plant)
    bad, _ = mismatches(t, g)
    return int(np.any(list(bad.values()), axis=0).sum())


@pytest.mark.parametrize("flaw", GR.GUIDE_FLAWS)
def test_each_planted_flaw_of_the_reference_is_detected(V, O, L, scenes, flaw):
    assert set(FLAW_INPUTS) == set(GR.GUIDE_FLAWS)
    name = FLAW_INPUTS[flaw]
    assert _flawed_count(V, O, L, scenes, name) == 0
    n = _flawed_count(V, O, L, scenes, name, flaws=(flaw,))
    print(f"{flaw} on {name}: {n} decided rays disagree")
    assert n >= 1, flaw


@pytest.mark.parametrize("plant", sorted(PLANT_INPUTS))
def test_each_plant_of_the_checker_is_detected(V, O, L, scenes, plant):
    assert set(PLANT_INPUTS) == set(GG.PLANT) - {None}
    n = _flawed_count(V, O, L, scenes, PLANT_INPUTS[plant], plant=plant)
    print(f"the checker's {plant} on {PLANT_INPUTS[plant]}: {n} decided rays disagree")
    assert n >= 1, plant


# ---- named cases -------------------------------------------------------------------------------------------------------------------
def test_materials_1_ray_384_the_cell_inside_a_larger_leaf(V, O, L, scenes):
    """the hit point's z is 12.99999987 inside a 2 x 2 x 2 leaf: the node does not depend on the floor, so shader_ref64's rule keeps
    the ray, but the float32 run floors 13 where float64 floors 12. The cell's own rule leaves the cell out and keeps the rest. The
    plain guide shows it: past glass the same ray goes on with a refracted z component of 1e-8 and is undecided for that."""
    b = ray_batch("materials_1", V, O, scenes)
    t = batch_trace(b, glass=False)
    g = G.rays(L, batch_scene(b, O, V), b.o, b.d)
    assert t.decided[384] and t.hit[384] and t.cell_near[384] and g.hit[384] == 1
    assert t.cell[384, 2] == 12 and g.cell[384, 2] == 13 and np.array_equal(t.cell[384, :2], g.cell[384, :2])
    assert np.array_equal(t.bytes4()[384], g.albedo[384].astype(np.int64))
    bad, _ = mismatches(t, g)
    assert not np.any(list(bad.values()), axis=0)[384]
    assert not batch_trace(b).decided[384]
