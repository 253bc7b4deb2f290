"""The sample-stack sweep on the CPU (sample_sweep_worlds.py; the device side is test_gpu_sample_sweep.py): that the 36 cases are a
test and not a walk through sky. The generator is deterministic; each family holds what it is there for, measured on the checkers
alone (asserted floors); the checkers themselves, on index 0 and 3 of every family, agree with the float64 restatements
(path_ref64.py through test_deep_reference64's comparison, guide_ref64.py through test_guides_reference64's) on the corner-source
rays at the case's own setting and uniforms; and every planted flaw the checkers offer changes a byte in at least one case."""
import numpy as np
import pytest

import guide_ref64 as GR
import oracle_emit_mis as om
import oracle_guides as G
import oracle_guides_glass as GG
import oracle_paths as core
import oracle_rays
import path_ref64 as PR
import sample_sweep_worlds as sw
import shader_ref64 as R
from test_deep_reference64 import CEILING
from test_guides_reference64 import cap_rule, check_sample
from test_rays_reference64 import check_floats

F = np.float32
ALL_SOURCES = {"corner": (False, False), "jitter": (True, False), "lens": (False, True), "jitter+lens": (True, True)}   # jitter, lens
MODE = {"uniform": (om.UNIFORM, 0), "power": (om.POWER, 0), "power+mis": (om.POWER, 1)}
REF_RULE = {"off": dict(emit=None, mis=False), "uniform": dict(emit="uniform", mis=False), "power": dict(emit="power", mis=False),
            "power+mis": dict(emit="power", mis=True)}
REF_INDICES = (0, 3)
MIN_TRANSLUCENT_PIXELS, MIN_TRANSLUCENT_CASES = 20, 2
MIN_CONNECTIONS = 50

# Undecided share of the in-world corner rays at the case's setting, sample 0, measured on the reference alone; the cap is
# test_deep_reference64's rule: that share plus a quarter of itself, rounded up to the next 0.005, never above its CEILING[D].
# (family, index): measured share of the path reference, of the guide reference (all rays / through-glass rays)
MEASURED = {
    ("opaque", 0): (0.0064, 0.0000, 0.0000),    # D = 1, ceiling 0.15
    ("opaque", 3): (0.0026, 0.0000, 0.0000),    # D = 8, ceiling 0.30
    ("mixed", 0): (0.1372, 0.0000, 0.0000),     # D = 3, ceiling 0.15
    ("mixed", 3): (0.1042, 0.0000, 0.0000),     # D = 2, ceiling 0.15
    ("inside", 0): (0.0064, 0.0000, 0.0000),    # D = 1, ceiling 0.15
    ("inside", 3): (0.1198, 0.0000, 0.0000),    # D = 8, ceiling 0.30
    ("origin", 0): (0.0032, 0.0000, 0.0000),    # D = 3, ceiling 0.15
    ("origin", 3): (0.0182, 0.0000, 0.0000),    # D = 2, ceiling 0.15
    ("uniforms", 0): (0.0016, 0.0000, 0.0000),  # D = 1, ceiling 0.15
    ("uniforms", 3): (0.0052, 0.0000, 0.0000),  # D = 8, ceiling 0.30
    ("far", 0): (0.0080, 0.0000, 0.0000),       # D = 3, ceiling 0.15
    ("far", 3): (0.0156, 0.0000, 0.0000),       # D = 2, ceiling 0.15
}


@pytest.fixture(scope="module")
def PL(tmp_path_factory):
    return om.build(tmp_path_factory.mktemp("oracle_sample_sweep_cpu"))


@pytest.fixture(scope="module")
def RL(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_sample_sweep_rays"))


@pytest.fixture(scope="module")
def GL(tmp_path_factory):
    return GG.build(tmp_path_factory.mktemp("oracle_sample_sweep_guides"))


@pytest.fixture(scope="module")
def cases(V, O):
    out = {(f, i): sw.case(V, O, f, i) for f in sw.FAMILIES for i in range(sw.N_INDEX)}
    yield out
    for c in out.values():
        c.close()


def corner_rays(RL, O, case):
    if not hasattr(case, "_corner"):
        o, d = oracle_rays.frame_rays(RL, case.scene(O), case.W, case.H)
        case._corner = (np.ascontiguousarray(np.broadcast_to(np.asarray(o, F).reshape(-1, 3), d.shape)), d)
    return case._corner


def checker_sample(PL, RL, O, case, k=0, log=False, flaw=core.FLAW_NONE, D=None):
    """the checker's corner-source sample k at the case's setting (D: another depth)"""
    s = case.setting
    o, d = corner_rays(RL, O, case)
    mode, mis = MODE.get(s["rule"], (om.UNIFORM, 0))
    on = s["rule"] != "off"
    return core.shade(PL, case.scene(O), o, d, D or s["D"], s["radius"], case.list if on else None, case.weights if on else None, mode, mis,
                      width=case.W, sample=k, log=log, flaw=flaw)


# ---- determinism ---------------------------------------------------------------------------------------------------------------
def test_two_builds_of_every_case_are_equal(V, O, cases):
    for (f, i), a in cases.items():
        b = sw.case(V, O, f, i)
        try:
            assert np.array_equal(a.tex, b.tex) and a.dim == b.dim and np.array_equal(a.records, b.records), (f, i)
            assert a.uniforms == b.uniforms and a.bounds == b.bounds and a.pose == b.pose and a.lens == b.lens, (f, i)
            assert a.setting == b.setting and (a.W, a.H) == (b.W, b.H) and a.outside_pose == b.outside_pose, (f, i)
            assert np.array_equal(a.rays[0].view(np.uint32), b.rays[0].view(np.uint32)), (f, i)
            assert np.array_equal(a.rays[1].view(np.uint32), b.rays[1].view(np.uint32)), (f, i)
            assert np.array_equal(a.list, b.list) and np.array_equal(a.weights, b.weights), (f, i)
        finally:
            b.close()


def test_the_setting_a_name_carries_rebuilds_the_case(cases):
    for (f, i), c in cases.items():
        assert c.setting == sw.scheduled_setting(f, i) and c.name().startswith(f"sweep case {f} {i} [D={c.setting['D']} ")
        assert (c.W, c.H) == sw.SIZES[i % 2] and len(c.rays[1]) == sw.N_RAYS
    assert all(cases[("opaque", i)].setting["rule"] == "off" for i in (0, 2, 4))
    assert all(cases[("opaque", i)].setting["rule"] != "off" for i in (1, 3, 5))


# ---- what each family holds, on the checkers alone -----------------------------------------------------------------------------
def test_every_case_passes_the_pose_rule(PL, RL, O, cases):
    for key, c in cases.items():
        ids = checker_sample(PL, RL, O, c, D=1)[1][:, 0]
        assert np.count_nonzero(ids) * sw.MIN_HIT_SHARE >= c.W * c.H, (key, int(np.count_nonzero(ids)))
        assert c.redraws <= sw.MAX_REDRAWS


def test_opaque_worlds_are_opaque_and_the_others_are_not(V, cases):
    for (f, i), c in cases.items():
        assert V.tree_is_opaque(c.tex) == (f == "opaque"), (f, i)


def test_translucent_first_hits(GL, O, cases):
    for f in ("mixed", "inside", "uniforms"):
        counts = []
        for i in range(sw.N_INDEX):
            c = cases[(f, i)]
            g = G.sample(GL, c.scene(O), c.W, c.H, 0)
            counts.append(int(((g.hit != 0) & (g.albedo[..., 3] < 255)).sum()))
        print(f"{f}: pixels whose first hit has alpha below 255: {counts}")
        assert sum(n >= MIN_TRANSLUCENT_PIXELS for n in counts) >= MIN_TRANSLUCENT_CASES, (f, counts)


def test_emitter_connections_reach_their_emitters(PL, RL, O, cases):
    for f in sw.FAMILIES:
        counts = []
        for i in range(sw.N_INDEX):
            c = cases[(f, i)]
            counts.append(int(checker_sample(PL, RL, O, c, log=True)[3]["conn_hit"].sum()) if c.setting["rule"] != "off" else 0)
        print(f"{f}: vertices with conn_hit at sample 0: {counts}")
        assert sum(counts) >= MIN_CONNECTIONS, (f, counts)


def test_the_lists_of_origin_hold_merged_and_negative_entries(cases):
    for i in range(sw.N_INDEX):
        lst = cases[("origin", i)].list
        assert {1, 2, 4} <= set(lst[:, 3].tolist()) and (lst[:, :3] < 0).any(), (i, sorted(set(lst[:, 3].tolist())))


def test_the_inside_eyes_are_in_their_voxels(cases):
    """by the host library's own lookup"""
    for i, kind in enumerate(sw.INSIDE_KINDS):
        c = cases[("inside", i)]
        cell = [int(v) for v in np.floor(np.asarray(c.cam[2][:3], np.float64) * c.uniforms["voxel_scale"])]
        colour, refraction, illum, _ = sw.PALETTE[sw.LAMP if kind == "cube" else kind]
        if kind == "cube":   # a merged leaf: the host's ray cast from the eye ends at once, in the leaf itself, whatever the direction
            lo, size = c.cubes[0]
            assert size > 1 and list(lo) + [size] in c.list.tolist() and all(l <= v < l + size for l, v in zip(lo, cell)), (cell, lo, size)
            eye = tuple(float(v) * c.uniforms["voxel_scale"] for v in c.cam[2][:3])
            for d in ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.3, 0.5, -0.8)):
                assert c.world.ray_cast(eye, d) == (tuple(lo), True), (eye, d, c.world.ray_cast(eye, d))
            w0, w1 = c.words[c.list.tolist().index(list(lo) + [size])]
            assert (int(w1) >> 8) & 0xff == 255 and int(w0) >> 24 == 255, (hex(w0), hex(w1))   # the lamp: illumination 1, alpha 255
            continue
        found = c.world.find(*cell)
        assert found["color"] == colour and found["refraction"] == pytest.approx(refraction), (i, cell, found)
        assert found["illumination"] == pytest.approx(illum), (i, cell, found)
    assert sw.PALETTE[sw.AIR12][0] & 0xff == 0 and sw.PALETTE[sw.AIR12][1] == 1.2


def test_the_uniforms_family_sets_what_the_rooms_hold_constant(cases):
    scales, zero, below = set(), 0, 0
    for i in range(sw.N_INDEX):
        c = cases[("uniforms", i)]
        u = c.uniforms
        scales.add(u["voxel_scale"])
        ld = np.array(u["light_dir"], F)
        assert abs(float(np.linalg.norm(ld.astype(np.float64))) - 1.0) < 1e-6
        zero += int((ld == 0).sum() == 1)
        below += int(ld[1] < 0)
        assert 0.0 <= min(u["global_light"]) and max(u["global_light"]) <= 1.5
        kinds = {0: (sw.LAMP, sw.EMBER, sw.BLACK), 1: (sw.GLASS, sw.WATER, sw.GREEN_GLASS)}.get(i // 2)
        assert tuple(u["highlighted"]) in c.vox and (kinds is None or c.vox[tuple(u["highlighted"])] in kinds), (i, u["highlighted"])
    assert scales == {0.5, 1.25, 2.0} and zero == 2 and below == 1


# ---- the checkers on these worlds against the float64 restatements ----------------------------------------------------------------
def _ref_world(case):
    return R.World(case.tex, case.dim, *(case.bounds or ((-1023,) * 3, (1024,) * 3)))


@pytest.mark.parametrize("index", REF_INDICES)
@pytest.mark.parametrize("family", sw.FAMILIES)
def test_the_checkers_match_the_float64_references(PL, RL, GL, O, cases, family, index):
    check_against_references(PL, RL, GL, O, cases[(family, index)], MEASURED[(family, index)])


def check_against_references(PL, RL, GL, O, c, measured):
    """the comparison itself, on any Case-shaped world (test_edit_sessions.py runs it on edited ones) with its measured shares"""
    s, u = c.setting, c.uniforms
    o, d = corner_rays(RL, O, c)
    what = c.name()
    world = _ref_world(c)
    scene = c.scene(O)
    # the path rules
    rgba, idd, rgb = checker_sample(PL, RL, O, c)
    t = PR.PathTrace.rays(world, o, d, c.W, sample=0, voxel_scale=u["voxel_scale"], global_light=u["global_light"],
                          light_dir=np.array(u["light_dir"], F), highlighted=u["highlighted"], depth=s["D"], tan_radius=s["radius"],
                          **REF_RULE[s["rule"]])
    f = t.frame()
    res = R.compare(f, rgba, idd)
    share = f.in_world_undecided_share()
    dec = f.all_decided()
    print(f"{what}: in-world {int((~f.outside).sum())} decided {int(dec.sum())} decided hits {int((dec & f.hit).sum())} undecided share {share:.4f}")
    assert res["bad"] == 0, (what, res)
    cap = min(cap_rule(measured[0]), CEILING[s["D"]])
    assert measured[0] <= CEILING[s["D"]] and share <= cap, (what, share, cap)
    assert (dec & f.hit).sum() * sw.MIN_HIT_SHARE * 2 >= c.W * c.H, (what, int((dec & f.hit).sum()))
    want, bound, decf = t.radiance()
    check_floats(rgb, want, bound, decf, what, min_decided=c.W * c.H // 2)
    # the guides, past glass and plain
    caps = (cap_rule(measured[1]), cap_rule(measured[2]))
    assert max(caps) <= 0.15, (what, caps)
    tg = GR.GuideTrace.rays(world, o, d, voxel_scale=u["voxel_scale"], highlighted=u["highlighted"], glass=True)
    check_sample(tg, GG.rays(GL, scene, o, d), GG.rays(GL, scene, o, d, plant="alpha_of_final"), what + " guides past glass", caps)
    tp = GR.GuideTrace.rays(world, o, d, voxel_scale=u["voxel_scale"], highlighted=u["highlighted"], glass=False)
    check_sample(tp, G.rays(GL, scene, o, d), None, what + " guides plain", caps)


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------
PATH_FLAWS = {"power_six_faces": (core.FLAW_POWER_SIX_FACES, ("power", "power+mis")), "power_no_p": (core.FLAW_POWER_NO_P, ("power", "power+mis")),
              "mis_bounce_full": (core.FLAW_MIS_BOUNCE_FULL, ("power+mis",)), "mis_bounce_none": (core.FLAW_MIS_BOUNCE_NONE, ("power+mis",))}


@pytest.mark.parametrize("flaw", sorted(PATH_FLAWS))
def test_each_planted_path_flaw_changes_a_case(PL, RL, O, cases, flaw):
    code, rules = PATH_FLAWS[flaw]
    changed = []
    for key, c in cases.items():
        if c.setting["rule"] in rules:
            a, b = checker_sample(PL, RL, O, c), checker_sample(PL, RL, O, c, flaw=code)
            if not np.array_equal(a[0], b[0]):
                changed.append(key)
    print(f"{flaw}: changes a byte in {len(changed)} cases: {changed}")
    assert changed, flaw


@pytest.mark.parametrize("plant", sorted(k for k in G.PLANT if k) + sorted(k for k in GG.PLANT if k))
def test_each_plant_of_the_guide_checkers_changes_a_case(GL, O, cases, plant):
    mod = G if plant in G.PLANT else GG
    changed = []
    for key, c in cases.items():
        scene = c.scene(O)
        jitter, lens = ALL_SOURCES[c.setting["source"]]          # the case's own source at sample 1: a lens moves the origin off the
        args = (GL, scene, c.W, c.H, 1, jitter, *(c.lens if lens else (0.0, 1.0)))   # eye, and sample 0 is the pinhole's
        a, b = mod.sample(*args), mod.sample(*args, plant=plant)
        if any(not np.array_equal(getattr(a, k).view(np.uint8), getattr(b, k).view(np.uint8)) for k in ("normal", "albedo", "depth", "hit")):
            changed.append(key)
    print(f"{plant}: changes a byte in {len(changed)} cases: {changed}")
    assert changed, plant
