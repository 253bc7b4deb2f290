"""The edit sessions on the CPU (edit_sessions.py; the device side is test_gpu_edit_sessions.py). The sessions are pure functions; each
holds the vocabulary its plan names and stays under the fall-back cap; the host structures, patched in a chain by the product's own
plan_patch / apply_patch / compact_records under vrt_patch.cpp's rules (vrt.PatchSession), answer at every checkpoint like a fresh
layout of the edited world's stream; every cached fact a group voids changes the checkers' output on the route that reads it, so that
a device which kept the old value cannot pass test_gpu_edit_sessions.py; and the checkers themselves, on the edited worlds, agree with
the float64 restatements at each session's last checkpoint under test_sample_sweep.py's rules.

`pytest -s` prints one line per cached fact and checkpoint at which the reference's output changes because of it."""
import copy

import numpy as np
import pytest

import edit_sessions as es
import oracle_emit_mis as om
import oracle_emit_power as oep
import oracle_guides as G
import oracle_guides_glass as GG
import oracle_rays
import sample_sweep_worlds as sw
import test_sample_sweep as tss

F = np.float32
N_RANDOM = 2000
KEYS = [(f, i) for f in es.FAMILIES for i in es.INDICES]

# Undecided share of the in-world corner rays at the LAST checkpoint of each session, at the case's setting, sample 0, measured on the
# reference alone; the caps are test_sample_sweep.py's rule on them (that share plus a quarter of itself, rounded up to the next
# 0.005, never above test_deep_reference64's CEILING[D]).
# (family, index): measured share of the path reference, of the guide reference (all rays / through-glass rays)
MEASURED = {
    ("opaque", 0): (0.0032, 0.0016, 0.0000),    # D = 1, ceiling 0.15
    ("opaque", 1): (0.0000, 0.0000, 0.0000),    # D = 2, ceiling 0.15
    ("mixed", 0): (0.0271, 0.0016, 0.0035),     # D = 3, ceiling 0.15
    ("mixed", 1): (0.2943, 0.0000, 0.0000),     # D = 8, ceiling 0.30
    ("inside", 0): (0.0319, 0.0016, 0.0000),    # D = 1, ceiling 0.15
    ("inside", 1): (0.0286, 0.0000, 0.0000),    # D = 2, ceiling 0.15
    ("origin", 0): (0.0032, 0.0000, 0.0000),    # D = 3, ceiling 0.15
    ("origin", 1): (0.2109, 0.0026, 0.0000),    # D = 8, ceiling 0.30
    ("uniforms", 0): (0.0016, 0.0016, 0.0000),  # D = 1, ceiling 0.15
    ("uniforms", 1): (0.0000, 0.0000, 0.0000),  # D = 2, ceiling 0.15
    ("far", 0): (0.0064, 0.0000, 0.0000),       # D = 3, ceiling 0.15
    ("far", 1): (0.0208, 0.0000, 0.0000),       # D = 8, ceiling 0.30
}


@pytest.fixture(scope="module")
def PL(tmp_path_factory):
    return om.build(tmp_path_factory.mktemp("oracle_edit_sessions_cpu"))


@pytest.fixture(scope="module")
def RL(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_edit_sessions_rays"))


@pytest.fixture(scope="module")
def GL(tmp_path_factory):
    return GG.build(tmp_path_factory.mktemp("oracle_edit_sessions_guides"))


def bounds_of(case):
    return case.bounds or ((-1023,) * 3, (1024,) * 3)


def probe_points(S, cp):
    """every edited voxel, its 26 neighbours, the eye's cell and N_RANDOM points around the content"""
    g = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    edited = np.array(cp.edited or [S.eye_cell], np.int64)
    near = (edited[:, None, :] + g[None]).reshape(-1, 3)
    keys = np.array(sorted(cp.vox))
    lo, hi = keys.min(axis=0) - 8, keys.max(axis=0) + 9
    rng = np.random.default_rng([es.SEED, es.FAMILIES.index(S.family), S.index, cp.k, 0x9017])
    pts = np.concatenate([near, [S.eye_cell], rng.integers(lo, hi, size=(N_RANDOM, 3))])
    return np.clip(pts, S.wlo, S.whi - 1).astype(np.int32)


def guide_bytes(mod, GL, O, cp):
    g = mod.sample(GL, cp.scene(O), cp.W, cp.H, 0)
    return np.concatenate([np.ascontiguousarray(getattr(g, k)).view(np.uint8).ravel() for k in ("normal", "albedo", "depth", "hit")])


def sample_bytes(s):
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(len(s[0]), -1) for a in s], axis=1)


@pytest.fixture(scope="module")
def runs(V, O, PL, RL, GL):
    """every session once, on the chained host probe; per checkpoint what the tests below assert on, computed while the world stands
    as the checkpoint describes it"""
    out = {}
    for f, i in KEYS:
        notes, S_of = [], [None]

        def target(S):
            c = S.case
            S.mirror = es.Mirror(O, S)
            S_of[0] = S
            assert np.array_equal(O.flatten(S.mirror.tree)[0], c.tex), (f, i)
            S.probe = V.PatchSession(c.tex, c.dim, *bounds_of(c))
            S.first_records = S.probe.counts()["n_records"]
            S.eye0 = S.vox.get(S.eye_cell)
            S.prev = dict(opaque=V.tree_is_opaque(c.tex), list=c.list, weights=c.weights, eye=S.vox.get(S.eye_cell),
                          frame=sample_bytes(tss.checker_sample(PL, RL, O, c)), plain=guide_bytes(G, GL, O, c), glass=guide_bytes(GG, GL, O, c))
            return S.probe

        def at_checkpoint(S, cp, counts, t):
            # the oracle's pointer tree, edited in step, is the edited world: what the device test's queries are held to
            assert np.array_equal(O.flatten(S.mirror.tree)[0], cp.tex), cp.name()
            pts = probe_points(S, cp)
            n = dict(k=cp.k, counts=counts, probe=t.check(cp.tex, cp.dim, pts, S.eye_cell), totals=t.counts(), ops=cp.ops)
            n["stale"] = t.check(cp.tex, cp.dim, pts, S.eye_cell, stale=True) if n["probe"]["repointed"] else None
            n["walk"] = (cp.list, np.array(oep.thresholds([int(w) for w in cp.weights]), np.uint32).reshape(-1))
            n["opaque"] = V.tree_is_opaque(cp.tex)
            now = dict(opaque=n["opaque"], list=cp.list, weights=cp.weights, eye=S.vox.get(S.eye_cell),
                       frame=sample_bytes(tss.checker_sample(PL, RL, O, cp)), plain=guide_bytes(G, GL, O, cp), glass=guide_bytes(GG, GL, O, cp))
            n["prev"], n["now"] = S.prev, now
            n["ray_pixel"] = S.state.get("ray_pixel")
            if cp.setting["rule"] != "off" and not (np.array_equal(S.prev["list"], cp.list) and np.array_equal(S.prev["weights"], cp.weights)):
                old = copy.copy(cp)                      # the edited world sampled with the list and table of before the group
                old.list, old.weights = S.prev["list"], S.prev["weights"]
                n["stale_list_frame"] = sample_bytes(tss.checker_sample(PL, RL, O, old))
            S.prev = now
            notes.append(n)

        S, groups = es.run(V, O, f, i, target=target, at_checkpoint=at_checkpoint, mirror=lambda *a: S_of[0].mirror(*a))
        out[(f, i)] = (S, groups, notes)
    yield out
    for S, _, _ in out.values():
        S.mirror.close()
        S.probe.close()
        S.close()


# ---- purity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,index", KEYS)
def test_sessions_are_pure_functions(V, O, runs, family, index):
    _, first, _ = runs[(family, index)]
    S, second = es.run(V, O, family, index)              # on no target at all: the plan does not depend on what is driven
    try:
        assert len(first) == len(second) == es.N_CHECKPOINTS
        for (ops_a, _, a), (ops_b, _, b) in zip(first, second):
            assert ops_a == ops_b and a.k == b.k
            assert np.array_equal(a.tex, b.tex) and a.dim == b.dim and np.array_equal(a.records, b.records)
            assert np.array_equal(a.list, b.list) and np.array_equal(a.weights, b.weights) and a.vox == b.vox
            assert np.array_equal(a.rays[0].view(np.uint32), b.rays[0].view(np.uint32))
            assert np.array_equal(a.rays[1].view(np.uint32), b.rays[1].view(np.uint32))
            assert a.name() == f"edit session {family} {index} checkpoint {a.k}" and len(a.rays[1]) == sw.N_RAYS
    finally:
        S.close()


def test_the_walk_over_the_voxels_sees_what_the_host_ray_cast_sees(V, O):
    """edit_sessions' notion of `visible` against World.ray_cast_many, on the rays that end in a single voxel from an eye in empty space"""
    S = es.session(V, O, "mixed", 0)
    try:
        hit, coords = S.world.ray_cast_many(tuple(float(v) for v in S.eye), S.dirs)
        keys = np.array(list(S.vox))
        lo, hi = keys.min(axis=0).astype(float), (keys.max(axis=0) + 1).astype(float)
        got = {p: S._march(S.dirs[p].astype(np.float64), lo, hi) for p in np.flatnonzero(hit == 1)}
        # a merged leaf answers with its corner, whichever of its cells the ray enters: compared where the walk ends in a single voxel
        px = [p for p, v in got.items() if v is not None and not sw._mergeable(S.vox, v)]
        assert len(px) > 50
        same = sum(got[p] == tuple(coords[p].tolist()) for p in px)
        assert same >= len(px) - 2, (same, len(px))      # float32 against float64 on a grazing ray
    finally:
        S.close()


# ---- vocabulary and fall-back -------------------------------------------------------------------------------------------------
def _ops_of(groups, kind):
    return [op for ops, _, _ in groups for op in ops if op[0] == kind]


@pytest.mark.parametrize("family,index", KEYS)
def test_each_session_holds_its_vocabulary_and_the_fallback_cap(V, runs, family, index):
    S, groups, notes = runs[(family, index)]
    items = es.items_of(family, index)
    edits = sum(c["edits"] for _, c, _ in groups)
    fell = sum(c["fallbacks"] for _, c, _ in groups)
    print(f"edit session {family} {index}: {edits} patch operations, {fell} full uploads, records {S.first_records} -> {notes[-1]['totals']}")
    assert fell * es.MAX_FALLBACK_SHARE <= edits, (edits, fell)
    strokes = _ops_of(groups, "batch")
    assert strokes and all(8 <= len(b[1]) <= 12 for b in strokes)
    assert len(_ops_of(groups, "compact")) == 1 and _ops_of(groups, "box")
    opaque = [V.tree_is_opaque(S.case.tex)] + [n["opaque"] for n in notes]
    if family == "opaque":
        assert opaque == [True, False, False, True], opaque                    # tree_is_opaque flips twice
        assert [len(n["walk"][0]) for n in notes] == [1, 1, 1] and notes[0]["walk"][0][0, 3] == 1 and notes[1]["walk"][0][0, 3] == 2
    else:
        assert not any(opaque)
    if "emit_split" in items:
        k = [j for j, g in enumerate(S.plan) if "emit_split" in g][0]
        before = groups[k - 1][2].list if k else S.case.list
        assert len(notes[k]["walk"][0]) > len(before) and 4 in before[:, 3].tolist()   # one entry of side 4 became many
    if "emit_clear" in items:
        assert len(notes[1]["walk"][0]) == 0 and S.case.setting["rule"] != "off"      # sampling on with an empty list
        lst, _ = notes[2]["walk"]
        assert len(lst) == 1 and groups[2][2].vox[tuple(lst[0, :3].tolist())] == sw.BLACK
    eye = [S.eye0] + [n["now"]["eye"] for n in notes]
    if "eye_in" in items:
        k = [j for j, g in enumerate(S.plan) if "eye_in" in g][0]
        assert eye[0] is None and eye[k + 1] == es.EYE_KIND[(family, index)] and eye[-1] is None, eye
    if "eye_remove" in items:
        assert eye[1] is not None and eye[2] is None, eye
    if "box_anchor" in items:
        assert any(op[1][0] < 64 * ((op[2][0]) // 64) <= op[2][0] for op in _ops_of(groups, "box")), "no box across x = 64 n"
    if "box_negative" in items:
        assert any(max(op[2]) < 0 for op in _ops_of(groups, "box"))
    if family == "uniforms":
        h = tuple(S.case.uniforms["highlighted"])
        first = groups[0][2].vox.get(h)
        assert first != S.vox0[h] and (first is None) == (index == 1)       # once removed, once another material
    if (family, index) == es.LONG:
        rec = [r for _, c, _ in groups for r in c["records"]]
        falls = [j for j in range(1, len(rec)) if rec[j] < rec[j - 1]]
        cap, regrown = S.first_records, 0
        for r in rec:                                                            # patch_device(): outgrown, the array doubles
            if r > cap:
                cap, regrown = 2 * r, regrown + 1
        print(f"edit session {family} {index}: record count falls at operations {falls}, the allocation is outgrown {regrown} times")
        assert len(_ops_of(groups[2:], "voxel")) >= es.LONG_EDITS
        assert notes[-1]["totals"]["compactions"] >= 2 and len(falls) >= 2      # the explicit one and vrt_patch_plan's own
        assert regrown >= 1


# ---- the chained host probe -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,index", KEYS)
def test_the_patched_host_structures_answer_like_fresh_layouts(runs, family, index):
    S, groups, notes = runs[(family, index)]
    saw_stale = 0
    for n in notes:
        p, what = n["probe"], f"edit session {family} {index} checkpoint {n['k']}"
        assert p["wide"], what                           # every session's world has a wide form: the cell pass compares something
        assert p["bad_cells"] == 0 and p["bad_records"] == 0, (what, p["bad_cells"], p["bad_records"])
        assert p["opaque"] == (n["opaque"], n["opaque"]), (what, p["opaque"])
        assert p["emitters_equal"] and p["n_emitters"][0] == p["n_emitters"][1], what
        assert np.array_equal(p["list"], n["walk"][0]) and np.array_equal(p["cdf"], n["walk"][1]), what
        assert p["root0"][0] == p["root0"][1], (what, p["root0"])
        assert p["texels"][0] == p["texels"][1] and p["tex_dim"][0] == p["tex_dim"][1], (what, p["texels"], p["tex_dim"])
        assert p["live_records"] == p["fresh_records"], (what, p["live_records"], p["fresh_records"])
        if n["ops"][-1] == ("compact",):
            assert p["n_records"] == p["fresh_records"], (what, p["n_records"], p["fresh_records"])
        else:
            assert p["n_records"] >= p["fresh_records"]
        if n["stale"] is not None:                       # the re-point the last patch made, planted out: the probe must notice
            saw_stale += 1
            assert n["stale"]["bad_cells"] > 0 and n["stale"]["bad_records"] == 0, (what, n["stale"]["bad_cells"])
            print(f"wide cells: {what}: {n['stale']['bad_cells']} lookups differ with the re-pointed cell left stale")
    if index % 2 == 1:
        assert saw_stale >= 1                             # these sessions' checkpoints come after patches, not after a compaction


def test_a_batch_goes_on_after_a_patch_that_voids_the_wide_layout(V):
    """PatchBatch::wide_invalid on the chained probe, by hand-written streams (edit_sessions.VOID_STEPS): the first patch of the batch
    voids the wide layout, the next two are planned and applied on the records alone, and after every one of them and after the
    batch's end the structures answer like a fresh layout of that step's own stream"""
    assert es.hand_stream(es.VOID_START).tolist() == [1, 0, 0, 0x81, 3, 0, 0x80, 0, 5, 0, 0, 0, 200, 40, 90, 255, 255, 0, 0, 255,
                                                      6, 0, 0, 0x01, 7, 0, 0x80, 0, 200, 40, 90, 255, 255, 0, 0, 255]   # `regular`
    pts = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3)
    t = V.PatchSession(es.hand_stream(es.VOID_START), es.VOID_DIM, *es.VOID_BOUNDS)
    try:
        first = t.check(es.hand_stream(es.VOID_START), es.VOID_DIM, pts, (1, 2, 0))
        assert first["wide"] and first["bad_cells"] == 0 and first["bad_records"] == 0
        t.patch_begin()
        voided = []
        for voxel, path, tree in es.VOID_STEPS:
            assert t.plan(*voxel) == path, (voxel, t.plan(*voxel))
            voided.append(t.apply(path, V.subtree_records(es.hand_stream(tree), path))[0])
        assert voided == [1, 0, 0], voided               # the first patch voids the layout; the others never see it
        t.patch_end()
        for stale in (False, True):                      # no re-point is left to plant: the layout was rebuilt, or never
            p = t.check(es.hand_stream(es.VOID_STEPS[-1][2]), es.VOID_DIM, pts, (1, 2, 0), stale=stale)
            assert not p["wide"] and not p["repointed"] and p["bad_records"] == 0 and p["bad_cells"] == 0, p
            assert p["texels"][0] == p["texels"][1] and p["tex_dim"] == (es.VOID_DIM, es.VOID_DIM), (p["texels"], p["tex_dim"])
            assert p["live_records"] == p["fresh_records"] and p["opaque"] == (True, True)
    finally:
        t.close()
    # the same patches one at a time, each its own batch: the layout is rebuilt (as none: a unit internal node) after the first
    t = V.PatchSession(es.hand_stream(es.VOID_START), es.VOID_DIM, *es.VOID_BOUNDS)
    try:
        for voxel, path, tree in es.VOID_STEPS:
            assert t.plan(*voxel) == path
            t.apply(path, V.subtree_records(es.hand_stream(tree), path))
            p = t.check(es.hand_stream(tree), es.VOID_DIM, pts, (1, 2, 0))
            assert not p["wide"] and p["bad_records"] == 0 and p["texels"][0] == p["texels"][1], (voxel, p)
    finally:
        t.close()


# ---- every transition is observable in the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("family,index", KEYS)
def test_every_voided_fact_changes_the_checkers_output(runs, family, index):
    S, groups, notes = runs[(family, index)]
    c = S.case
    seen = set()
    for n in notes:
        prev, now, what = n["prev"], n["now"], f"edit session {family} {index} checkpoint {n['k']}"
        if prev["opaque"] != now["opaque"]:
            px = n["ray_pixel"]
            assert px is not None and not np.array_equal(prev["frame"][px], now["frame"][px]), (what, px)
            print(f"opacity: {what}: tree_is_opaque {prev['opaque']} -> {now['opaque']}, the full sample changes at pixel {px} (through the glass)")
        if "stale_list_frame" in n:
            # a device that kept the old list and table samples the EDITED world with them: that picture is not the right one
            diff = np.flatnonzero((n["stale_list_frame"] != now["frame"]).any(axis=1))
            assert len(diff) > 0, what
            print(f"emitter list: {what}: {len(prev['list'])} -> {len(now['list'])} entries, the sample with the old list and table differs "
                  f"on {len(diff)} pixels (rule {c.setting['rule']})")
        if prev["eye"] != now["eye"]:
            assert not np.array_equal(prev["frame"][0], now["frame"][0]), what
            print(f"eye medium: {what}: the eye's cell {prev['eye']} -> {now['eye']}, the frame's first pixel changes")
        changed = [key for key in ("plain", "glass") if not np.array_equal(prev[key], now[key])]
        assert changed, what                             # an eye inside glass has one plain first hit, whatever the world holds
        seen |= set(changed)
        print(f"guides: {what}: the plain planes change in {int((prev['plain'] != now['plain']).sum())} bytes, those past glass in "
              f"{int((prev['glass'] != now['glass']).sum())}")
    assert seen == {"plain", "glass"}, seen


# ---- the checkers on the edited worlds against the float64 restatements ----------------------------------------------------------
@pytest.mark.parametrize("family,index", KEYS)
def test_the_checkers_match_the_float64_references_on_the_edited_worlds(PL, RL, GL, O, runs, family, index):
    S, groups, _ = runs[(family, index)]
    tss.check_against_references(PL, RL, GL, O, groups[-1][2], MEASURED[(family, index)])
