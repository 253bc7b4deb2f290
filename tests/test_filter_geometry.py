"""The coverage model of the guided filter's launch geometry (tests/filter_geometry.py) on the CPU: the probe of the compiled tile
constants, the model against a walk over the launch's own index arithmetic, the tile counts the seam shapes were derived from, and
the property tests/test_gpu_filter_seams.py relies on -- its shape list contains every event at every lattice step in both axes and
every form at steps 2 and 4, with the tile this build has. A retuned tile under which the shapes stop crossing seams fails here."""
import pytest

import filter_geometry as FG

TILE_32_8 = {"kBlockX": 64, "kBlockY": 4, "kVarX": 32, "kVarY": 8, "kLatX": 32, "kLatY": 8, "kLatticeMaxStep": 4}
# the frames of the stateless tests of tests/test_gpu_filter_hdr.py and tests/test_gpu_filter_var.py, with their level counts
OLDER_SHAPES = ((70, 37), (8, 8), (9, 1), (1, 1), (1, 9), (65, 5), (20, 12), (90, 41), (33, 9), (40, 24), (43, 21), (24, 13))


@pytest.fixture(scope="module")
def K(V):
    return FG.constants(V)


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    import oracle_filter_var as FV
    return FV.build(tmp_path_factory.mktemp("oracle_filter_seams"))


def test_the_probe_returns_the_compiled_constants(K):
    assert tuple(K) == FG.NAMES
    assert all(v >= 1 for v in K.values())
    assert K["kLatticeMaxStep"] & (K["kLatticeMaxStep"] - 1) == 0                   # steps are powers of two
    assert K["kBlockX"] * K["kBlockY"] <= 1024 and K["kVarX"] * K["kVarY"] <= 1024 and K["kLatX"] * K["kLatY"] <= 1024


def _walk(k, width, height, s):
    """the lattice kernel's index arithmetic, workgroup by workgroup -> (early returns, per-axis sets of events seen, pixels owned)"""
    gx, gy = FG.grid(k, width, height, s)
    owned, returns = {}, 0
    seen = {"x": set(), "y": set()}
    tiles = {"x": {}, "y": {}}
    for by in range(gy):
        for bx in range(gx):
            rx, ry = bx % s, by % s
            lx0, ly0 = (bx // s) * k["kLatX"], (by // s) * k["kLatY"]
            gone_x, gone_y = rx + s * lx0 >= width, ry + s * ly0 >= height
            if gone_x and rx < width:                                            # a class with pixels, not one the frame is too narrow for
                seen["x"].add("early_return")
            if gone_y and ry < height:
                seen["y"].add("early_return")
            if gone_x or gone_y:
                returns += 1
                continue
            tiles["x"].setdefault(rx, set()).add(lx0)
            tiles["y"].setdefault(ry, set()).add(ly0)
            for ty in range(k["kLatY"]):
                for tx in range(k["kLatX"]):
                    x, y = rx + s * (lx0 + tx), ry + s * (ly0 + ty)
                    if x >= width:
                        seen["x"].add("ragged")
                    if y >= height:
                        seen["y"].add("ragged")
                    if x < width and y < height:
                        owned[x, y] = owned.get((x, y), 0) + 1
    for axis in ("x", "y"):
        if max(len(t) for t in tiles[axis].values()) >= 3:
            seen[axis].add("interior")
        if "ragged" not in seen[axis] and "early_return" not in seen[axis]:
            seen[axis].add("exact")
    return returns, seen, owned


@pytest.mark.parametrize("size", [(257, 33), (131, 35), (256, 32), (65, 5), (33, 70), (3, 2), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_model_is_the_launchs_own_arithmetic(size):
    """every pixel is owned by exactly one lane, and the model's events and early returns are those of a walk over the grid"""
    w, h = size
    for e in FG.levels_of(TILE_32_8, w, h, 3):
        returns, seen, owned = _walk(TILE_32_8, w, h, e["step"])
        assert len(owned) == w * h and set(owned.values()) == {1}, e["step"]
        assert returns == e["returns"], e["step"]
        assert seen["x"] == e["x"] and seen["y"] == e["y"], (e["step"], seen, e)


def test_the_tile_counts_the_shapes_were_derived_from():
    assert FG.class_tiles(257, 1, 32) == [9] and FG.class_tiles(257, 2, 32) == [5, 4] and FG.class_tiles(257, 4, 32) == [3, 2, 2, 2]
    assert FG.class_tiles(33, 1, 8) == [5] and FG.class_tiles(33, 2, 8) == [3, 2] and FG.class_tiles(33, 4, 8) == [2, 1, 1, 1]
    assert FG.class_tiles(131, 4, 32) == [2, 2, 2, 1] and FG.class_tiles(35, 4, 8) == [2, 2, 2, 1]
    for s in (1, 2, 4):
        assert FG.axis_events(256, s, 32) - {"interior"} == {"exact"} and FG.axis_events(32, s, 8) - {"interior"} == {"exact"}
    assert [e["returns"] for e in FG.levels_of(TILE_32_8, 257, 33, 3)] == [0, 10 * 6 - 9 * 5, 12 * 8 - 9 * 5]
    # the forms: levels 2 and 3 end on steps 2 and 4, levels 3 and 4 pass through them, level 4 ends gathered
    forms = {n: [(e["step"], e["lattice"], e["first"], e["last"]) for e in FG.levels_of(TILE_32_8, 257, 33, n)] for n in (2, 3, 4)}
    assert forms[2] == [(1, True, True, False), (2, True, False, True)]
    assert forms[3] == [(1, True, True, False), (2, True, False, False), (4, True, False, True)]
    assert forms[4] == [(1, True, True, False), (2, True, False, False), (4, True, False, False), (8, False, False, True)]


def test_the_seam_shapes_contain_every_event_and_form(K):
    """with the tile the library was compiled with"""
    no_event, no_form = FG.missing(K, FG.SEAM_SHAPES, FG.SEAM_LEVELS)
    assert not no_event and not no_form, (K, no_event, no_form)
    for w, h in FG.SEAM_SHAPES:                                                 # each shape crosses a seam at the widest lattice step
        s = K["kLatticeMaxStep"]
        assert max(FG.class_tiles(w, s, K["kLatX"])) >= 2 or max(FG.class_tiles(h, s, K["kLatY"])) >= 2, (w, h)


def test_the_model_rejects_shape_lists_that_stop_crossing_seams():
    """the frames the older device tests filter: no interior tile past step 1 in x, no early return in y (what the seam shapes add);
    and the seam shapes themselves under a tile twice as wide"""
    no_event, _ = FG.missing(TILE_32_8, OLDER_SHAPES, (1, 2, 3, 4, 5, 8))
    assert {(2, "x", "interior"), (4, "x", "interior"), (2, "y", "early_return"), (4, "x", "early_return"), (4, "y", "early_return")} <= set(no_event)
    assert (2, "x", "early_return") not in no_event                              # 65 x 5 takes it
    wider = dict(TILE_32_8, kLatX=64)
    no_event, _ = FG.missing(wider, FG.SEAM_SHAPES, FG.SEAM_LEVELS)
    assert (4, "x", "interior") in no_event
    _, no_form = FG.missing(dict(TILE_32_8, kLatticeMaxStep=8), FG.SEAM_SHAPES, FG.SEAM_LEVELS)
    assert (8, False, False) in no_form


@pytest.mark.parametrize("kind", ["smooth", "random"])
@pytest.mark.parametrize("size", [(257, 33), (33, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_seam_inputs_carry_a_change_across_the_seam_by_step_4_alone(K, L, size, kind):
    """tests/filter_seam_cases.py's sensitivity condition on the checkers, at the two frames that between them have an x and a y seam
    with room on both sides (the device module asserts it of all four before it asks the device anything)"""
    import filter_seam_cases as SC
    w, h = size
    SC.assert_sensitive(L, K, kind, w, h, *SC.make(kind, w, h))
