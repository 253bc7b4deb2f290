"""Frames, world queries and ray batches interleaved on one context. The three entry points fill the scene and light blocks of
their kernel arguments through the same builders and take the same base variant, and each decides for itself what it may assume
of the world outside wide root 0: a frame takes `root0_only` and a root tightened around its eye, a ray batch `root0_only`
alone, a query neither. A decision of one leaking into another through the shared code would show here: every result, in
either call order, equals the oracle's byte for byte and equals the same call on a fresh context that did nothing else.

Three worlds: content near one corner of the default world, all of it inside one 64-cell of wide root 0 (the frames' eye
inside that cell, so both shortcuts apply to them; the rays and points start outside wide root 0 and aim into the cell); and
the two hand-written streams of test_gpu_parity in a world [0, 8)^3, which take the record-array (v2) and explicit-AABB (v1)
fallbacks of the base variant."""
import ctypes as C

import numpy as np
import pytest

import oracle_rays
from test_gpu_queries import leaf_words, oracle_cast, placement, zero_leaves_emptied

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 64, 48
N = 64
BOX = ((0, 0, 0), (1024, 1024, 1024))   # what src/main.cpp:827 passes, Context.cast_rays' default
LEAF_COLOR = 0xc8285aff   # the hand-written streams' leaf: texels (200, 40, 90, 255), (255, 0, 0, 255)


def _tx(value, alpha):
    return [value & 255, (value >> 8) & 255, (value >> 16) & 255, alpha]


def _rays(rng, starts, targets):
    """one ray per start, aimed at its target, lengths 0.5 .. 2 (used as given)"""
    d = (targets - starts) * rng.uniform(0.5, 2.0, (len(starts), 1)) / np.linalg.norm(targets - starts, axis=1, keepdims=True)
    return starts.astype(F), d.astype(F)


def _corner_world(V, O):
    """A 16 x 16 floor with a wall and a pillar on it, inside [16, 40)^3: wide root 0 is [0, 1024)^3, and the deepest node that
    can stand in for it is its 64-cell [0, 64)^3 (the content spans two of that cell's 16-cells)."""
    vox = [(x, 10, z) for x in range(20, 36) for z in range(20, 36)]
    vox += [(20, y, z) for y in range(11, 19) for z in range(20, 36, 2)]
    vox += [(x, y, 30) for x in (28, 29) for y in range(11, 24)]
    w, tree = V.World(), O.new_tree()
    for i, (x, y, z) in enumerate(vox):
        c = [0x50b43cff, 0x644628ff, 0xa0a0a0ff][i % 3]
        w.insert(x, y, z, c)
        O.lib().o_octree_insert(tree, O.VoxelObj(O.IVec3(x, y, z), c, O.Voxel(3.0, 0.0, 0.0)))
    tex, dim = w.flatten()
    w.close()
    rng = np.random.default_rng(30)
    # starts outside wide root 0 (x or z below 0) and so outside [0, 64)^3; three in four aimed at the floor's top, the rest above it all
    starts = np.stack([rng.uniform(-40, -4, N), rng.uniform(14, 60, N), rng.uniform(-40, 50, N)], axis=1)
    targets = np.stack([rng.uniform(21, 35, N), np.full(N, 11.0), rng.uniform(21, 35, N)], axis=1)
    targets[3::4, 1] = rng.uniform(40, 60, N // 4)
    o, d = _rays(rng, starts, targets)
    assert ((o[:, 0] < 0) | (o[:, 2] < 0)).all()
    return dict(tex=tex, dim=dim, bounds=None, tree=tree, pose=(50.5, 40.5, 50.5, -135.0, -43.0), o=o, d=d)


def _hand_tree(O, lo, hi, spec, keep):
    """an oracle tree node by node; spec: "leaf" (a voxel volume, coord = its minimum corner) or {child slot: spec}, split as
    find_leaf splits (lo + (hi - lo) / 2, so a unit cell's child 7 is the cell itself)"""
    n = O.lib().o_octree_create(None, O.IVec3(*lo), O.IVec3(*hi))
    if spec == "leaf":
        n.contents.voxel = O.VoxelObj(O.IVec3(*lo), LEAF_COLOR, O.Voxel(3.0, 0.0, 0.0))
        n.contents.has_voxel = 1
        return n
    kids = (C.POINTER(O.Octree) * 8)()
    mid = [a + (b - a) // 2 for a, b in zip(lo, hi)]
    for slot, sub in spec.items():
        bits = (slot & 4, slot & 2, slot & 1)
        kids[slot] = _hand_tree(O, [m if b else a for a, m, b in zip(lo, mid, bits)], [h if b else m for m, h, b in zip(mid, hi, bits)],
                                sub, keep)
    keep.append(kids)   # the node points into this array: it lives as long as the case does (these trees are never deleted)
    n.contents.children = C.cast(kids, C.POINTER(C.POINTER(O.Octree)))
    return n


def _small_world(O, name):
    """test_custom_world_bounds_and_unit_internal_node's streams, with the pointer tree each one flattens"""
    leaf = [200, 40, 90, 255, 255, 0, 0, 255]
    if name == "regular":     # [0, 4)^3 and [4, 6)^3 are leaf volumes
        stream = _tx(1, 0x81) + _tx(3 | 0x800000, 0) + _tx(5, 0) + leaf + _tx(6, 0x01) + _tx(7 | 0x800000, 0) + leaf
        spec = {0: "leaf", 7: {0: "leaf"}}
    else:                     # the unit cell [4, 5)^3 is an internal node whose child 7 is the leaf
        stream = (_tx(1, 0x80) + _tx(2, 0) + _tx(3, 0x01) + _tx(4, 0) + _tx(5, 0x01) + _tx(6, 0) + _tx(7, 0x80) +
                  _tx(8 | 0x800000, 0) + leaf)
        spec = {7: {0: {0: {7: "leaf"}}}}
    keep = []
    tree = _hand_tree(O, (0, 0, 0), (8, 8, 8), spec, keep)
    tex = np.array(stream, np.uint8)
    rng = np.random.default_rng(31)
    # three in four start in the world's empty space (regular: beside and above the two volumes) and aim at the content; the rest
    # start outside the world, where octree_ray_cast finds nothing and the shader enters through the world's face
    starts = np.stack([rng.uniform(0.1, 3.9, N), rng.uniform(6.1, 7.9, N), rng.uniform(4.1, 7.9, N)], axis=1)
    starts[3::4] = np.stack([rng.uniform(-6, -1, N // 4), rng.uniform(9, 14, N // 4), rng.uniform(-6, 14, N // 4)], axis=1)
    targets = rng.uniform(4.05, 4.95, (N, 3))
    if name == "regular":
        targets[::2] = rng.uniform(0.5, 3.5, (N // 2, 3))
    targets[5::8] = starts[5::8] + (0.3, 4.0, 0.2)   # an eighth, from inside, leave through the top: no answer finds anything
    o, d = _rays(rng, starts, targets)
    return dict(tex=tex, dim=3, bounds=((0, 0, 0), (8, 8, 8)), tree=tree, keep=keep, pose=(1.3, 2.1, 0.7, 52.0, 18.0), o=o, d=d)


CALLS = ("frame 0", "frame 1", "frame 2", "cast_rays", "find_voxels", "shade_rays 0", "shade_rays 2")


def build_case(V, O, R, name):
    """the world, the calls' inputs and the oracle's answer to each call (no device involved)"""
    case = _corner_world(V, O) if name == "corner" else _small_world(O, name)
    tex, dim, pose, o, d = case["tex"], case["dim"], case["pose"], case["o"], case["d"]
    case["cam"] = V.camera_block(pose[:3], pose[3], pose[4], W, H)[:3]
    s = O.make_scene(tex, dim, *case["cam"])
    if case["bounds"]:
        s.bounds_min[:], s.bounds_max[:] = case["bounds"]
        assert np.array_equal(O.flatten(case["tree"])[0], tex), "the hand-built tree is not the stream's"
    want = {}
    for mode in (0, 1, 2):
        rgba, idd, _, st = O.render(s, W, H, mode)
        assert st["hits"] > 20, (name, mode, st["hits"])
        want[f"frame {mode}"] = (rgba, idd)
    # octree_ray_cast and octree_find on the tree as the device holds it (test_gpu_queries: zero-word leaves are empty space there)
    with zero_leaves_emptied(case["tree"]):
        hits = [oracle_cast(O, case["tree"], o[i], d[i], BOX) for i in range(N)]
        coord = np.array([(h.voxel.coord.x, h.voxel.coord.y, h.voxel.coord.z) if h else (-1, -1, -1) for h in hits], np.int32)
        want["cast_rays"] = (np.array([h is not None for h in hits]), coord,
                             np.array([placement(o[i], d[i], coord[i]) if h else (-1, -1, -1) for i, h in enumerate(hits)], np.int32),
                             np.array([leaf_words(h.voxel) if h else (0, 0) for h in hits], np.uint32))
        # the points: where each ray starts, and the voxel it hits (one inside the content's cell where it hits none)
        inside = (30, 12, 30) if name == "corner" else (4, 4, 4)
        case["pts"] = np.concatenate([np.floor(o).astype(np.int32), np.where(coord[:, :1] >= 0, coord, np.array(inside, np.int32))])
        found = [O.lib().o_octree_find(case["tree"], O.IVec3(*map(int, p))) for p in case["pts"]]
    n_hit = int(want["cast_rays"][0].sum())
    assert N // 4 <= n_hit < N, (name, n_hit)
    want["find_voxels"] = (np.array([v.coord.y > -1024 for v in found]),
                           np.array([leaf_words(v) if v.coord.y > -1024 else (0, 0) for v in found], np.uint32))
    if name == "corner":
        assert want["find_voxels"][0][N:].sum() >= N // 4 and not want["find_voxels"][0][:N].any()
    want["shade_rays 0"] = oracle_rays.mean(R, s, o, d, 0, 8, 5, 2)
    want["shade_rays 2"] = oracle_rays.mean(R, s, o, d, 2, 8, 5, 2)
    # what a miss looks like in mode 0: a ray that starts above all content and goes straight up
    sky = oracle_rays.shade(R, s, np.array([[2.0, s.bounds_max[1] - 0.5, 6.0]], F), np.array([[0.0, 1.0, 0.0]], F), 0)[0][0]
    n_shaded = int(np.count_nonzero(np.any(want["shade_rays 0"][0] != sky, axis=1)))
    assert N // 4 <= n_shaded < N, (name, n_shaded)
    case["want"] = want
    return case


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_rays"))


def _context(V, case):
    c = V.Context(0)
    p = c.default_params()
    if case["bounds"]:
        p.world_min[:], p.world_max[:] = case["bounds"]
    c.set_params(p)
    c.upload_octree(case["tex"], case["dim"])
    c.set_camera(*case["cam"])
    return c


def _call(ctx, case, what):
    if what.startswith("frame"):
        return ctx.dispatch(W, H, int(what[-1]))
    if what == "cast_rays":
        return ctx.cast_rays(case["o"], case["d"])
    if what == "find_voxels":
        return ctx.find_voxels(case["pts"])
    return ctx.shade_rays(case["o"], case["d"], int(what[-1]), width=8, first_sample=5, n_samples=2)


def _check(case, what, got, fresh, when):
    for a, b in zip(got, fresh):
        assert np.array_equal(a, b), f"{what} ({when}) differs from the same call on a fresh context"
    for k, (a, b) in enumerate(zip(got, case["want"][what])):   # (cast_rays: every output but the device's step count)
        bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
        assert not len(bad), f"{what} ({when}), output {k}: {len(bad)} entries differ from the oracle, first {bad[0]}: {a[bad[0]]} for {b[bad[0]]}"


@pytest.mark.parametrize("name", ["corner", "regular", "unit-internal"])
def test_interleaved_entry_points_equal_the_oracle_and_a_fresh_context(V, O, R, name):
    case = build_case(V, O, R, name)
    fresh = {}
    for what in CALLS:   # each call alone, on a context that does nothing else
        c = _context(V, case)
        try:
            fresh[what] = _call(c, case, what)
        finally:
            c.close()
        _check(case, what, fresh[what], fresh[what], "fresh context")
    ctx = _context(V, case)
    try:
        for order, when in ((CALLS, "frames first"), (CALLS[::-1], "ray batches first")):
            for what in order:
                _check(case, what, _call(ctx, case, what), fresh[what], when)
    finally:
        ctx.close()
