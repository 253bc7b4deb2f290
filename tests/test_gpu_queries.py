"""World queries on the MI355X (vrt_cast_rays, vrt_cast_rays_device, vrt_find_voxels) against the reference's own
functions: o_octree_ray_cast / o_octree_find of the oracle (oracle/octree_oracle.c) on the pointer tree the device tree
was made from, and get_placement_coord restated below. Every field is compared exactly."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import MAPS, GOLDEN, room_tree, room_world, terrain_world

pytestmark = pytest.mark.gpu

F = np.float32
BOXES = [((0, 0, 0), (1024, 1024, 1024)),            # what src/main.cpp:827 passes
         ((-1023, -1023, -1023), (1024, 1024, 1024)),
         ((-5.7, 3.2, 0.9), (70.5, 300.0, 20.0)),     # truncated to int, as ivec3_vec3 does
         ((0, 0, 0), (0, 0, 0))]


def placement(o, d, coord):
    """get_placement_coord (src/main.cpp:315-360) in float32: plain division (a zero component gives inf / NaN),
    std::swap ordering, fmax (a NaN operand loses), |tEntry - tMin| < 1e-4f tested in x, y, z order."""
    o = np.asarray(o, F)
    d = np.asarray(d, F)
    bmin = np.asarray(coord, np.int32).astype(F)
    bmax = bmin + F(1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (bmin - o) / d
        t1 = (bmax - o) / d
    tmin = np.where(t0 > t1, t1, t0)
    t_entry = np.fmax(np.fmax(tmin[0], tmin[1]), tmin[2])
    p = list(int(v) for v in coord)
    with np.errstate(invalid="ignore"):
        for ax in range(3):
            if ax == 2 or abs(F(t_entry - tmin[ax])) < F(1e-4):
                p[ax] += -1 if d[ax] > 0 else 1
                break
    return p


def leaf_words(vobj):
    """the record words vrth_world_records emits for a voxel (host_capi.cpp emit_records); refraction byte 0 under alpha 0"""
    c = int(vobj.color)
    r, g, b, a = (c >> 24) & 255, (c >> 16) & 255, (c >> 8) & 255, c & 255
    q = lambda v, s: int(F(v) * F(s)) & 255
    refr = q(vobj.voxel.refraction, 85.0) if a else 0
    return r | g << 8 | b << 16 | a << 24, refr | q(vobj.voxel.illumination, 255.0) << 8 | q(vobj.voxel.k, 255.0) << 16


def oracle_cast(O, tree, o, d, box):
    L = O.lib()
    n = L.o_octree_ray_cast(tree, O.Vec3(*map(float, o)), O.Vec3(*map(float, d)), O.Vec3(*map(float, box[0])),
                            O.Vec3(*map(float, box[1])))
    if not n:
        return None
    return n.contents


def zero_word_leaves(tree):
    """the leaves of an oracle tree that hold a voxel whose device record words are 0/0 (colour 0, zero material): the
    phantom voxels of SURVEY F3 and the "ghost" volumes the F1 split makes of them (coord = lbb, y > MIN_HEIGHT: the
    reference's ray cast and octree_find hit those). Both layouts store all of them as empty space."""
    out, stack = [], [tree]
    while stack:
        p = stack.pop()
        n = p.contents
        if n.children:
            stack.extend(n.children[i] for i in range(8) if n.children[i])
        elif n.has_voxel and leaf_words(n.voxel) == (0, 0):
            out.append(p)
    return out


class zero_leaves_emptied:
    """with-block: the oracle tree with its zero-word leaves' has_voxel cleared (restored on exit). find_leaf's bounds do not
    depend on has_voxel, so this is the reference's function on the tree as the device holds it."""

    def __init__(self, tree):
        self.nodes = zero_word_leaves(tree)

    def __enter__(self):
        for p in self.nodes:
            p.contents.has_voxel = 0
        return self

    def __exit__(self, *exc):
        for p in self.nodes:
            p.contents.has_voxel = 1
        return False


def check_rays(O, tree, ctx, origins, dirs, box, what):
    """device answers vs the oracle for every ray (on the tree with its zero-word leaves emptied); returns the device's steps"""
    hit, coord, place, leaf, steps = ctx.cast_rays(origins, dirs, box)
    shared = np.asarray(origins).shape == (3,)
    with zero_leaves_emptied(tree):
        compare_rays(O, tree, origins, dirs, box, what, shared, hit, coord, place, leaf)
    assert steps.min() >= 1 and steps.max() <= 512
    return steps


def compare_rays(O, tree, origins, dirs, box, what, shared, hit, coord, place, leaf):
    for i in range(len(dirs)):
        o = origins if shared else origins[i]
        node = oracle_cast(O, tree, o, dirs[i], box)
        ctxt = f"{what} ray {i}: origin {list(o)} dir {list(dirs[i])} box {box}"
        assert bool(hit[i]) == (node is not None), ctxt
        if node is None:
            assert coord[i].tolist() == [-1, -1, -1] and place[i].tolist() == [-1, -1, -1] and leaf[i].tolist() == [0, 0], ctxt
            continue
        want = [node.voxel.coord.x, node.voxel.coord.y, node.voxel.coord.z]
        assert coord[i].tolist() == want, ctxt
        assert place[i].tolist() == placement(o, dirs[i], want), ctxt
        assert tuple(leaf[i].tolist()) == leaf_words(node.voxel), ctxt


def make_rays(rng, n, lo, hi, solid):
    """origins inside / outside the world and inside solid voxels, on integer planes and node faces; directions random,
    axis-aligned, with 0.0 / -0.0 / |d| < 1e-8 components, unnormalised"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    k = n // 8
    ctr = (lo + hi) / 2
    parts = [
        rng.uniform(lo - 40, hi + 40, (k, 3)),                               # around the model
        rng.uniform(-1100, 1100, (k, 3)),                                    # anywhere, in and out of the world
        np.floor(rng.uniform(lo - 8, hi + 8, (k, 3))),                       # integer planes
        np.floor(rng.uniform(lo, hi, (k, 3)) / 16) * 16,                     # node faces (aligned corners)
        solid[rng.integers(0, len(solid), k)] + rng.uniform(0, 1, (k, 3)),   # inside a solid voxel
        solid[rng.integers(0, len(solid), k)].astype(F),                     # on a voxel's corner
        ctr + rng.normal(0, 1, (k, 3)) * (hi - lo),
    ]
    o = np.concatenate(parts).astype(F)
    o = np.concatenate([o, rng.uniform(lo - 200, hi + 200, (n - len(o), 3)).astype(F)])
    d = rng.normal(0, 1, (n, 3)).astype(F)
    # aim a third of them at the model
    aim = rng.random(n) < 0.35
    tgt = rng.uniform(lo, hi, (n, 3)).astype(F)
    d[aim] = (tgt - o)[aim]
    sel = rng.random(n)
    axis = rng.integers(0, 3, n)
    for i in range(n):
        if sel[i] < 0.08:    # axis-aligned
            v = np.zeros(3, F); v[axis[i]] = F(rng.choice([-1.0, 1.0])); d[i] = v
        elif sel[i] < 0.16:  # one component exactly 0.0 or -0.0
            d[i, axis[i]] = F(rng.choice([0.0, -0.0]))
        elif sel[i] < 0.22:  # one component below 1e-8 in magnitude
            d[i, axis[i]] = F(rng.choice([5e-9, -5e-9, 1e-12, -9.9e-9]))
        elif sel[i] < 0.30:  # unnormalised
            d[i] *= F(rng.choice([1e-3, 7.0, 300.0]))
    return o, d


def scene_voxels(O, tree, lo, hi, rng, n=400):
    """cells of solid voxels (by octree_find) in [lo, hi) for origins inside solids"""
    L = O.lib()
    pts = rng.integers(lo, hi, (20000, 3))
    out = []
    for p in pts:
        v = L.o_octree_find(tree, O.IVec3(*map(int, p)))
        if v.coord.y > -1024:
            out.append(p)
        if len(out) >= n:
            break
    if not out:
        out = [lo]
    return np.asarray(out, F)


# name -> (product World, oracle tree, model bounds)
@pytest.fixture(scope="module")
def scenes(V, O):
    out = {}
    rng = np.random.default_rng(7)
    for m in ("dragon", "monu9", "nature"):
        w = V.World()
        assert w.load_vox(os.path.join(MAPS, m + ".vox"))
        t, ok, _ = O.load_vox(os.path.join(MAPS, m + ".vox"))
        assert ok
        out[m] = (w, t)
    data = V.make_custom_vox()
    w = V.World()
    w.load_vox_bytes(data)
    t, ok, _ = O.load_vox(bytes(data))
    assert ok
    out["custom"] = (w, t)
    out["room"] = (room_world(V), room_tree(O))
    tj = json.load(open(os.path.join(GOLDEN, "terrain.json")))
    wd = tj["window"]
    t = O.new_tree()
    O.fill_heights(t, np.load(os.path.join(GOLDEN, "terrain_heights.npz"))["heights"], wd["x0"], wd["z0"], wd["nx"], wd["nz"],
                   tj["band"], tj["floor"])
    out["terrain"] = (terrain_world(V), t)
    bounds = {"dragon": ((0, 0, 0), (128, 128, 128)), "monu9": ((0, 0, 0), (128, 128, 128)), "nature": ((0, 0, 0), (256, 128, 256)),
              "custom": ((0, 0, 0), (64, 64, 64)), "room": ((8, 12, 8), (84, 44, 56)),
              "terrain": ((wd["x0"], 0, wd["z0"]), (wd["x0"] + wd["nx"], 160, wd["z0"] + wd["nz"]))}
    return {k: (v[0], v[1], bounds[k]) for k, v in out.items()}


def upload(ctx, w, how="texels"):
    if how == "texels":
        tex, dim = w.flatten()
        ctx.upload_octree(tex, dim)
    else:
        rec = w.records()
        assert rec is not None
        ctx.upload_records(*rec)


@pytest.fixture(scope="module")
def qctx(V):
    c = V.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", ["dragon", "monu9", "nature", "custom", "room", "terrain"])
def test_rays_match_octree_ray_cast(V, O, qctx, scenes, name):
    w, tree, (lo, hi) = scenes[name]
    upload(qctx, w)
    rng = np.random.default_rng(["dragon", "monu9", "nature", "custom", "room", "terrain"].index(name) + 100)
    solid = scene_voxels(O, tree, lo, hi, rng)
    total, hits, capped = 0, 0, 0
    for bi, box in enumerate(BOXES):
        o, d = make_rays(rng, 5200, lo, hi, solid)
        steps = check_rays(O, tree, qctx, o, d, box, f"{name} box {bi}")
        total += len(d)
        capped += int((steps == 512).sum())
        # the shared-origin form (config 1, picking)
        o1 = o[rng.integers(0, len(o))]
        check_rays(O, tree, qctx, o1, d[:600], box, f"{name} shared origin box {bi}")
        total += 600
        hits += int(qctx.cast_rays(o, d, box)[0].sum())
    assert total >= 20000 and hits > 100, (total, hits)


def test_the_only_difference_from_the_raw_tree_is_zero_word_leaves(V, O, qctx, scenes):
    """On the tree as built -- ghost volumes included -- every ray the device answers differently is one whose reference hit
    is a leaf with record words 0/0, which the device tree stores as empty space; the device then goes on past it exactly
    as the reference does on the tree without that leaf (checked above). nature.vox has 682 such hittable leaves."""
    w, tree, (lo, hi) = scenes["nature"]
    upload(qctx, w)
    rng = np.random.default_rng(21)
    o, d = make_rays(rng, 6000, lo, hi, scene_voxels(O, tree, lo, hi, rng))
    hit, coord, _, _, _ = qctx.cast_rays(o, d, BOXES[0])
    differ = 0
    for i in range(len(d)):
        node = oracle_cast(O, tree, o[i], d[i], BOXES[0])
        same = (node is None and not hit[i]) or (node is not None and hit[i] and
                                                 coord[i].tolist() == [node.voxel.coord.x, node.voxel.coord.y, node.voxel.coord.z])
        if not same:
            assert node is not None and leaf_words(node.voxel) == (0, 0), f"ray {i}: {o[i].tolist()} {d[i].tolist()}"
            differ += 1
    assert 0 < differ < len(d) // 4, differ


def test_the_512_step_cap(V, O, qctx, scenes):
    """rays that end at the loop's cap: a ray that creeps along a tiny component from inside the box but outside the tree"""
    w, tree, _ = scenes["dragon"]
    upload(qctx, w)
    o = np.array([[500.5, 900.25, 500.5], [3.5, 1000.5, 3.5], [700.0, 700.0, 700.0]], F)
    d = np.array([[1e-9, 1e-3, -1e-9], [0.0, 1e-4, 0.0], [1e-9, -1e-9, 1e-4]], F)
    steps = check_rays(O, tree, qctx, o, d, BOXES[0], "cap")
    assert (steps == 512).any(), steps


def test_find_voxels_match_octree_find(V, O, qctx, scenes):
    L = O.lib()
    rng = np.random.default_rng(11)
    for name in ("dragon", "room", "terrain", "custom"):
        w, tree, (lo, hi) = scenes[name]
        upload(qctx, w)
        pts = np.concatenate([rng.integers(lo, hi, (6000, 3)), rng.integers(-1100, 1100, (2000, 3)),
                              rng.choice([-1024, -1023, 0, 1023, 1024], (500, 3)),   # on and beyond the world's edge
                              scene_voxels(O, tree, lo, hi, rng, 500).astype(np.int64)]).astype(np.int32)
        present, leaf = qctx.find_voxels(pts)
        # octree_find's equality finds a merged volume only in its corner column: few points are "solid" in merged scenes
        assert present.sum() >= 5, (name, int(present.sum()))
        with zero_leaves_emptied(tree):
            compare_points(O, L, w, tree, pts, present, leaf, name)


def compare_points(O, L, w, tree, pts, present, leaf, name):
    for i, p in enumerate(pts):
        v = L.o_octree_find(tree, O.IVec3(*map(int, p)))
        ok = v.coord.y > -1024
        assert bool(present[i]) == ok, f"{name} point {p.tolist()}"
        assert tuple(leaf[i].tolist()) == (leaf_words(v) if ok else (0, 0)), f"{name} point {p.tolist()}"
        if ok and i < 800:   # the product's own octree_find agrees
            assert w.find(*map(int, p))["coord"][1] > -1024, f"{name} point {p.tolist()}"


def test_find_voxels_on_the_planes_octree_find_routes_differently(V, O, qctx):
    """octree_find picks a child at (lbb + rtf) / 2 (truncating), the tree splits at lo + (hi - lo) / 2: in the negative half
    of the reference's [-1023, 1024) world the two differ on the planes -512, -768, -896, ..., and a voxel there is not found
    (isVoxelSolid is false) although the ray cast hits it. A small tree with voxels on and beside those planes, all octants."""
    L = O.lib()
    w = V.World()
    tree = O.new_tree()
    planes = [-1023, -897, -896, -895, -769, -768, -767, -513, -512, -511, -256, -1, 0, 1, 3, 511, 512, 1023]
    rng = np.random.default_rng(17)
    vox = set()
    for _ in range(3000):
        v = tuple(int(rng.choice(planes)) if rng.random() < 0.7 else int(rng.integers(-1023, 1024)) for _ in range(3))
        vox.add(v)
    vox |= {(-512, 5, -512), (-512, 5, 3), (3, 5, -768), (-511, 5, -511), (-768, 40, -896), (-896, -512, -768)}
    for i, (x, y, z) in enumerate(sorted(vox)):
        c = [0x50b43cff, 0x644628ff, 0xa0a0a0ff][i % 3]
        w.insert(x, y, z, c)
        L.o_octree_insert(tree, O.VoxelObj(O.IVec3(x, y, z), c, O.Voxel(3.0, 0.0, 0.0)))
    upload(qctx, w)
    pts = np.array(sorted(vox) + [tuple(int(rng.choice(planes)) for _ in range(3)) for _ in range(4000)], np.int32)
    present, leaf = qctx.find_voxels(pts)
    with zero_leaves_emptied(tree):
        compare_points(O, L, w, tree, pts, present, leaf, "negative planes")
    for p in ((-512, 5, -512), (-512, 5, 3), (3, 5, -768)):   # in the tree, not found by octree_find
        assert not present[sorted(vox).index(p)], p
    assert present[sorted(vox).index((-511, 5, -511))]
    # the ray cast routes as the tree does: rays at those voxels hit them
    o, d = make_rays(rng, 4000, (-1023, -1023, -1023), (1024, 1024, 1024), np.array(sorted(vox), F))
    check_rays(O, tree, qctx, o, d, BOXES[1], "negative planes")
    w.close()
    L.o_octree_delete(tree)


def test_options_and_upload_forms_give_the_same_answers(V, O, qctx, scenes):
    """every VRT_OPT_EMPTY_OCTANTS setting and the record upload answer as the texel upload does"""
    w, tree, (lo, hi) = scenes["dragon"]
    rng = np.random.default_rng(3)
    o, d = make_rays(rng, 8000, lo, hi, scene_voxels(O, tree, lo, hi, rng))
    pts = rng.integers(-20, 280, (8000, 3)).astype(np.int32)
    upload(qctx, w)
    ref = qctx.cast_rays(o, d), qctx.find_voxels(pts)
    for how in ("texels", "records"):
        upload(qctx, w, how)
        for opt in (0, 1, 2):
            qctx.set_option(V.OPT_EMPTY_OCTANTS, opt)
            got = qctx.cast_rays(o, d), qctx.find_voxels(pts)
            for a, b in zip(ref[0] + ref[1], got[0] + got[1]):
                assert np.array_equal(a, b), (how, opt)
    qctx.set_option(V.OPT_EMPTY_OCTANTS, 1)


def test_scripted_edit_session_on_dragon(V, O, qctx):
    """src/main.cpp:822-914 against the device tree: pick the centre ray, destroy at coord or build at place on both the
    product World and the oracle tree, patch the device (single patches, batches, box patches, one forced compaction),
    pick again -- every pick equals o_octree_ray_cast on the edited oracle tree"""
    L = O.lib()
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    tree, ok, _ = O.load_vox(os.path.join(MAPS, "dragon.vox"))
    assert ok
    upload(qctx, w)
    rng = np.random.default_rng(5)
    clicks, edits = 0, 0
    color = 0x3c64dcff
    box = BOXES[0]
    for step in range(90):
        eye = np.array([rng.uniform(10, 120), rng.uniform(30, 90), rng.uniform(10, 150)], F)
        tgt = np.array([rng.uniform(40, 90), rng.uniform(10, 60), rng.uniform(40, 90)], F)
        front = tgt - eye
        front = (front / np.sqrt((front * front).sum())).astype(F)
        hit, coord, place, _, _ = qctx.cast_rays(eye, front[None, :], box)
        check_rays(O, tree, qctx, eye, front[None, :], box, f"click {step}")
        clicks += 1
        if not hit[0]:
            continue
        c, p = [int(v) for v in coord[0]], [int(v) for v in place[0]]
        kind = step % 5
        if kind in (0, 1):     # destroy (left click)
            w.remove(*c)
            L.o_octree_remove(tree, O.IVec3(*c))
            targets = [c]
        elif kind == 2:        # build (right click)
            if min(p) < 0:
                continue
            w.insert(*p, color, 3.0, 0.0, 0.0)
            L.o_octree_insert(tree, O.VoxelObj(O.IVec3(*p), color, O.Voxel(3.0, 0.0, 0.0)))
            targets = [p]
        else:                  # a 3x3x3 blast around the hit
            lo_ = [max(v - 1, 0) for v in c]
            hi_ = [v + 1 for v in c]
            for x in range(lo_[0], hi_[0] + 1):
                for y in range(lo_[1], hi_[1] + 1):
                    for z in range(lo_[2], hi_[2] + 1):
                        w.remove(x, y, z)
                        L.o_octree_remove(tree, O.IVec3(x, y, z))
            if qctx.patch_box(w, lo_, hi_) is None:
                upload(qctx, w)
            edits += 1
            continue
        if step % 7 == 0:      # a batch of one more edit
            qctx.patch_begin()
            for t_ in targets:
                if qctx.patch_voxel(w, *t_) is None:
                    qctx.patch_end()
                    upload(qctx, w)
                    break
            else:
                qctx.patch_end()
        else:
            for t_ in targets:
                if qctx.patch_voxel(w, *t_) is None:
                    upload(qctx, w)
        if step == 40:
            qctx.compact()
        edits += 1
        # after the edit: a fan of rays around the centre sees it too
        fan = (front[None, :] + rng.normal(0, 0.02, (64, 3))).astype(F)
        check_rays(O, tree, qctx, eye, fan, box, f"click {step} fan")
    assert clicks >= 50 and edits >= 30, (clicks, edits)
    w.close()
    L.o_octree_delete(tree)


def test_config4_full_extent_against_the_host_ray_cast(V, qctx):
    """the terrain at its full extent (beyond the 2^23-texel stream: records upload) against the product's own
    octree_ray_cast, the reference's function on the same pointer tree"""
    w = terrain_world(V, {"x0": 0, "z0": 0, "nx": 1024, "nz": 1024})
    upload(qctx, w, "records")
    rng = np.random.default_rng(9)
    o = np.concatenate([rng.uniform(0, 1024, (1500, 3)) * [1, 0.1, 1] + [0, 40, 0], rng.uniform(-50, 1100, (500, 3))]).astype(F)
    d = rng.normal(0, 1, (2000, 3)).astype(F)
    d[:, 1] -= 0.5
    hit, coord, place, _, _ = qctx.cast_rays(o, d, BOXES[0])
    ghost = 0
    for i in range(len(d)):
        # vrth_world_ray_cast passes the reference's box (0..1024)
        r = w.ray_cast(tuple(map(float, o[i])), tuple(map(float, d[i])))
        if r is not None and w.find(*r[0])["color"] == 0:
            # a zero-word leaf (the terrain has no voxel of colour 0, none below y = 20): the device tree holds empty space there
            ghost += 1
            continue
        assert bool(hit[i]) == (r is not None and r[1]), i
        if hit[i]:
            assert tuple(coord[i].tolist()) == tuple(r[0]), i
            assert place[i].tolist() == placement(o[i], d[i], r[0]), i
    assert hit.sum() > 200 and ghost < len(d) // 10, (int(hit.sum()), ghost)
    w.close()


def test_device_form_on_a_side_stream_after_a_patch(V, O, qctx):
    """vrt_cast_rays_device on a caller stream ordered after a patch on the context's stream answers as the host form"""
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    tree, ok, _ = O.load_vox(os.path.join(MAPS, "dragon.vox"))
    upload(qctx, w)
    for x in range(40, 60):
        w.remove(x, 30, 60)
        O.lib().o_octree_remove(tree, O.IVec3(x, 30, 60))
    qctx.patch_box(w, (40, 30, 60), (59, 30, 60))
    rng = np.random.default_rng(2)
    o, d = make_rays(rng, 4096, (0, 0, 0), (128, 128, 128), np.array([[50, 30, 60]], F))
    want = qctx.cast_rays(o, d)
    n = len(d)
    d_o, d_d, d_out = qctx.device_alloc(o.nbytes), qctx.device_alloc(d.nbytes), qctx.device_alloc(n * 40)
    flag = qctx.device_alloc(4)
    try:
        import torch
        side = torch.cuda.Stream(device=0)
        sp = side.cuda_stream
        qctx.device_write(d_o, o)
        qctx.device_write(d_d, d)
        # the caller's ordering: the side stream waits for what the context's stream has done (the patch)
        qctx._L.vrt_stream_write_flag(qctx._h, C.c_void_p(flag), 1, None)
        qctx._L.vrt_stream_wait_flag(qctx._h, C.c_void_p(flag), 1, C.c_void_p(sp))
        qctx.cast_rays_device(n, d_o, 3, d_d, d_out, stream=sp)
        side.synchronize()
        got = qctx.device_read(d_out, (n,), V.RAY_HIT_DTYPE, stream=sp)
    finally:
        for p in (d_o, d_d, d_out, flag):
            qctx.device_free(p)
    assert np.array_equal(got["hit"] != 0, want[0]) and np.array_equal(got["coord"], want[1])
    assert np.array_equal(got["place"], want[2]) and np.array_equal(got["leaf"], want[3]) and np.array_equal(got["steps"], want[4])
    check_rays(O, tree, qctx, o[:1500], d[:1500], BOXES[0], "after patch")
    w.close()
    O.lib().o_octree_delete(tree)


def test_empty_world_root_leaf_and_custom_bounds(V, O, qctx):
    """an empty world; a small world given other bounds with a merged volume at y = 0"""
    rng = np.random.default_rng(4)
    o, d = make_rays(rng, 2000, (-50, -50, -50), (50, 50, 50), np.zeros((1, 3), F))
    w = V.World()
    upload(qctx, w)
    hit, coord, place, leaf, steps = qctx.cast_rays(o, d)
    assert not hit.any() and (coord == -1).all() and (leaf == 0).all()
    present, _ = qctx.find_voxels(rng.integers(-1100, 1100, (1000, 3)))
    assert not present.any()
    # the oracle agrees on the empty tree
    check_rays(O, O.new_tree(), qctx, o[:500], d[:500], BOXES[1], "empty")
    w.close()
    # a root that is itself a leaf has no device form (the texel stream of one leaf is refused, vrth_world_records
    # returns -2), so no context holds one; the smallest tree that does: a 4^3 world whose first octant is a merged volume
    # (coord = its lbb, with y = 0) and one unit voxel
    w = V.World((0, 0, 0), (2, 2, 2))
    for x in range(2):
        for y in range(2):
            for z in range(2):
                w.insert(x, y, z, 0x50b43cff)
    assert w.records() is None
    with pytest.raises(V.VrtError):
        qctx.upload_octree(*w.flatten())
    w.close()
    lo, hi = (0, 0, 0), (4, 4, 4)
    w = V.World(lo, hi)
    t = O.lib().o_octree_create(None, O.IVec3(*lo), O.IVec3(*hi))
    vox = [(x, y, z) for x in range(2) for y in range(2) for z in range(2)] + [(3, 2, 3)]
    for x, y, z in vox:
        w.insert(x, y, z, 0x50b43cff)
        O.lib().o_octree_insert(t, O.VoxelObj(O.IVec3(x, y, z), 0x50b43cff, O.Voxel(3.0, 0.0, 0.0)))
    p = qctx.default_params()
    for k in range(3):
        p.world_min[k], p.world_max[k] = lo[k], hi[k]
    qctx.set_params(p)
    try:
        upload(qctx, w)
        o2, d2 = make_rays(rng, 3000, lo, hi, np.zeros((1, 3), F))
        o2 = (o2 / 30).astype(F)
        for box in BOXES:
            check_rays(O, t, qctx, o2, d2, box, "4^3 world")
        pts = rng.integers(-2, 4, (500, 3)).astype(np.int32)
        present, leaf = qctx.find_voxels(pts)
        for i, q in enumerate(pts):
            v = O.lib().o_octree_find(t, O.IVec3(*map(int, q)))
            assert bool(present[i]) == (v.coord.y > -1024), q
    finally:
        qctx.set_params(qctx.default_params())
        w.close()
        O.lib().o_octree_delete(t)


def test_error_states(V):
    ctx = V.Context(0)
    try:
        o, d = np.zeros(3, F), np.ones((4, 3), F)
        L = ctx._L
        box = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1024, 1024, 1024)
        out = (V.RayHit * 4)()
        # before any upload
        assert L.vrt_cast_rays(ctx._h, 4, o.ctypes.data, 0, d.ctypes.data, box[0], box[1], out) == -5
        assert L.vrt_find_voxels(ctx._h, 1, np.zeros(3, np.int32).ctypes.data, np.zeros(3, np.uint32).ctypes.data) == -5
        assert L.vrt_cast_rays_device(ctx._h, 4, None, 0, None, box[0], box[1], None, None) == -5
        w = V.World()
        assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
        upload(ctx, w)
        # NULL buffers with n > 0; a bad stride
        assert L.vrt_cast_rays(ctx._h, 4, None, 0, d.ctypes.data, box[0], box[1], out) == -1
        assert L.vrt_cast_rays(ctx._h, 4, o.ctypes.data, 0, None, box[0], box[1], out) == -1
        assert L.vrt_cast_rays(ctx._h, 4, o.ctypes.data, 0, d.ctypes.data, box[0], box[1], None) == -1
        assert L.vrt_cast_rays(ctx._h, 4, o.ctypes.data, 1, d.ctypes.data, box[0], box[1], out) == -1
        assert L.vrt_find_voxels(ctx._h, 1, None, np.zeros(3, np.uint32).ctypes.data) == -1
        assert L.vrt_cast_rays_device(ctx._h, 4, None, 0, None, box[0], box[1], None, None) == -1
        # n == 0: a successful no-op, NULL buffers allowed
        assert L.vrt_cast_rays(ctx._h, 0, None, 0, None, None, None, None) == 0
        assert L.vrt_find_voxels(ctx._h, 0, None, None) == 0
        assert L.vrt_cast_rays_device(ctx._h, 0, None, 3, None, None, None, None, None) == 0
        h = ctx.cast_rays(np.zeros((0, 3), F), np.zeros((0, 3), F))
        assert all(len(a) == 0 for a in h)
        # inside an open patch batch
        ctx.patch_begin()
        assert L.vrt_cast_rays(ctx._h, 4, o.ctypes.data, 0, d.ctypes.data, box[0], box[1], out) == -5
        assert L.vrt_find_voxels(ctx._h, 1, np.zeros(3, np.int32).ctypes.data, np.zeros(3, np.uint32).ctypes.data) == -5
        ctx.patch_end()
        assert L.vrt_cast_rays(ctx._h, 4, o.ctypes.data, 0, d.ctypes.data, box[0], box[1], out) == 0
        w.close()
    finally:
        ctx.close()
