"""Seeded edit sessions over the sweep's worlds (test_edit_sessions.py, test_gpu_edit_sessions.py, fuzz/fuzz_edits.py) -- TEST
INFRASTRUCTURE ONLY, not collected by pytest.

session(V, O, family, index) is a pure function of (SEED, family, index): it starts from sample_sweep_worlds.case(family, index) and
plans N_CHECKPOINTS groups of edits, each out of the vocabulary below, on the world as the groups before it left it. A group is a list
of operations

    ("voxel", xyz, material or None)            one voxel inserted (a palette index) or removed (None), one patch_voxel
    ("box", lo, hi, [(xyz, material or None)])  every edit of the list, all inside [lo, hi], then ONE patch_box
    ("batch", [voxel operations])               a brush stroke: patch_begin, a patch_voxel per edit, patch_end
    ("compact",)                                an explicit compaction

and drive() is the one place that carries them out: on the host World and the voxel dictionary, and in step on a target with
Context's editing methods -- a vrt.Context (the device) or a vrt.PatchSession (the chained host probe). Where a patch is refused
(None) the target gets the full upload, as the patch tests do; drive() counts those. Session.checkpoint(k) is the world as it then
stands in a Case's shape: its flatten(), its records, the emitter list and words of oracle_emit_power.walk, the case's own pose,
uniforms, lens, frame size and setting, and a ray batch redrawn by the case's rule on the edited voxels.

PLAN names what each session's three groups hold; _assert_vocabulary() holds at import that every item of the vocabulary stands in
at least two sessions (the one long session, `mixed` 1, is the exception the item is defined by). An item that cannot do what its name
says on the world it meets (no visible voxel, no free block for the lamp) raises: a session is never silently thinner than its plan.

One rule of vrt_patch.cpp no World edit reaches: a patch that voids the wide layout in the middle of a batch
(PatchBatch::wide_invalid). The layout is voided only by an internal node of unit size inside an aligned cube, which no sub-tree of the
host library in a cubic world holds. vrt_patch_apply takes the caller's sub-tree, though: VOID_START / VOID_STEPS below are that
batch, written by hand in the world [0, 8)^3, for the probe (test_edit_sessions.py) and for a Context (test_gpu_edit_sessions.py)."""
import copy
import tempfile

import numpy as np

import oracle_emit_power as oep
import oracle_rays
import sample_sweep_worlds as sw
from test_gpu_shade_rays import _ray_mix

SEED = sw.SEED
FAMILIES = sw.FAMILIES
INDICES = (0, 1)
N_CHECKPOINTS = 3
LONG = ("mixed", 1)
LONG_EDITS, LONG_SIDE = 800, 24       # a patch appends some ten records: 300 edits stay far below vrt_patch_plan's own compaction
MAX_FALLBACK_SHARE = 3                 # per session at most one operation in three may need the full upload
F = np.float32

PLAN = {   # the emitter chains stand where the schedule has emitter sampling on (far 0 and far 1 by power: the threshold table)
    ("opaque", 0): (("strip_emitters", "emit_gain", "glass_on_ray", "visible"), ("emit_merge", "box_fill", "visible", "stroke"),
                    ("glass_off_ray", "visible", "compact_last")),
    ("opaque", 1): (("strip_emitters", "emit_gain", "glass_on_ray", "visible"), ("emit_merge", "compact_mid", "box_clear", "visible", "stroke"),
                    ("glass_off_ray", "visible")),
    ("mixed", 0): (("visible", "box_glass"), ("stroke", "visible", "box_clear"), ("visible", "box_fill", "compact_last")),
    ("mixed", 1): (("eye_in", "visible", "compact_mid", "stroke"), ("box_fill", "visible"), ("long_run", "eye_out", "visible")),
    ("inside", 0): (("emit_split", "visible", "box_clear"), ("eye_remove", "emit_clear", "visible", "stroke"),
                    ("emit_black", "visible", "box_fill", "compact_last")),
    ("inside", 1): (("visible", "stroke"), ("eye_remove", "compact_mid", "visible", "box_glass"), ("visible",)),
    ("origin", 0): (("box_anchor", "visible"), ("box_negative", "visible", "stroke"), ("visible", "box_glass", "compact_last")),
    ("origin", 1): (("box_negative", "visible"), ("compact_mid", "eye_in", "box_anchor", "visible", "stroke"), ("eye_out", "visible")),
    ("uniforms", 0): (("highlight_replace", "visible"), ("eye_in", "stroke", "visible", "box_fill"), ("eye_out", "visible", "compact_last")),
    ("uniforms", 1): (("highlight_remove", "visible"), ("compact_mid", "box_clear", "visible", "stroke"), ("visible", "box_glass")),
    ("far", 0): (("emit_split", "box_anchor", "visible"), ("emit_clear", "box_negative", "visible", "stroke"),
                 ("emit_black", "visible", "box_clear", "compact_last")),
    ("far", 1): (("emit_split", "box_anchor", "visible"), ("compact_mid", "emit_clear", "visible", "stroke", "box_fill"),
                 ("emit_black", "visible")),
}
EYE_KIND = {("mixed", 1): sw.GLASS, ("origin", 1): sw.STONE, ("uniforms", 0): sw.WATER}
RAY_GLASS = {("opaque", 0): sw.GLASS, ("opaque", 1): sw.WATER}
VOCABULARY = ("visible", "glass_on_ray", "glass_off_ray", "emit_gain", "emit_merge", "emit_split", "emit_clear", "emit_black", "eye_in",
              "eye_out", "eye_remove", "box_fill", "box_clear", "box_glass", "box_anchor", "box_negative", "stroke", "compact_last",
              "compact_mid", "highlight_replace", "highlight_remove", "long_run")
EMITTER_ITEMS = ("strip_emitters", "emit_gain", "emit_merge", "emit_split", "emit_clear", "emit_black")


def items_of(family, index):
    return [it for group in PLAN[(family, index)] for it in group]


def _assert_vocabulary():
    assert set(PLAN) == {(f, i) for f in FAMILIES for i in INDICES} and all(len(g) == N_CHECKPOINTS for g in PLAN.values())
    for item in VOCABULARY:
        where = [key for key in PLAN if item in items_of(*key)]
        if item == "long_run":
            assert where == [LONG], where
        elif item.startswith("highlight"):          # the highlighted voxel is edited in two sessions: once removed, once replaced
            assert len(where) == 1 and where[0][0] == "uniforms", (item, where)
        else:
            assert len(where) >= 2, (item, where)
    for key, groups in PLAN.items():
        f, i = key
        assert "stroke" in items_of(f, i) and all("visible" in g for g in groups), key   # every checkpoint shows another picture
        last = [g[-1] == "compact_last" for g in groups]
        assert (i % 2 == 0) == any(last), key                                   # half the sessions: the last operation before a checkpoint
        mid = [g.index("compact_mid") < len(g) - 1 for g in groups if "compact_mid" in g]
        assert (i % 2 == 1) == bool(mid) and all(mid), key                      # the others: patches follow it
        if f == "opaque":                           # the world's tree_is_opaque flips twice
            assert "glass_on_ray" in groups[0] and "glass_off_ray" in groups[2], key
        if f == "inside":
            assert "eye_remove" in items_of(f, i), key
        for a, b in (("eye_in", "eye_out"), ("glass_on_ray", "glass_off_ray"), ("emit_gain", "emit_merge"), ("emit_split", "emit_clear"),
                     ("emit_clear", "emit_black")):
            if a in items_of(f, i) and (b in items_of(f, i) or a.startswith("eye") or a.startswith("glass")):
                ga = [k for k, g in enumerate(groups) if a in g][0]
                gb = [k for k, g in enumerate(groups) if b in g][0]
                assert ga < gb, (key, a, b)         # in order over the checkpoints
    for key in PLAN:                                # the emitter items stand where the schedule samples emitters (opaque 0 apart)
        if any(it in EMITTER_ITEMS for it in items_of(*key)) and key != ("opaque", 0):
            assert sw.scheduled_setting(*key)["rule"] != "off", key
    assert sum(sw.scheduled_setting(*key)["rule"].startswith("power") for key in PLAN if "emit_clear" in items_of(*key)) >= 2
    for f in ("far", "origin"):
        for item in ("box_anchor", "box_negative"):
            assert any(item in items_of(f, i) for i in INDICES), (f, item)


_assert_vocabulary()

_RL = None


def rays_lib():
    """oracle_rays' library, compiled once per process: the frame's rays are what `visible` means"""
    global _RL
    if _RL is None:
        _RL = oracle_rays.build(tempfile.mkdtemp(prefix="edit_sessions_rays_"))
    return _RL


class Checkpoint(sw.Case):
    def name(self):
        return f"edit session {self.family} {self.index} checkpoint {self.k}"


def apply_edit(world, vox, xyz, m, mirror=None):
    """one voxel of the world and of the dictionary; mirror(xyz, m, replaces): a second tree that takes the same edit"""
    xyz = tuple(int(v) for v in xyz)
    if mirror:
        mirror(xyz, m, m is not None and xyz in vox)
    if m is None:
        world.remove(*xyz)
        vox.pop(xyz, None)
    else:
        if xyz in vox:
            world.remove(*xyz)
        c, refr, illum, k = sw.PALETTE[m]
        world.insert(xyz[0], xyz[1], xyz[2], c, refr, illum, k)
        vox[xyz] = m


def drive(t, world, vox, ops, mirror=None):
    """carries the operations out on world and vox and, edit by edit, on the target t -> dict(edits, fallbacks, records, own): the patch
    operations made, how many of them needed the full upload, and t's record count after every one of them"""
    out = {"edits": 0, "fallbacks": 0, "records": [], "own": []}

    def settle(result, batch_open=False):
        out["edits"] += 1
        if result is None:
            if batch_open:
                t.patch_end()
            t.upload_octree(*world.flatten())
            out["fallbacks"] += 1
        out["records"].append(int(t.scene_info()["n_records"]))
        out["own"].append(result is not None)            # a patch: whatever the record count did, the library did by itself
        return result is not None

    for op in ops:
        if op[0] == "voxel":
            apply_edit(world, vox, op[1], op[2], mirror)
            settle(t.patch_voxel(world, *op[1]))
        elif op[0] == "box":
            for xyz, m in op[3]:
                apply_edit(world, vox, xyz, m, mirror)
            settle(t.patch_box(world, op[1], op[2]))
        elif op[0] == "batch":
            t.patch_begin()
            is_open = True
            for _, xyz, m in op[1]:
                apply_edit(world, vox, xyz, m, mirror)
                is_open = settle(t.patch_voxel(world, *xyz), is_open) and is_open
            if is_open:
                t.patch_end()
        elif op[0] == "compact":
            t.compact()
            out["records"].append(int(t.scene_info()["n_records"]))
            out["own"].append(False)
        else:
            raise ValueError(op)
    return out


class NullTarget:
    """drive() on the world alone"""
    def patch_voxel(self, *a): return 1
    def patch_box(self, *a): return 1
    def patch_begin(self): pass
    def patch_end(self): pass
    def compact(self): pass
    def upload_octree(self, *a): pass
    def scene_info(self): return {"n_records": 0}


def edited_voxels(ops):
    out = []
    for op in ops:
        if op[0] == "voxel":
            out.append(tuple(op[1]))
        elif op[0] == "box":
            out += [tuple(xyz) for xyz, _ in op[3]]
        elif op[0] == "batch":
            out += [tuple(xyz) for _, xyz, _ in op[1]]
    return out


class Session:
    def __init__(self, V, O, family, index, seed=SEED, plan=None):
        self.V, self.O, self.family, self.index = V, O, family, index
        self.case = sw.case(V, O, family, index, seed=seed)
        self.world, self.vox = self.case.world, self.case.vox
        self.vox0 = dict(self.vox)                 # as the case drew them: self.vox follows the edits
        self.plan = plan or PLAN[(family, index % len(INDICES))]
        self.rng = np.random.default_rng([seed, FAMILIES.index(family), index, 0xED17])
        self.seed = seed
        c = self.case
        self.scale = c.uniforms["voxel_scale"]
        self.eye = np.asarray(c.cam[2][:3], np.float64) * F(self.scale)            # in voxel space, as the kernels scale it
        self.eye_cell = tuple(int(v) for v in np.floor(self.eye))
        lo, hi = (c.bounds or ((-1023,) * 3, (1024,) * 3))
        self.wlo, self.whi = np.asarray(lo), np.asarray(hi)
        self.dirs = oracle_rays.frame_rays(rays_lib(), c.scene(O), c.W, c.H)[1]
        # where the schedule samples emitters (or the plan holds an emitter item) the list changes by the plan's own items alone, so that
        # each change of it can be held to change the picture; elsewhere incidental edits take emissive voxels and materials too
        self.no_emit = self.case.setting["rule"] != "off" or any(it in EMITTER_ITEMS for g in self.plan for it in g)
        self.opaque = family == "opaque"
        self.state = {}
        self.flags = set()
        # the far family's floor is no part of the case's voxel dictionary; from 700 units it is most of what the pixels' rays meet
        floor = sw._draw_voxels(np.random.default_rng([seed, FAMILIES.index(family), index]), family, index % sw.N_INDEX)[3]
        self.floor = None
        if floor is not None:
            cells = np.asarray(floor[0])
            self.floor = dict(y=int(cells[0, 1]), lo=cells[:, [0, 2]].min(axis=0), hi=cells[:, [0, 2]].max(axis=0) + 1, gone=set())

    def close(self):
        self.case.close()

    # ---- what the items draw from ----
    def free(self, p):
        p = tuple(int(v) for v in p)
        if self.floor is not None and p[1] == self.floor["y"]:      # the floor's own layer: `visible` alone takes voxels out of it
            return False
        if self.no_emit and p in self.vox and sw.PALETTE[self.vox[p]][2] > 0:
            return False
        return p != self.eye_cell and all(self.wlo[k] <= p[k] < self.whi[k] for k in range(3))

    def materials(self, emissive_too=False):
        if self.opaque:
            pool = [sw.STONE, sw.GRASS, sw.AIR12]
        else:
            pool = [sw.STONE, sw.GRASS, sw.WATER, sw.GLASS, sw.AIR12, sw.GREEN_GLASS]
        if emissive_too and not self.no_emit:
            pool += [sw.LAMP, sw.EMBER, sw.BLACK] + ([] if self.opaque else [sw.GLOW_GLASS])
        return pool

    def material(self, emissive_too=False):
        pool = self.materials(emissive_too)
        return pool[int(self.rng.integers(0, len(pool)))]

    def _march(self, d, lo, hi):
        """the first occupied cell other than the eye's own along the ray eye + t d, by a cell walk over the voxel dictionary"""
        o = self.eye
        t0, t1 = 0.0, 1e30
        for k in range(3):
            if d[k] == 0.0:
                if not lo[k] <= o[k] < hi[k]:
                    return None
                continue
            a, b = (lo[k] - o[k]) / d[k], (hi[k] - o[k]) / d[k]
            t0, t1 = max(t0, min(a, b)), min(t1, max(a, b))
        if t0 >= t1:
            return None
        start = o + d * (t0 + 1e-4)
        p = [int(np.floor(v)) for v in start]
        step = [1 if v > 0 else -1 for v in d]
        inv = [abs(1.0 / v) if v != 0.0 else 1e30 for v in d]
        nxt = [t0 + ((p[k] + (1 if d[k] > 0 else 0)) - start[k]) / d[k] if d[k] != 0.0 else 1e30 for k in range(3)]
        t = t0
        while t < t1:
            q = (p[0], p[1], p[2])
            if q in self.vox and q != self.eye_cell:
                return q
            k = nxt.index(min(nxt))
            t = nxt[k]
            nxt[k] += inv[k]
            p[k] += step[k]
        return None

    def visible(self):
        """-> [(pixel, voxel)]: for the frame's rays that end in a voxel, the first one they meet from the eye (the eye's own cell
        looked through, so that an eye inside a voxel still sees), in a drawn order"""
        keys = np.array(list(self.vox))
        lo, hi = keys.min(axis=0).astype(float), (keys.max(axis=0) + 1).astype(float)
        found = []
        for px in range(0, len(self.dirs)):
            d = self.dirs[px].astype(np.float64)
            v = self._march(d, lo, hi)
            if v is None and self.floor is not None and d[1] < 0:     # the floor: one layer of cells, met from above
                q = self.eye + d * ((self.floor["y"] + 1 - self.eye[1]) / d[1])
                q = (int(np.floor(q[0])), self.floor["y"], int(np.floor(q[2])))
                if np.all(self.floor["lo"] <= (q[0], q[2])) and np.all((q[0], q[2]) < self.floor["hi"]) and q not in self.floor["gone"]:
                    v = q
            if v is not None and v not in self.vox:
                found.append((px, v))
            elif v is not None and not (self.no_emit and sw.PALETTE[self.vox[v]][2] > 0):
                found.append((px, v))
        if not found:      # from 700 units a pixel is some 30 voxels wide: what the eye sees between the pixels' own rays (pixel -1)
            keys = sorted(self.vox)
            for i in self.rng.permutation(len(keys))[:64]:
                d = np.asarray(keys[i]) + 0.5 - self.eye
                v = self._march(d / np.linalg.norm(d), lo, hi)
                if v is not None and not (self.no_emit and sw.PALETTE[self.vox[v]][2] > 0):
                    found.append((-1, v))
        assert found, f"{self.family} {self.index}: the eye sees no voxel"
        return [found[i] for i in self.rng.permutation(len(found))]

    def kept(self):
        """the voxels later items and checks count on: no incidental edit touches them"""
        return {tuple(self.state[k]) for k in ("lamp", "ray_glass", "black") if k in self.state}

    def beside(self, v):
        """an empty cell next to voxel v, towards the eye first"""
        order = sorted(range(6), key=lambda j: -((self.eye[j // 2] - v[j // 2] - 0.5) * (1 if j % 2 else -1)))
        for j in order:
            p = list(v)
            p[j // 2] += 1 if j % 2 else -1
            if tuple(p) not in self.vox and self.free(p):
                return tuple(p)
        return None

    # ---- the vocabulary: each item -> a list of operations, planned on the world as it stands ----
    def item_visible(self):
        """up to two voxels the frame shows removed, up to two inserted beside voxels it shows (from far away few rays end in
        different voxels: at least one of each)"""
        seen = self.visible()
        keep = self.kept()
        gone = []
        for _, v in seen:
            if len(gone) < 2 and v not in gone and v not in keep:
                gone.append(v)
        new = []
        for _, v in seen:
            p = self.beside(v)
            if len(new) < 2 and p is not None and p not in new:
                new.append(p)
        assert gone and new, (self.family, self.index, gone, new)
        if self.floor is not None:
            self.floor["gone"] |= {v for v in gone if v not in self.vox}
        return [("voxel", v, None) for v in gone] + [("voxel", p, self.material(emissive_too=True)) for p in new]

    def item_glass_on_ray(self):
        """a first translucent voxel on a pixel's ray between the eye and its hit"""
        for px, v in self.visible():
            d = self.dirs[px].astype(np.float64)
            dist = float(np.linalg.norm(np.asarray(v) + 0.5 - self.eye))
            for t in np.linspace(0.35, 0.75, 5) * dist:
                p = tuple(int(x) for x in np.floor(self.eye + d * t))
                if p not in self.vox and self.free(p) and p != v:
                    self.state["ray_glass"], self.state["ray_pixel"] = p, px
                    return [("voxel", p, RAY_GLASS.get((self.family, self.index % len(INDICES)), sw.GLASS))]
        raise AssertionError("no empty cell on a pixel's ray")

    def item_glass_off_ray(self):
        return [("voxel", self.state.pop("ray_glass"), None)]

    def _emissive_boxes(self):
        """every emissive voxel, as clearances of the 4^3 blocks that hold them"""
        blocks = {}
        for p, m in self.vox.items():
            if sw.PALETTE[m][2] > 0 and (sw.PALETTE[m][0] & 0xff) > 0:
                blocks.setdefault(tuple(v >> 2 for v in p), []).append(p)
        ops = []
        for key in sorted(blocks):
            cells = sorted(blocks[key])
            lo, hi = np.min(cells, axis=0), np.max(cells, axis=0)
            if len(cells) == 1:
                ops.append(("voxel", cells[0], None))
            else:
                ops.append(("box", tuple(lo.tolist()), tuple(hi.tolist()), [(c, None) for c in cells]))
        return ops

    def item_strip_emitters(self):
        return self._emissive_boxes()

    def item_emit_clear(self):
        ops = self._emissive_boxes()
        assert ops
        return ops

    def item_emit_gain(self):
        """a LAMP single at the corner of an empty aligned 2^3 block beside something the frame shows"""
        for _, v in self.visible():
            for dy in (1, 2, 3, 0):
                for dx, dz in ((0, 0), (2, 0), (-2, 0), (0, 2), (0, -2)):
                    c = tuple((a + b) & ~1 for a, b in zip(v, (dx, dy + 1, dz)))
                    cells = [(c[0] + i, c[1] + j, c[2] + k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
                    if all(p not in self.vox and self.free(p) for p in cells):
                        self.state["lamp"] = c
                        return [("voxel", c, sw.LAMP)]
        raise AssertionError("no free 2^3 block")

    def item_emit_merge(self):
        c = self.state["lamp"]
        cells = [(c[0] + i, c[1] + j, c[2] + k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
        assert self.vox.get(c) == sw.LAMP and all(p not in self.vox for p in cells[1:])
        return [("box", c, cells[-1], [(p, sw.LAMP) for p in cells[1:]])]

    def item_emit_split(self):
        c, size = self.case.cubes[0]
        assert size == 4
        p = self.eye_cell
        while p == self.eye_cell:
            p = tuple(int(a + b) for a, b in zip(c, self.rng.integers(0, 4, size=3)))
        return [("voxel", p, None)]

    def item_emit_black(self):
        for _, v in self.visible():
            p = self.beside(v)
            if p is not None:
                self.state["black"] = p
                return [("voxel", p, sw.BLACK)]
        raise AssertionError("no place for the black emitter")

    def item_eye_in(self):
        assert self.eye_cell not in self.vox
        return [("voxel", self.eye_cell, EYE_KIND.get((self.family, self.index % len(INDICES)), sw.GLASS))]

    def item_eye_out(self):
        assert self.eye_cell in self.vox
        return [("voxel", self.eye_cell, None)]

    def item_eye_remove(self):
        assert self.eye_cell in self.vox, "the inside family's eye is in a voxel"
        return [("voxel", self.eye_cell, None)]

    def _box_near(self, side):
        """a box of this side around a voxel of the dictionary that the eye sees (the far family's floor is not one), else a drawn one"""
        seen = [v for _, v in self.visible() if v in self.vox and v not in self.kept()]
        keys = sorted(self.vox)
        v = seen[0] if seen else keys[int(self.rng.integers(0, len(keys)))]
        lo = np.asarray(v) - self.rng.integers(0, side, size=3)
        lo = np.clip(lo, self.wlo, self.whi - side)
        return lo, lo + side - 1

    def _cells(self, lo, hi):
        g = [np.arange(lo[k], hi[k] + 1) for k in range(3)]
        return [tuple(int(v) for v in p) for p in np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3) if self.free(p)]

    def _fill(self, lo, hi, m, share):
        cells = [(p, m) for p in self._cells(lo, hi) if self.rng.random() < share and p not in self.kept()]
        assert cells
        return [("box", tuple(int(v) for v in lo), tuple(int(v) for v in hi), cells)]

    def item_box_fill(self):
        """a ragged fill: seven cells in ten of a box of one material"""
        lo, hi = self._box_near(int(self.rng.integers(3, 7)))
        return self._fill(lo, hi, self.material(), 0.7)

    def item_box_clear(self):
        lo, hi = self._box_near(int(self.rng.integers(3, 7)))
        keep = self.kept()
        cells = [(p, None) for p in self._cells(lo, hi) if p in self.vox and p not in keep]
        assert cells
        return [("box", tuple(int(v) for v in lo), tuple(int(v) for v in hi), cells)]

    def item_box_glass(self):
        lo, hi = self._box_near(int(self.rng.integers(2, 5)))
        return self._fill(lo, hi, sw.GLASS, 1.1)

    def item_box_anchor(self):
        """a box across a plane x = 64 n, an anchor of the wide layout, beside the content"""
        _, v = self.visible()[0]
        x0 = int(round(v[0] / 64.0)) * 64
        x0 = min(max(x0, int(self.wlo[0]) + 64), int(self.whi[0]) - 64)
        lo = np.array([x0 - 2, v[1] + 1, v[2]])
        hi = lo + np.array([3, int(self.rng.integers(1, 3)), int(self.rng.integers(1, 3))])
        self.flags.add("anchor")
        assert lo[0] < x0 <= hi[0] and x0 % 64 == 0
        return self._fill(lo, hi, sw.STONE if self.opaque else self.material(), 0.8)

    def item_box_negative(self):
        """a box in negative coordinates: outside the octant of wide root 0"""
        lo = -np.asarray(self.rng.integers(4, 30, size=3)) - 4
        hi = lo + np.asarray(self.rng.integers(1, 4, size=3))
        assert np.all(hi < 0) and np.all(lo >= self.wlo)
        return self._fill(lo, hi, self.material(), 0.8)

    def item_stroke(self):
        """a brush stroke: 8 to 12 voxel edits in one batch, walking on from something the frame shows"""
        _, p = self.visible()[0]
        p = np.asarray(p)
        n = int(self.rng.integers(8, 13))
        ops, seen = [], set()
        keep = self.kept()
        while len(ops) < n:
            p = np.clip(p + self.rng.integers(-1, 2, size=3), self.wlo, self.whi - 1)
            q = tuple(int(v) for v in p)
            if q in seen or not self.free(q) or q in keep or (self.no_emit and q in self.vox and sw.PALETTE[self.vox[q]][2] > 0):
                continue
            seen.add(q)
            ops.append(("voxel", q, None if q in self.vox else self.material()))
        return [("batch", ops)]

    def item_compact_last(self):
        return [("compact",)]

    item_compact_mid = item_compact_last

    def item_highlight_replace(self):
        h = tuple(self.case.uniforms["highlighted"])
        assert h in self.vox
        pool = [m for m in self.materials() if m != self.vox[h]]
        return [("voxel", h, pool[int(self.rng.integers(0, len(pool)))])]

    def item_highlight_remove(self):
        h = tuple(self.case.uniforms["highlighted"])
        assert h in self.vox
        return [("voxel", h, None)]

    def item_long_run(self):
        """LONG_EDITS single-voxel edits in a LONG_SIDE^3 region around something the frame shows: cells toggled"""
        _, v = self.visible()[0]
        lo = np.clip(np.asarray(v) - LONG_SIDE // 2, self.wlo, self.whi - LONG_SIDE)
        ops, state = [], dict(self.vox)
        while len(ops) < LONG_EDITS:
            q = tuple(int(a) for a in lo + self.rng.integers(0, LONG_SIDE, size=3))
            if not self.free(q) or (q in state and sw.PALETTE[state[q]][2] > 0):
                continue
            m = None if q in state else self.material()
            ops.append(("voxel", q, m))
            if m is None:
                del state[q]
            else:
                state[q] = m
        return ops

    # ---- the session ----
    def item(self, name):
        """the operations of one item, planned on the world as it stands now: drive() them before the next call"""
        return getattr(self, "item_" + name)()

    def checkpoint(self, k, ops):
        c = self.case
        cp = copy.copy(c)
        cp.__class__ = Checkpoint
        cp.k, cp.ops, cp.edited = k, ops, edited_voxels(ops)
        cp.vox = dict(self.vox)
        cp.tex, cp.dim = self.world.flatten()
        cp.records = self.world.records()[0]
        cp.list, cp.words = oep.walk(cp.records, *(c.bounds or ()))
        cp.weights = np.array(oep.weights(cp.list, cp.words), np.uint64)
        cp.eye_cell = self.eye_cell
        keys = sorted(cp.vox)
        rng = np.random.default_rng([self.seed, FAMILIES.index(self.family), self.index, 0xED17, k])
        lo, hi = np.min(keys, axis=0), np.max(keys, axis=0) + 1
        glass = [p for p in keys if (sw.PALETTE[cp.vox[p]][0] & 0xff) not in (0, 255)] or keys
        solid = [p for p in keys if (sw.PALETTE[cp.vox[p]][0] & 0xff) == 255]
        g, s = glass[int(rng.integers(0, len(glass)))], solid[int(rng.integers(0, len(solid)))]
        o, d = _ray_mix(rng, sw.N_RAYS, lo, hi, (g, tuple(v + 1 for v in g)), (s, tuple(v + 1 for v in s)))
        cp.rays = ((o / F(self.scale)).astype(F), d)
        cp.outside_pose = None
        return cp


def draw_plan(rng, family, index):
    """a plan of a drawn length for fuzz/fuzz_edits.py: two to five groups out of the items that need nothing before them, with the
    paired ones (the eye's cell, the glass on a ray, the emitter chain) laid over them in their order"""
    n = int(rng.integers(2, 6))
    pool = ["box_fill", "box_clear", "stroke", "compact_mid", "box_anchor"] + ([] if family == "opaque" else ["box_glass"])
    if not (family == "far" and index % sw.N_INDEX in (1, 2)):        # custom bounds: the negative octants are outside the world, or small
        pool.append("box_negative")
    groups = [["visible"] + [pool[int(j)] for j in rng.choice(len(pool), size=int(rng.integers(1, 4)), replace=False)] for _ in range(n)]
    a, b = sorted(int(v) for v in rng.choice(n, size=2, replace=False))
    if family == "inside":
        if sw.INSIDE_KINDS[index % sw.N_INDEX] != "cube":
            groups[a].insert(0, "eye_remove")
    elif family == "opaque":
        groups[a].insert(0, "glass_on_ray")
        groups[b].insert(0, "glass_off_ray")
        groups[0][0:0] = ["strip_emitters", "emit_gain"]
        groups[1].insert(0, "emit_merge")
    else:
        groups[a].insert(0, "eye_in")
        groups[b].insert(0, "eye_out")
        chain = ["emit_split", "emit_clear", "emit_black"][:n]
        for k, item in enumerate(chain):
            groups[k].insert(0, item)
    return tuple(tuple(g) for g in groups)


class Mirror:
    """the oracle's pointer tree of a session's world, edited in step with it (what o_octree_ray_cast and o_octree_find walk)"""

    def __init__(self, O, S):
        self.O, self.L = O, O.lib()
        lo, hi = (S.case.bounds or ((-1023,) * 3, (1024,) * 3))
        self.tree = self.L.o_octree_create(None, O.IVec3(*lo), O.IVec3(*hi))
        floor = sw._draw_voxels(np.random.default_rng([S.seed, FAMILIES.index(S.family), S.index]), S.family, S.index % sw.N_INDEX)[3]
        if floor is not None:                            # sample_sweep_worlds._build_world's order
            for p in floor[0].tolist():
                self.insert(p, floor[1])
        for m in range(len(sw.PALETTE)):
            for p, mm in S.vox0.items():
                if mm == m:
                    self.insert(p, m)

    def insert(self, p, m):
        c, refr, illum, k = sw.PALETTE[m]
        self.L.o_octree_insert(self.tree, self.O.VoxelObj(self.O.IVec3(*[int(v) for v in p]), c, self.O.Voxel(refr, illum, k)))

    def __call__(self, xyz, m, replaces):
        if m is None or replaces:
            self.L.o_octree_remove(self.tree, self.O.IVec3(*[int(v) for v in xyz]))
        if m is not None:
            self.insert(xyz, m)

    def close(self):
        self.L.o_octree_delete(self.tree)


# ---- the batch that voids the wide layout: hand-written streams -------------------------------------------------------------------
# World edits never void the wide layout (the docstring above), but vrt_patch_apply takes the caller's sub-tree: in the world [0, 8)^3
# of test_gpu_parity's unit-internal stream, one batch replaces the node [4, 8)^3 -- a wide root -- by a sub-tree whose unit cell
# [4, 5)^3 is an internal node (build_wide_node refuses it: PatchRanges::wide_invalid), and goes on with two more patches, which
# patch_host() then plans and applies on the records alone. VOID_STEPS: (voxel that plans the patch, the path it must find, the tree
# whose sub-tree it applies and which the structures must equal afterwards).
VOID_BOUNDS = ((0, 0, 0), (8, 8, 8))
VOID_DIM = 3
LEAF = "leaf"
VOID_START = {0: LEAF, 7: {0: LEAF}}                                     # test_gpu_parity's `regular`
VOID_STEPS = (((4, 4, 4), [7], {0: LEAF, 7: {0: {0: {7: LEAF}}}}),       # [4, 5)^3 internal: the wide layout is void from here on
              ((6, 6, 6), [7], {0: LEAF, 7: {0: {0: {7: LEAF}}, 7: LEAF}}),
              ((4, 4, 4), [7, 0, 0], {0: LEAF, 7: {0: {0: {0: LEAF, 7: LEAF}}, 7: LEAF}}))


def hand_stream(tree):
    """a texel stream written by hand from {child index: sub-tree or LEAF}: per node a header (first pointer, child mask), one
    pointer per child (bit 23: a leaf), then the children; every leaf the parity test's opaque pink -> uint8 array"""
    out = []

    def tx(value, alpha):
        return [value & 255, (value >> 8) & 255, (value >> 16) & 255, alpha]

    def emit(node):
        at, kids = len(out), sorted(node)
        out.append(None)
        ptr = len(out)
        out.extend([None] * len(kids))
        out[at] = tx(ptr, sum(1 << k for k in kids))
        for j, k in enumerate(kids):
            if node[k] == LEAF:
                out[ptr + j] = tx(len(out) | 0x800000, 0)
                out.extend([[200, 40, 90, 255], [255, 0, 0, 255]])
            else:
                out[ptr + j] = tx(emit(node[k]), 0)
        return at

    emit(tree)
    return np.array(out, np.uint8).reshape(-1)


def session(V, O, family, index, seed=SEED, plan=None):
    return Session(V, O, family, index, seed=seed, plan=plan)


def run(V, O, family, index, target=None, at_checkpoint=None, before_group=None, seed=SEED, plan=None, mirror=None):
    """the whole session on one target (an object, or a function of the Session that makes one) -> (Session, [(ops, counts,
    checkpoint)]), counts drive()'s summed over the group. Item by item: each is planned on the world the one before it left.
    before_group(S, k, t) runs before group k and at_checkpoint(S, cp, counts, t) after it, while the world stands as cp describes it"""
    S = session(V, O, family, index, seed=seed, plan=plan)
    out = []
    try:
        t = target(S) if callable(target) else (target or NullTarget())
        for k in range(len(S.plan)):
            if before_group:
                before_group(S, k, t)
            ops, counts = [], {"edits": 0, "fallbacks": 0, "records": [], "own": []}
            for name in S.plan[k]:
                part = S.item(name)
                got = drive(t, S.world, S.vox, part, mirror)
                ops += part
                counts["edits"] += got["edits"]
                counts["fallbacks"] += got["fallbacks"]
                counts["records"] += got["records"]
                counts["own"] += got["own"]
            cp = S.checkpoint(k + 1, ops)
            if at_checkpoint:
                at_checkpoint(S, cp, counts, t)
            out.append((ops, counts, cp))
    except BaseException:
        S.close()
        raise
    return S, out
