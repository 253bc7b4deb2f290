"""Which launch geometry a frame gives the guided filter's level kernels -- TEST INFRASTRUCTURE ONLY, pure Python.

The lattice form (csrc/vrt_filter.hip.h filter_level_lattice_kernel) serves the levels of step s <= kLatticeMaxStep. Along one axis of
n pixels with a tile of T lanes, residue class r (the pixels r, r + s, r + 2 s, ...) has c_r = ceil((n - r) / s) pixels and
t_r = ceil(c_r / T) tiles; the launch gives every class class 0's t_0 workgroups (csrc/vrt_launch_filter.hip). Per step and axis a
launch contains any of four events:
  interior      a class with at least 3 tiles: a tile whose window is staged from inside the image on both sides
  ragged        a class whose last tile is not full: lanes leave at `x >= l.width`
  early_return  a class that has pixels and fewer tiles than class 0: its last workgroup leaves whole, before it stages anything
                (steps >= 2 only: step 1 has one class). A frame narrower than the step has classes without any pixel, whose
                workgroups leave the same way; that is counted in "returns" and is not this event: no seam lies beside it
  exact         every class's pixels fill its tiles: no lane of the launch is past the edge
and each step runs one <FIRST, LAST> form. constants() reads the tile from the compiled test library (vrt_test_filter_geometry), so
a retuned tile changes what the model says about the committed shapes; SEAM_SHAPES and SEAM_LEVELS are those shapes, shared by
tests/test_filter_geometry.py (the model, no device) and tests/test_gpu_filter_seams.py (the device against the checkers)."""
import ctypes as C

NAMES = ("kBlockX", "kBlockY", "kVarX", "kVarY", "kLatX", "kLatY", "kLatticeMaxStep")
EVENTS = ("interior", "ragged", "early_return", "exact")

# (W, H), derived from the 32 s x 8 s pixels a tile covers at step s:
#   257 x 33   x: 9 tiles at step 1; 5 | 4 per class at step 2; 3 | 2 | 2 | 2 at step 4.  y: 5; 3 | 2; 2 | 1 | 1 | 1
#   33 x 257   the same with the axes exchanged (y: 33 tiles; 17 | 16; 9 | 8 | 8 | 8)
#   256 x 32   an exact fit at every step in both axes
#   131 x 35   2 | 2 | 2 | 1 at step 4 in both axes: the LAST class is the short one
SEAM_SHAPES = ((257, 33), (33, 257), (256, 32), (131, 35))
SEAM_LEVELS = (2, 3, 4)


def constants(V):
    """the seven constants as the compiled test library has them -> {name: int}"""
    T = V.test_lib()
    T.vrt_test_filter_geometry.argtypes = [C.c_void_p]
    T.vrt_test_filter_geometry.restype = None
    out = (C.c_int32 * len(NAMES))()
    T.vrt_test_filter_geometry(out)
    return dict(zip(NAMES, (int(v) for v in out)))


def _ceil_div(a, b):
    return (a + b - 1) // b


def class_tiles(n, s, tile):
    """tiles per residue class 0 .. s - 1 along an axis of n pixels"""
    return [_ceil_div(_ceil_div(n - r, s), tile) if r < n else 0 for r in range(s)]


def axis_events(n, s, tile):
    """the events of one axis of one lattice launch -> a set of EVENTS"""
    pixels = [_ceil_div(n - r, s) if r < n else 0 for r in range(s)]
    tiles = [_ceil_div(c, tile) for c in pixels]
    ev = set()
    if max(tiles) >= 3:
        ev.add("interior")
    if any(c % tile for c in pixels):
        ev.add("ragged")
    if any(0 < t < tiles[0] for t in tiles):
        ev.add("early_return")
    if all(c > 0 and c % tile == 0 for c in pixels):
        ev.add("exact")
    return ev


def grid(k, width, height, s):
    """the lattice launch's grid as csrc/vrt_launch_filter.hip computes it -> (x, y) workgroups"""
    return (_ceil_div(_ceil_div(width, s), k["kLatX"]) * s, _ceil_div(_ceil_div(height, s), k["kLatY"]) * s)


def levels_of(k, width, height, levels):
    """one entry per level: {"step", "lattice", "first", "last"} and, for a lattice level, "x" and "y" (sets of EVENTS), "grid" and
    "returns" (the workgroups that take the early return)"""
    out = []
    for i in range(levels):
        s = 1 << i
        e = {"step": s, "lattice": s <= k["kLatticeMaxStep"], "first": i == 0, "last": i == levels - 1}
        if e["lattice"]:
            e["x"], e["y"] = axis_events(width, s, k["kLatX"]), axis_events(height, s, k["kLatY"])
            tx, ty = class_tiles(width, s, k["kLatX"]), class_tiles(height, s, k["kLatY"])
            e["grid"] = grid(k, width, height, s)
            assert e["grid"] == (tx[0] * s, ty[0] * s)
            e["returns"] = e["grid"][0] * e["grid"][1] - sum(tx) * sum(ty)
        out.append(e)
    return out


def lattice_steps(k):
    s, out = 1, []
    while s <= k["kLatticeMaxStep"]:
        out.append(s)
        s *= 2
    return out


def coverage(k, shapes, level_counts):
    """what the launches of every shape at every level count contain -> ({(step, axis, event)}, {(step, first, last)}), lattice levels only"""
    events, forms = set(), set()
    for w, h in shapes:
        for levels in level_counts:
            for e in levels_of(k, w, h, levels):
                if not e["lattice"]:
                    continue
                forms.add((e["step"], e["first"], e["last"]))
                for axis in ("x", "y"):
                    events.update((e["step"], axis, ev) for ev in e[axis])
    return events, forms


def required(k):
    """what a seam shape list must contain: every event at every lattice step in both axes (the early return from step 2: step 1 has one
    class), and both forms a level after the first can take -- middle and last -- at every lattice step above 1"""
    events = {(s, axis, ev) for s in lattice_steps(k) for axis in ("x", "y") for ev in EVENTS if not (s == 1 and ev == "early_return")}
    forms = {(s, False, last) for s in lattice_steps(k) if s > 1 for last in (False, True)}
    return events, forms


def missing(k, shapes, level_counts):
    have_e, have_f = coverage(k, shapes, level_counts)
    need_e, need_f = required(k)
    return sorted(need_e - have_e), sorted(need_f - have_f)
