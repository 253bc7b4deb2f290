"""The world of the emitter-MIS tests (test_emit_mis.py, test_gpu_emit_mis.py) -- TEST INFRASTRUCTURE ONLY: emit_worlds.py's lamp room
without its lamp and singles, and with emitters that touch surfaces, which is where the power rule's connection weight is unbounded:
a merged lamp of size 2 standing on the floor at an even corner, three single emitters with different illumination bytes against a
wall, the ceiling and another wall, and one black emitter (colour 0, illumination > 0) on the floor. The "near" rays run from EYE to
surface points 0.15 to 1.5 voxels from the foot of the lamp and beside a single; the "far" rays are emit_worlds.probe_rays()."""
import numpy as np

import emit_worlds as ew

W, H = ew.W, ew.H
FLOOR_Y = ew.LO + 1                                    # the floor's upper face, where the lamp stands
LAMP = ((46, FLOOR_Y, 48), 0xffe0a0ff, 2)              # the eight voxels lo .. lo + 1: one leaf of size 2 in the host tree
SINGLES = (((32, 40, 44), 0xa0c0ffff, 255),            # against the wall x = LO
           ((50, 55, 36), 0xffc0a0ff, 128),            # under the ceiling
           ((44, 45, 32), 0xa0ffc0ff, 64))             # against the wall z = LO: position, colour, illumination byte
BLACK = ((52, FLOOR_Y, 36), 0x000000ff, 200)           # W_j == 0: the bounce ray alone carries what the shader gives it
SPARE = ((34, 55, 34), 0xa0ffc0ff, 90)                 # the single emitter a patch adds (test_gpu_emit_mis.py)
EYE, POSE, LENS = ew.EYE, ew.POSE, ew.LENS
INSIDE_POSE = (36.5, 44.5, 50.5, -20.0, -35.0)         # towards the foot of the lamp (tools/accum_rate.py mis_room_1080p, tools/shade_rays_rate.py --emit-world mis_room)
N_EMITTERS = 5
NEAR = (0.15, 0.3, 0.6, 1.5)


def room(V, pane=True):
    w = ew.lamp_room(V, pane=pane, singles=False, lamp=False)
    (lx, ly, lz), c, size = LAMP
    assert lx % 2 == 0 and ly % 2 == 0 and lz % 2 == 0 and size == 2
    for dx in range(size):
        for dy in range(size):
            for dz in range(size):
                w.insert(lx + dx, ly + dy, lz + dz, c, 3.0, 1.0, 0.0)
    for (sx, sy, sz), c, illum in SINGLES + (BLACK,):
        w.insert(sx, sy, sz, c, 3.0, illum / 255.0, 0.0)
    return w


def expected_list():
    return sorted([list(LAMP[0]) + [LAMP[2]]] + [list(p) + [1] for p, _, _ in SINGLES + (BLACK,)])


def near_points():
    """surface points next to emitters: on the floor at NEAR voxels from the lamp's foot on its -x and +z sides (the two EYE sees), on
    the wall x = LO beside and above the first single, and on the ceiling beside the second"""
    (lx, _, lz), _, size = LAMP
    pts = []
    for d in NEAR:
        pts.append((lx - d, FLOOR_Y, lz + 0.9))
        pts.append((lx + 1.1, FLOOR_Y, lz + size + d))
    (sx, sy, sz), _, _ = SINGLES[0]
    pts += [(sx, sy + 0.5, sz + 1.15), (sx, sy + 0.4, sz + 1.5), (sx, sy + 1.3, sz + 0.5)]
    (cx, cy, cz), _, _ = SINGLES[1]
    pts.append((cx + 1.3, cy + 1, cz + 0.5))
    return np.array(pts, np.float32)


def near_rays():
    """-> (origin float32[3], dirs float32[n, 3]): from EYE to near_points(), not normalised"""
    o = np.array(EYE, np.float32)
    return o, (near_points() - o).astype(np.float32)


far_rays = ew.probe_rays


def all_rays():
    """near then far -> (origin, dirs, number of near rays)"""
    o, dn = near_rays()
    _, df = far_rays()
    return o, np.concatenate([dn, df]).astype(np.float32), len(dn)
