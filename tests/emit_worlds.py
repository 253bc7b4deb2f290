"""The worlds of the emitter-sampling tests (test_emitters.py, test_gpu_emitters.py) -- TEST INFRASTRUCTURE ONLY: the lamp room, a
closed room lit by one merged lamp and three single emitters under the ceiling, with a table and a pane of glass in front of the camera; and the dragon,
which has no emitter."""
import numpy as np

W, H = 72, 44   # nine tiles across and a half tile at the bottom edge
LO, HI = 31, 56                       # the shell: every voxel of [LO, HI]^3 with a coordinate equal to LO or HI
WALL = 0xc0c0c0ff
LAMP = ((44, 48, 44), 0xffe0a0ff)     # the eight voxels lo .. lo + 1: one leaf of size 2 in the host tree
SINGLES = (((36, 55, 38), 0xa0c0ffff), ((50, 55, 36), 0xa0c0ffff), ((39, 55, 51), 0xa0c0ffff))   # under the ceiling
SPARE = ((52, 55, 50), 0xa0ffc0ff)    # the single emitter a patch adds (test_gpu_emitters.py)
TABLE_Y, TABLE = 40, (40, 46)         # y = 40, x and z in [40, 46)
PANE_X, PANE_Y, PANE_Z = 40, (42, 52), (41, 52)   # one translucent voxel thick, between the camera and the lamp
GLASS = (0xc8dcff50, 1.5)             # colour (alpha 0x50), refraction
EYE = (36.5, 44.5, 50.5)              # the probe rays' origin and the camera
POSE = EYE + (-38.0, 8.0)             # yaw, pitch: towards the lamp, through the pane
LENS = (0.7, 30.0)                    # aperture, focus distance
DRAGON_POSE = (63.5, 60.5, 140.5, -90.0, -10.0)


def lamp_room(V, pane=True, singles=True, lamp=True, lamp_alpha=0xff):
    """-> V.World. lamp_alpha 0: the lamp's voxels keep their illumination and lose their alpha (no emitter: the shader's emission is
    gated by alpha)"""
    w = V.World()
    r = np.arange(LO, HI + 1)
    x, y, z = np.meshgrid(r, r, r, indexing="ij")
    on = (x == LO) | (x == HI) | (y == LO) | (y == HI) | (z == LO) | (z == HI)
    shell = np.stack([x[on], y[on], z[on]], axis=1)
    w.insert_many(shell, np.full(len(shell), WALL, np.uint32), 3.0, 0.0, 0.0)
    for tx in range(*TABLE):
        for tz in range(*TABLE):
            w.insert(tx, TABLE_Y, tz, 0x805030ff, 3.0, 0.0, 0.0)
    if lamp:
        (lx, ly, lz), c = LAMP
        for dx in range(2):
            for dy in range(2):
                for dz in range(2):
                    w.insert(lx + dx, ly + dy, lz + dz, (c & 0xffffff00) | lamp_alpha, 3.0, 1.0, 0.0)
    if singles:
        for (sx, sy, sz), c in SINGLES:
            w.insert(sx, sy, sz, c, 3.0, 1.0, 0.0)
    if pane:
        for py in range(*PANE_Y):
            for pz in range(*PANE_Z):
                w.insert(PANE_X, py, pz, GLASS[0], GLASS[1], 0.0, 0.0)
    return w


def lamp_list(boxes=1):
    """the lamp alone as an emitter list: one entry of size 2, or its eight unit cells"""
    (lx, ly, lz), _ = LAMP
    if boxes == 1:
        return np.array([[lx, ly, lz, 2]], np.int32)
    return np.array(sorted((lx + dx, ly + dy, lz + dz, 1) for dx in range(2) for dy in range(2) for dz in range(2)), np.int32)


def probe_rays():
    """16 rays from EYE: np.random.default_rng(1).normal(size=(16, 3)) as float32, direction 0 set to (0.6, 0.35, -0.5), which sees
    the lamp"""
    d = np.random.default_rng(1).normal(size=(16, 3)).astype(np.float32)
    d[0] = (0.6, 0.35, -0.5)
    return np.array(EYE, np.float32), d
