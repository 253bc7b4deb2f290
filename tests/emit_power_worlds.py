"""The world of the emitter-importance tests (test_emit_power.py, test_gpu_emit_power.py) -- TEST INFRASTRUCTURE ONLY: emit_worlds.py's
lamp room with a merged lamp of size 4 in place of its size-2 one, and, in place of its three singles, a 16 x 16 panel of dim single
emitters under the ceiling whose illumination byte and colour vary from voxel to voxel, so that none merge: 257 emitters, one of which
holds most of the power."""
import numpy as np

import emit_worlds as ew

W, H = ew.W, ew.H
LAMP = ((44, 48, 44), 0xffe0a0ff, 4)      # the 64 voxels lo .. lo + 3: one leaf of size 4 in the host tree
PANEL_Y, PANEL = 55, (36, 52)             # y = 55, x and z in [36, 52)
SPARE = ((34, 55, 34), 0xa0ffc0ff, 9)     # the single emitter a patch adds (test_gpu_emit_power.py): position, colour, illumination byte
EYE, POSE, LENS = ew.EYE, ew.POSE, ew.LENS
N_EMITTERS = 257


def panel_voxel(i, k):
    """colour 0xRRGGBBAA and illumination byte of the panel's voxel (PANEL[0] + i, PANEL_Y, PANEL[0] + k)"""
    return ((0x40 + 8 * i) << 24) | ((0x40 + 8 * k) << 16) | (0x80 << 8) | 0xff, 4 + (7 * i + 3 * k) % 29


def room(V, pane=True):
    w = ew.lamp_room(V, pane=pane, singles=False, lamp=False)
    (lx, ly, lz), c, size = LAMP
    for dx in range(size):
        for dy in range(size):
            for dz in range(size):
                w.insert(lx + dx, ly + dy, lz + dz, c, 3.0, 1.0, 0.0)
    for i in range(PANEL[1] - PANEL[0]):
        for k in range(PANEL[1] - PANEL[0]):
            c, illum = panel_voxel(i, k)
            w.insert(PANEL[0] + i, PANEL_Y, PANEL[0] + k, c, 3.0, illum / 255.0, 0.0)
    return w


def expected_list():
    (lx, ly, lz), _, size = LAMP
    return sorted([[lx, ly, lz, size]] + [[PANEL[0] + i, PANEL_Y, PANEL[0] + k, 1] for i in range(16) for k in range(16)])


probe_rays = ew.probe_rays
