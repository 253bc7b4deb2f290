"""Hand-built worlds of the past-glass guide tests (test_guides_glass.py, test_gpu_guides_glass.py) -- TEST INFRASTRUCTURE ONLY: each
with the rays that go with it and what rule G0-G6 of include/vrt.h must give for them in closed form."""
import numpy as np

OPAQUE, OPAQUE_BYTES = 0xC08040FF, (0xC0, 0x80, 0x40)       # R, G, B = 192, 128, 64, alpha 255
GLASS, GLASS_REFR, GLASS_ALPHA = 0x80C0FF80, 1.5, 0x80      # R, G, B, A = 128, 192, 255, 128
GLASS_REFR_STORED = 127 * 3.0 / 255.0                       # the leaf keeps refraction 1.5 as the byte 127: 1.494
GLASS_BYTES = (0x80, 0xC0, 0xFF, 0x80)
EYE = (2.5, 10.5, 10.5)


def slab(x0, x1, y0, y1, z0, z1, c=OPAQUE, r=3.0):
    return [(x, y, z, c, r, 0.0) for x in range(x0, x1) for y in range(y0, y1) for z in range(z0, z1)]


def build(V, voxels):
    """voxels: (x, y, z, rgba, refraction, illumination) -> (texels, tex_dim)"""
    w = V.World()
    for x, y, z, c, r, i in voxels:
        w.insert(int(x), int(y), int(z), int(c), float(r), float(i), 0.0)
    out = w.flatten()
    w.close()
    return out


EYE_BACK = (18.5, 10.5, 10.5)


def pane_wall(back=False):
    """a pane one voxel thick at x = 10 and a wall at x = 14, seen along +x from EYE: three surfaces, the wall 11.5 away; back: the
    wall at x = 6 instead, seen along -x from EYE_BACK, 11.5 away too"""
    return slab(10, 11, 5, 16, 5, 16, c=GLASS, r=GLASS_REFR) + (slab(6, 7, 5, 16, 5, 16) if back else slab(14, 15, 5, 16, 5, 16))


def pane_sky():
    return slab(10, 11, 5, 16, 5, 16, c=GLASS, r=GLASS_REFR)


# The reference's room (conftest.room_world) from close to its glass wall x = 51, towards the stone block behind it: nearly every
# pixel sees stone through the pane, at up to 40 degrees off the wall's normal. (From guide_worlds' pose inside the room 44 % of the
# through-glass pixels see sky behind the wall and 23 % end on the jelly cube's glass: too few end on an opaque surface.)
ROOM_THROUGH_WALL = (44.5, 27.5, 36.5, 15.0, 0.0)


# ---- an oblique ray through a slab four voxels thick ----------------------------------------------------------------------------
SLAB_X, SLAB_T, SLAB_WALL_X = 10, 4, 21
SLAB_EYE = (2.5, 10.5, 10.0)
SLAB_DIR = (1.0, 0.004, 1.0)       # 45 degrees to the slab's normal, un-normalised; no zero component (axis_rays())


def oblique_slab():
    return slab(SLAB_X, SLAB_X + SLAB_T, 8, 13, 5, 36, c=GLASS, r=GLASS_REFR) + slab(SLAB_WALL_X, SLAB_WALL_X + 1, 8, 13, 5, 40)


def oblique_slab_closed_form():
    """-> (z of the wall cell by Snell's lateral shift, z of the straight line's cell, the bent path's length, the straight distance
    from the eye to the final point), float64"""
    ti = np.arctan2(SLAB_DIR[2], SLAB_DIR[0])
    tt = np.arcsin(np.sin(ti) / GLASS_REFR_STORED)
    shift = SLAB_T * np.sin(ti - tt) / np.cos(tt)              # perpendicular distance between the ray's line and the line it leaves on
    run = SLAB_WALL_X - SLAB_EYE[0]
    z_straight = SLAB_EYE[2] + run * np.tan(ti)
    z_bent = z_straight - shift / np.cos(ti)                   # the shift measured along the wall
    bent = (run - SLAB_T) / np.cos(ti) + SLAB_T / np.cos(tt)
    straight = np.hypot(run, z_bent - SLAB_EYE[2])
    return z_bent, z_straight, bent, straight


# ---- total internal reflection: a ray that starts inside glass ---------------------------------------------------------------------
TIR_EYE = (2.5, 4.5, 4.0)
TIR_DIR = (0.5, 0.01, 0.8660254)   # 60 degrees to the +x face's normal; the critical angle of 1.5 is 41.8 degrees


def tir_block():
    """glass in [0, 8) x [0, 8) x [0, 30): the ray from TIR_EYE along TIR_DIR meets the face x = 8 at z = 13.53"""
    return slab(0, 8, 0, 8, 0, 30, c=GLASS, r=GLASS_REFR)


# ---- ten panes with air gaps -----------------------------------------------------------------------------------------------
PANES_X = tuple(range(10, 30, 2))


def ten_panes():
    """panes at x = 10, 12, .., 28, a wall at x = 32: along +x the eighth surface is the far side of the fourth pane, x = 17"""
    v = []
    for x in PANES_X:
        v += slab(x, x + 1, 8, 13, 8, 13, c=GLASS, r=GLASS_REFR)
    return v + slab(32, 33, 8, 13, 8, 13)


def axis_rays(n=5, back=False):
    """n rays from EYE along +x, the first 1e-3 off the axis and the rest up to 1.5 degrees off it, un-normalised (a direction with a
    zero component is the shader's degenerate case: its march leaves along that axis at once, see tests/test_guides.py W, H)"""
    d = np.zeros((n, 3), np.float32)
    d[:, 0] = 2.0
    d[0, 1:] = (0.002, -0.002)
    d[1:, 1] = np.linspace(-0.05, 0.05, n - 1)
    d[1:, 2] = np.linspace(0.04, -0.04, n - 1)
    if back:
        d[:, 0] = -2.0
    return np.array(EYE_BACK if back else EYE, np.float32), d
