"""Hand-built worlds of the past-glass guide tests (test_guides_glass.py, test_gpu_guides_glass.py) -- TEST INFRASTRUCTURE ONLY: each
with the rays that go with it and what rule G0-G6 of include/vrt.h must give for them in closed form. The worlds from PANES_WIDE on
belong to the comparison with the float64 reference (test_guides_reference64.py, test_gpu_guides_reference64.py): each exists to
reach one rule of G4 / G5 in rays the reference decides."""
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


def ten_panes(lo=8, hi=13):
    """panes at x = 10, 12, .., 28, a wall at x = 32: along +x the eighth surface is the far side of the fourth pane, x = 17;
    lo, hi: the panes' extent in y and z"""
    v = []
    for x in PANES_X:
        v += slab(x, x + 1, lo, hi, lo, hi, c=GLASS, r=GLASS_REFR)
    return v + slab(32, 33, lo, hi, lo, hi)


# ... wide enough to be seen 30 degrees off the axis as a 40 x 24 frame: chains that end at the surface cap (G4) with refraction on
# the way, through the accumulation routes too (tests/test_guides_reference64.py, tests/test_gpu_guides_reference64.py)
PANES_WIDE = (-6, 40)
PANES_POSE = (2.5, 15.5, 4.5, 30.0, 0.0)
PANES_LENS = (0.5, 12.0)        # aperture, focus distance of its lens sources


# ---- a slab whose index is close to air's: the reflect share's threshold -----------------------------------------------------------
NEAR_REFR = 1.04                   # stored as the byte 88: 88 * 3 / 255 = 1.0353, R0 = 3.0e-4 < 0.001
NEAR_BYTE = 88
NEAR_EYE = (2.5, 10.5, 10.5)


def near_index():
    """a slab two voxels thick of refraction 1.0353 at x = 10, 11 and a wall at x = 16"""
    return slab(10, 12, 0, 21, 0, 56, c=GLASS, r=NEAR_REFR) + slab(16, 17, 0, 21, 0, 64)


def near_index_rays(n=40, seed=7):
    """-> (origin, dirs float32[2n, 3], steep bool[2n]): n rays within 12 degrees of the slab's normal -- there Schlick's term stays below
    (1 - cos 12)^5 = 5e-9 and the reflect share is R0 = 3.0e-4 <= 0.001: the chain ends on the slab with S = 1 -- and n rays 58 to 62
    degrees off it, where the term is (1 - 0.5)^5 = 0.031: the chain goes on, leaves the slab (0.019 there) and ends on the wall"""
    rng = np.random.default_rng(seed)
    d = np.empty((2 * n, 3))
    d[:n, 0] = 1.0
    d[:n, 1:] = rng.uniform(-0.15, 0.15, size=(n, 2))
    ang = np.radians(rng.uniform(58.0, 62.0, size=n))
    d[n:, 0], d[n:, 2] = np.cos(ang), np.sin(ang)
    d[n:, 1] = rng.uniform(-0.1, 0.1, size=n)
    d *= 10.0 ** rng.uniform(-1.0, 1.0, size=(2 * n, 1))
    return np.array(NEAR_EYE, np.float32), d.astype(np.float32), np.arange(2 * n) >= n


# ---- grazing incidence: the refract share's threshold ------------------------------------------------------------------------------
# refract_i = 1 - fres <= 0.001 without TIR needs Schlick's term (1 - cos)^5 >= 0.999 / (1 - R0): cos below about 2.0e-4. A decided
# ray CAN reach it: the reference leaves |cos| undecided only below 1e-6 + the direction's bound, and the shares only within e_F =
# 1.6e-5 of 0.001, so cos in [6e-5, 1.8e-4] is decided by the Fresnel rule. What remains is the march: a ray that slides along the
# face crosses a y or z plane about once per voxel and gains 1e-4 in x per voxel, so from further away its last landing before the
# face lies within the floor margin of it more often than not (from 0.005 in front 19 of 30 such rays were undecided). The rays below
# start 2e-4 in front of the pane and reach it within 3.4 voxels.
GRAZE_EYE = (9.9998, 5.3, 5.3)


def grazing_pane():
    """a pane at x = 10 with a wall right behind it: a ray that entered grazing would leave the glass at the critical angle, where
    TIR is undecided, so it meets an opaque surface first"""
    return slab(10, 11, 0, 14, 0, 14, c=GLASS, r=GLASS_REFR) + slab(11, 12, 0, 14, 0, 14)


def grazing_rays(n=30, seed=9):
    """-> (origin, dirs float32[2n, 3], below bool[2n]): n rays whose cosine to the pane's normal is 6e-5 .. 1.8e-4 (refract_i <= 0.001:
    the chain ends on the pane, S = 1) and n with 2.3e-4 .. 6e-4 (refract_i > 0.001: the chain goes on through the glass to the wall
    behind it)"""
    rng = np.random.default_rng(seed)
    c = np.concatenate([rng.uniform(6e-5, 1.8e-4, size=n), rng.uniform(2.3e-4, 6e-4, size=n)])
    phi = rng.uniform(0.6, 1.0, size=2 * n)
    d = np.stack([c, np.cos(phi), np.sin(phi)], 1) * 10.0 ** rng.uniform(-1.0, 1.0, size=(2 * n, 1))
    return np.array(GRAZE_EYE, np.float32), d.astype(np.float32), np.arange(2 * n) < n


# ---- alpha-0 leaves with a refraction property of their own, on both sides of glass ------------------------------------------------
PHANTOM, PHANTOM_REFR = 0x11223300, 2.0    # alpha 0: air to the march, whatever its property says
ALPHA0_EYE = (2.5, 10.5, 4.5)


def alpha0_beside_glass():
    """air | alpha-0 leaves x = 8, 9 | glass x = 10 .. 13 | alpha-0 leaves x = 14, 15 | air | a wall at x = 20. A ray along +x meets the
    glass with an alpha-0 PREVIOUS voxel (comp:504: its property reads 0, so n1 = 1) and leaves it into an alpha-0 HIT leaf
    (comp:503: its property reads 1, so n2 = 1): the stored 2.0 must show nowhere. A ray that STARTS in the leaves x = 8, 9 carries
    their 2.0 as its medium (comp:448 asks no alpha) and still has n1 = 1 at the glass."""
    return (slab(8, 10, 0, 21, 0, 60, c=PHANTOM, r=PHANTOM_REFR) + slab(10, 14, 0, 21, 0, 60, c=GLASS, r=GLASS_REFR)
            + slab(14, 16, 0, 21, 0, 60, c=PHANTOM, r=PHANTOM_REFR) + slab(20, 21, 0, 21, 0, 80))


def alpha0_rays(n=40, seed=8):
    """-> (origins float32[2n, 3], dirs float32[2n, 3], inside bool[2n]): n rays from ALPHA0_EYE and n from inside the leaves x = 8, 9, all
    20 to 50 degrees off the glass's normal, where a wrong n1 or n2 moves the wall cell"""
    rng = np.random.default_rng(seed)
    o = np.tile(np.array(ALPHA0_EYE), (2 * n, 1))
    o[n:] = np.array([8.0, 8.0, 3.0]) + rng.random((n, 3)) * np.array([2.0, 5.0, 5.0])
    ang = np.radians(rng.uniform(20.0, 50.0, size=2 * n))
    d = np.stack([np.cos(ang), rng.uniform(-0.1, 0.1, size=2 * n), np.sin(ang)], 1)
    d *= 10.0 ** rng.uniform(-1.0, 1.0, size=(2 * n, 1))
    return o.astype(np.float32), d.astype(np.float32), np.arange(2 * n) >= n


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
