"""The worlds of the sun-disc tests (test_sun_disc.py, test_gpu_sun_disc.py) -- TEST INFRASTRUCTURE ONLY: those of
test_gpu_path_depth.py (the dragon, the room seen from inside, the unit-internal stream) with their poses and lenses, and the
hand-built slab over a floor whose penumbra has a closed form."""
import numpy as np

W, H = 72, 44   # nine tiles across and a half tile at the bottom edge
WORLDS = ("dragon", "room", "unit")
POSES = {"dragon": (63.5, 60.5, 140.5, -90.0, -10.0), "room": (14.5, 30.5, 16.5, 32.0, -10.0), "unit": (1.3, 2.1, 0.7, 52.0, 18.0)}
LENS = {"dragon": (0.8, 80.0), "room": (0.7, 30.0), "unit": (0.05, 3.0)}   # aperture, focus distance
UNIT_BOUNDS = ((0, 0, 0), (8, 8, 8))


def _tx(value, alpha):
    return [value & 255, (value >> 8) & 255, (value >> 16) & 255, alpha]


def unit_stream():
    """test_gpu_parity's hand-written stream whose unit cell [4,5)^3 is still an internal node: no wide layout, the explicit-AABB kernels"""
    leaf = [200, 40, 90, 255, 255, 0, 0, 255]
    return np.array(_tx(1, 0x80) + _tx(2, 0) + _tx(3, 0x01) + _tx(4, 0) + _tx(5, 0x01) + _tx(6, 0) + _tx(7, 0x80) + _tx(8 | 0x800000, 0) + leaf,
                    np.uint8), 3


def scenes(O, V, product_scenes):
    """name -> (texels, tex_dim, (inv_proj, inv_view, cam_pos), oracle scene) of the three worlds at W x H"""
    out = {}
    for name in WORLDS:
        tex, dim = unit_stream() if name == "unit" else product_scenes[name]
        pose = POSES[name]
        ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
        s = O.make_scene(tex, dim, ip, iv, cp)
        if name == "unit":
            s.bounds_min[:] = UNIT_BOUNDS[0]
            s.bounds_max[:] = UNIT_BOUNDS[1]
        out[name] = (tex, dim, (ip, iv, cp), s)
    return out


# The slab: an opaque floor whose top face is y = SLAB_FLOOR_TOP, and an opaque slab SLAB_H voxels above it whose straight edge
# lies along z at x = SLAB_X0; the slab reaches 20 voxels beyond the edge in -x and 19.5 in +-z around the floor points.
SLAB_X0, SLAB_Z, SLAB_FLOOR_TOP, SLAB_H = 40, 40.5, 11, 8
SLAB_LIGHT = (0.0, 1.0, 0.0)   # T = (-1, 0, 0), B = (0, 0, 1)


def slab_world(V):
    w = V.World()
    stone = (0xa0a0a0ff, 3.0, 0.0, 0.0)   # opaque, non-emissive
    for x in range(20, 60):
        for z in range(20, 60):
            w.insert(x, SLAB_FLOOR_TOP - 1, z, *stone)
            if x < SLAB_X0:
                w.insert(x, SLAB_FLOOR_TOP + SLAB_H, z, *stone)
    return w


def slab_rays(offsets):
    """one ray per offset x - x0: from 0.5 above the floor point, straight down -- but for 1e-6 in x and z: on a direction component
    below 1e-8 hitMarching takes 1e20 for its reciprocal (comp:250-258) and such a ray, the shader's degenerate axis-parallel case,
    leaves the world backwards without meeting the floor. 1e-6 moves the hit point by 5e-7, an eighth of the float32 spacing at x = 40."""
    o = np.array([(SLAB_X0 + dx, SLAB_FLOOR_TOP + 0.5, SLAB_Z) for dx in offsets], np.float32)
    d = np.tile(np.array([1e-6, -1.0, 1e-6], np.float32), (len(offsets), 1))
    return o, d
