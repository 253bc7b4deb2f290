"""Miss tiles (include/vrt.h VRT_OPT_MISS_TILES, DESIGN 3 "Miss tiles"), host side: the mask the dispatcher hands the EYE85 primary kernels,
built by the same host code and the same per-box function the device build runs (vrt_test_miss_mask), against oracle frames.
The claim under test: every pixel of a tile the mask clears is a miss in the oracle's frame (the kernel additionally requires the
ray to point forward on every axis; these checks leave that condition out and so test a superset of the pixels it skips).

Zero-colour "ghost" leaves (include/vrt.h, vrt_cast_rays): the device tree stores them as empty space. They have refraction byte 0,
which the occupancy boxes skip, and alpha 0, so a primary ray that meets one does not stop in the oracle either (its medium reads as
empty space, comp:318-326): the maps' ghost leaves change no frame, and the bench frames below are compared with the oracle as they
are. A world whose frames did depend on them would be checked against the device's rule instead -- none of the worlds here does."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, MAPS, terrain_world

SKY = (0.5, 0.7, 1.0)
BENCH = {  # bench.py POSES and the BASELINE configurations' frame sizes
    "dragon": ((63.5, 60.5, 140.5, -90.0, -10.0), 1920, 1080),
    "monu9": ((48.5, 60.5, 170.5, -90.0, -12.0), 1280, 720),
    "nature": ((60.5, 80.5, 200.5, -90.0, -20.0), 3840, 2160),
    "terrain": ((512.5, 420.5, 1000.5, -90.0, -20.0), 1920, 1080),
}
PALETTE = [(0xa0a0a0ff, 3.0, 0.0, 0.0), (0x50b43cff, 3.0, 0.0, 0.0), (0xffd2d2ff, 3.0, 1.0, 0.0), (0x3c64dc96, 1.33, 0.0, 0.02),
           (0xc8dcff50, 1.5, 0.0, 0.0), (0xff3030ff, 3.0, 0.25, 0.0), (0x20202000, 1.2, 0.0, 0.0), (0x80ff80c0, 1.0, 0.0, 0.0)]


def _unorm8(v):
    return int(np.rint(np.float32(min(max(v, 0.0), 1.0)) * np.float32(255.0)))


def _miss_pixels(rgba, idd, W, H, wmin0=-1023, wmax0=1024):
    """per pixel: the oracle's frame shows the miss outputs (sky x global light 1, voxel id 0, dist = the world's x extent)"""
    sky = _unorm8(SKY[0]) | (_unorm8(SKY[1]) << 8) | (_unorm8(SKY[2]) << 16) | (255 << 24)
    rgba = np.ascontiguousarray(rgba).view(np.uint32).reshape(H, W)
    idd = np.asarray(idd).reshape(H, W, 2)
    return (rgba == np.uint32(sky)) & (idd[..., 0] == 0) & (idd[..., 1] == wmax0 - wmin0)


def _check_view(V, O, tex, dim, pose, W, H, what):
    """-> the fraction of tiles the mask clears (None: the view gets no mask); asserts that no cleared tile holds a hit"""
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    r = V.miss_mask(tex, ip, iv, cp, W, H)
    if r is None:
        return None
    mask, _, whole = r
    if whole:
        assert mask.all()
        return 0.0
    rgba, idd, _, _ = O.render(O.make_scene(tex, dim, ip, iv, cp), W, H, 0)
    miss = _miss_pixels(rgba, idd, W, H)
    cleared = np.repeat(np.repeat(mask == 0, 8, axis=0), 8, axis=1)[:H, :W]
    bad = cleared & ~miss
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels of cleared tiles hit, first at {np.argwhere(bad)[0]}"
    return float((mask == 0).mean())


@pytest.mark.parametrize("name", ["dragon", "monu9", "nature", "terrain"])
def test_bench_poses_clear_only_miss_tiles(V, O, name):
    pose, W, H = BENCH[name]
    if name == "terrain":
        w = terrain_world(V)
    else:
        w = V.World()
        assert w.load_vox(os.path.join(MAPS, name + ".vox"))
    tex, dim = w.flatten()
    w.close()
    frac = _check_view(V, O, tex, dim, pose, W, H, name)
    assert frac is not None
    if name == "dragon":   # the headline frame: the oracle has 47.3 % of its tiles all-miss
        assert frac >= 0.35, frac


def _random_world(V, rng):
    w = V.World()
    span = int(rng.choice([12, 40, 200]))
    positive = rng.random() < 0.6
    lo = 0 if positive else -span // 4
    base = rng.integers(0, 3, size=3) * int(rng.choice([0, 64, 256])) if positive else np.zeros(3, int)
    pts = []
    for _ in range(int(rng.integers(1, 4))):
        y = int(rng.integers(0, span // 2 + 1))
        x0, z0 = (int(v) for v in rng.integers(lo, span // 2, size=2))
        sx, sz = (int(v) for v in rng.integers(2, 14, size=2))
        m = PALETTE[int(rng.integers(0, len(PALETTE)))]
        xs, zs = np.meshgrid(np.arange(x0, x0 + sx), np.arange(z0, z0 + sz))
        xyz = np.stack([xs.ravel(), np.full(xs.size, y), zs.ravel()], axis=1) + base
        w.insert_many(xyz.astype(np.int32), np.full(len(xyz), m[0], np.uint32), m[1], m[2], m[3])
        pts.append(xyz)
    for _ in range(int(rng.integers(2, 7))):
        c = rng.integers(lo, span, size=3)
        k = int(rng.integers(1, 60))
        xyz = (c + rng.integers(-3, 4, size=(k, 3))).astype(np.int64)
        if positive:
            xyz = np.abs(xyz)
        xyz = xyz + base
        m = PALETTE[int(rng.integers(0, len(PALETTE)))]
        w.insert_many(xyz.astype(np.int32), np.full(k, m[0], np.uint32), m[1], m[2], m[3])
        pts.append(xyz)
    return w, np.concatenate(pts), span


def _edit(w, rng, pts):
    """a voxel edit and a box edit: remove some voxels, fill a small box with a solid"""
    for p in pts[rng.integers(0, len(pts), size=int(rng.integers(1, 6)))]:
        w.remove(int(p[0]), int(p[1]), int(p[2]))
    c = pts[int(rng.integers(0, len(pts)))] + rng.integers(-6, 7, size=3)
    n = rng.integers(1, 5, size=3)
    g = np.stack(np.meshgrid(*[np.arange(int(c[k]), int(c[k] + n[k])) for k in range(3)], indexing="ij"), -1).reshape(-1, 3)
    m = PALETTE[int(rng.integers(0, 3))]
    w.insert_many(g.astype(np.int32), np.full(len(g), m[0], np.uint32), m[1], m[2], m[3])
    return np.concatenate([pts, g])


def _pose(rng, pts, span, kind):
    target = pts[int(rng.integers(0, len(pts)))] + 0.5
    if kind == "inside":             # in the content's bounding box
        lo, hi = pts.min(0), pts.max(0) + 1
        pos = lo + rng.random(3) * (hi - lo)
    elif kind == "face":             # beside a face of a voxel
        ax = int(rng.integers(0, 3))
        pos = target.copy()
        pos[ax] += float(rng.choice([-1.0, 1.0])) * float(rng.uniform(0.5, 0.6))
    elif kind == "outside":          # outside the world [-1023, 1024)^3
        d = rng.normal(size=3)
        pos = target + d / np.linalg.norm(d) * 1600.0
    else:
        away = rng.normal(size=3)
        away[1] = abs(away[1]) + 0.2
        pos = target + away / np.linalg.norm(away) * float(rng.choice([1.7, 6.0, span * 0.5, span * 1.5, 700.0]))
    d = target - pos
    if not np.any(d):
        d = np.array([1.0, 0.0, 0.0])
    yaw = float(np.degrees(np.arctan2(d[2], d[0])))
    pitch = float(np.clip(np.degrees(np.arctan2(d[1], np.hypot(d[0], d[2]))), -89.0, 89.0))
    if kind == "axis":               # directions on and next to the axes
        yaw = float(rng.choice([-180.0, -90.0, 0.0, 90.0])) + float(rng.choice([0.0, 1e-4, -1e-3]))
        pitch = float(rng.choice([-89.0, 0.0, 89.0, 1e-4]))
    return (float(pos[0]), float(pos[1]), float(pos[2]), yaw, pitch)


def test_random_worlds_and_poses_clear_only_miss_tiles(V, O):
    rng = np.random.default_rng(20261016)
    kinds = ["near", "inside", "face", "outside", "axis"]
    views = masked = cleared = outside = 0
    for case in range(44):
        w, pts, span = _random_world(V, rng)
        for stage in range(2):       # the world as built, then after a voxel edit and a box edit
            if stage:
                pts = _edit(w, rng, pts)
            tex, dim = w.flatten()
            for _ in range(3 if stage == 0 else 2):
                kind = kinds[int(rng.integers(0, len(kinds)))]
                W, H = int(rng.integers(24, 129)), int(rng.integers(16, 97))
                pose = _pose(rng, pts, span, kind)
                frac = _check_view(V, O, tex, dim, pose, W, H, f"case {case} stage {stage} {kind}")
                views += 1
                if not all(-1023 <= np.float32(c) < 1024 for c in pose[:3]):   # an eye outside the world: no mask (the march's
                    # first step can go backwards)
                    assert frac is None
                    outside += 1
                elif frac is not None:
                    masked += 1
                    cleared += frac > 0.0
        w.close()
    assert views >= 200
    assert outside >= 20 and masked >= 0.9 * (views - outside) and cleared >= views // 3, (views, outside, masked, cleared)


def test_empty_world_clears_every_tile(V):
    w = V.World()
    tex, dim = w.flatten()
    w.close()
    ip, iv, cp, _ = V.camera_block((10.5, 20.5, 30.5), -90.0, -10.0, 64, 48)
    mask, boxes, whole = V.miss_mask(tex, ip, iv, cp, 64, 48)
    assert boxes == 0 and not whole and not mask.any()


def test_eye_in_a_box_marks_the_whole_view(V):
    """a box that reaches the eye's plane: every tile traced"""
    w = V.World()
    w.insert(10, 20, 30, 0xa0a0a0ff, 3.0, 0.0, 0.0)
    tex, dim = w.flatten()
    w.close()
    ip, iv, cp, _ = V.camera_block((10.5, 20.5, 30.5), -90.0, -10.0, 64, 48)
    mask, boxes, whole = V.miss_mask(tex, ip, iv, cp, 64, 48)
    assert boxes == 1 and whole and mask.all()
    # ... and behind the eye: nothing traced
    ip, iv, cp, _ = V.camera_block((10.5, 20.5, 40.5), 90.0, 0.0, 64, 48)
    mask, boxes, whole = V.miss_mask(tex, ip, iv, cp, 64, 48)
    assert not whole and not mask.any()


def test_non_separable_projection_gets_no_mask(V):
    """the mask is made in the ray tables' coordinates: a projection the table check refuses gets none"""
    w = V.World()
    w.insert(10, 20, 30, 0xa0a0a0ff, 3.0, 0.0, 0.0)
    tex, dim = w.flatten()
    w.close()
    ip, iv, cp, _ = V.camera_block((10.5, 20.5, 60.5), -90.0, 0.0, 64, 48)
    ip = np.array(ip, np.float32).reshape(-1).copy()
    ip[4] = 0.01   # x now depends on v too: not the separable shape
    assert V.miss_mask(tex, ip, iv, cp, 64, 48) is None
