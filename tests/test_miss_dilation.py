"""Miss tiles with the occupancy boxes dilated by the proof's bound (vrt_miss.h kDilate = 0.25 voxel, DESIGN 3 "Miss tiles") instead of a whole
voxel, host side. The property is the one of tests/test_miss_tiles.py, exact: no pixel of a tile the host mask clears is a hit in
the oracle's frame -- here on views where a dilation of one voxel hid whatever the constant was: rays that graze a voxel at 0.25 to
1 voxel, rays that have marched several hundred steps before they pass one, rays that go the negative way or barely move on an
axis. Each group also shows that it exercises the change: it clears tiles that a dilation of 1.0 would have marked."""
import os

import numpy as np
import pytest

import miss_dilation_cases as K
from conftest import MAPS
from test_miss_tiles import BENCH, _check_view, _miss_pixels


def _check(V, O, tex, dim, ip, iv, cp, W, H, what):
    """_check_view() of tests/test_miss_tiles.py for a camera given by its matrices -> the mask (None: the view gets none)"""
    r = V.miss_mask(tex, ip, iv, cp, W, H)
    if r is None:
        return None
    mask, _, whole = r
    if whole:
        assert mask.all()
        return mask
    rgba, idd, _, _ = O.render(O.make_scene(tex, dim, ip, iv, cp), W, H, 0)
    miss = _miss_pixels(rgba, idd, W, H)
    cleared = np.repeat(np.repeat(mask == 0, 8, axis=0), 8, axis=1)[:H, :W]
    bad = cleared & ~miss
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels of cleared tiles hit, first at {np.argwhere(bad)[0]}"
    return mask


def _grazed(mask, ip, iv, cp, W, H, voxels):
    """the tiles the mask clears although a dilation of 1.0 would mark them: a ray of theirs (its centre line, float64) meets a
    voxel's box dilated by 1.0, and the mask marks at least the tiles of the rays that meet a dilated box (the bounding rectangle
    of its corners' projections holds them) -> (tiles, how the rays of those tiles pass the voxel: counts for face, edge, corner)"""
    d = K.pixel_rays(ip, iv, W, H)
    eye = np.asarray(cp[:3], np.float64)
    cleared = np.repeat(np.repeat(mask == 0, 8, axis=0), 8, axis=1)[:H, :W]
    near = np.zeros((H, W), bool)
    kinds = np.zeros(4, int)
    for vox in voxels:
        mn = np.asarray(vox, np.float64)
        m, t0, t1 = K.meets_box(eye, d, mn - 1.0, mn + 2.0)
        m &= cleared
        near |= m
        if m.any():
            kinds += np.bincount(K.approach_kind(eye, d[m], t0[m], t1[m], vox), minlength=4)
    return int(K.tiles_any(near).sum()), kinds


@pytest.fixture(scope="module")
def few(V):
    worlds = {}
    for name in K.FEW:
        w = K.few_voxel_world(V, name)
        worlds[name] = w.flatten()
        w.close()
    return worlds


def test_grazing_rays(V, O, few):
    """one to three voxels, seeded poses whose rays pass 0.3 to 0.9 voxel beside a face, an edge or a corner"""
    tiles, kinds, masked = 0, np.zeros(4, int), 0
    views = K.grazing_views()
    for name, pose, W, H in views:
        tex, dim = few[name]
        ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
        mask = _check(V, O, tex, dim, ip, iv, cp, W, H, f"{name} {pose} {W}x{H}")
        if mask is None:
            continue
        masked += 1
        t, k = _grazed(mask, ip, iv, cp, W, H, K.FEW[name])
        tiles += t
        kinds += k
    print(f"grazing: {masked} of {len(views)} views masked, {tiles} cleared tiles within one voxel of a box, rays beside a "
          f"face / an edge / a corner: {kinds[1]} / {kinds[2]} / {kinds[3]}")
    assert masked == len(views)
    assert kinds[0] == 0                                  # a ray of a cleared tile that enters the voxel: the numpy rays are wrong
    assert tiles >= len(views) and kinds[1] and kinds[2] and kinds[3], (tiles, kinds)


def test_axis_directions_negative_and_tiny_components(V, O, few):
    """along +-x, +-y, +-z, exactly and a hair off: negative-going rays on every axis, zero and tiny components around the centre"""
    tex, dim = few["one"]
    tiles, negative = 0, np.zeros(3, bool)
    tiny = False
    for name, pose, W, H in K.axis_views():
        ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
        mask = _check(V, O, tex, dim, ip, iv, cp, W, H, f"axis view {pose}")
        assert mask is not None
        t, kinds = _grazed(mask, ip, iv, cp, W, H, K.FEW[name])
        assert kinds[0] == 0
        tiles += t
        d = K.pixel_rays(ip, iv, W, H)
        negative |= (d < 0.0).all(axis=(0, 1))            # every ray of the view goes the negative way on this axis
        tiny |= bool((np.abs(d) < 1e-6).any())
    print(f"axis views: {tiles} cleared tiles within one voxel of the box")
    assert negative.all() and tiny and tiles >= 18, (negative, tiny, tiles)


@pytest.mark.parametrize("name", K.LONG)
def test_long_paths(V, O, name):
    """the eye near a corner of the world, 900 unit cells of refraction 1.0 (no box: occupancy_boxes() skips them) on the centre
    ray's way, then one stopping voxel 0.3 to 0.6 voxel beside it. Steps of the centre ray as the oracle counts them (Stats.steps
    of a frame narrowed to that ray): 906 (plus_x), 908 (minus_x), 915 (minus_xz)"""
    w, pose, stop = K.long_path_world(V, name)
    tex, dim = w.flatten()
    w.close()
    W, H = K.LONG_W, K.LONG_H
    ip, iv, cp = K.long_path_camera(V, pose, stop)
    r = V.miss_mask(tex, ip, iv, cp, W, H)
    assert r is not None and r[1] == 1 and not r[2], r   # one box: the stopping voxel's
    mask = _check(V, O, tex, dim, ip, iv, cp, W, H, name)
    # the centre ray's own steps: a frame of 8 x 8 rays that all lie within a thousandth of a pixel of it
    _, idd, _, st = O.render(O.make_scene(tex, dim, K.zoomed(ip, 1e6), iv, cp), 8, 8, 0)
    steps = st["steps"] / 64.0
    t, kinds = _grazed(mask, ip, iv, cp, W, H, [stop])
    print(f"long path {name}: {steps:.0f} steps on the centre ray, {t} cleared tiles within one voxel of the box")
    assert st["hits"] == 0 and 600 <= steps <= 1024, (steps, st)
    assert kinds[0] == 0 and t >= 4, (t, kinds)
    # the frame does see the voxel, and the mask traces every tile that does
    rgba, idd, _, _ = O.render(O.make_scene(tex, dim, ip, iv, cp), W, H, 0)
    hit = ~_miss_pixels(rgba, idd, W, H)
    assert hit.sum() >= 16 and 0.0 < (mask == 0).mean() < 1.0


def test_dragon_bench_frame_floor(V, O):
    """the headline frame: 43.52 % of its 32,400 tiles cleared (measured on the host with kDilate = 0.25; 39.51 % with 1.0; the oracle
    finds 47.26 % all-miss). No fewer than that less half a percentage point"""
    pose, W, H = BENCH["dragon"]
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    tex, dim = w.flatten()
    w.close()
    frac = _check_view(V, O, tex, dim, pose, W, H, "dragon")
    print(f"dragon bench frame: {frac:.4f} of the tiles cleared")
    assert frac is not None and frac >= 0.4352 - 0.005, frac
