"""Miss tiles with the occupancy boxes dilated by 0.25 voxel (vrt_miss.h kDilate), on the device: the worlds and views of
tests/test_miss_dilation.py -- rays that graze a voxel at 0.25 to 1 voxel, views along the axes, voxels reached after some 900 march
steps -- at the same small frame sizes, modes 0 and 1, VRT_OPT_MISS_TILES on against off byte for byte, and one frame per world
against the live oracle. Ordinary launches on small frames."""
import numpy as np
import pytest

import miss_dilation_cases as K
from test_gpu_miss_tiles import _same

pytestmark = pytest.mark.gpu


def _context(V, w, cam, W, H):
    """a context on w's tree whose dispatcher has made its box list: the option on, the tree unchanged for 160 mask requests (at
    least max(64, records / 512) are needed) on a small frame of the camera `cam` (inv_proj, inv_view, cam_pos)"""
    c = V.Context(0)
    tex, dim = w.flatten()
    c.upload_octree(tex, dim)
    c.set_option(V.OPT_MISS_TILES, 1)
    c.set_camera(*cam)
    for _ in range(160):
        c.dispatch(W, H, V.MODE_PRIMARY)
    return c, tex, dim


def _on_off(ctx, V, W, H, what):
    """both modes with the option on, off, on again (a view's mask is built the second time the view is seen: the third run reads it)
    -> the frames with the option off"""
    ref = {}
    for mode in (V.MODE_PRIMARY, V.MODE_PRIMARY_SHADOW):
        out = []
        for on in (1, 0, 1):
            ctx.set_option(V.OPT_MISS_TILES, on)
            out.append(ctx.dispatch(W, H, mode))
        ctx.set_option(V.OPT_MISS_TILES, 1)
        _same(out[0], out[1], f"{what} mode {mode} (on / off)")
        _same(out[2], out[1], f"{what} mode {mode} (on again / off)")
        ref[mode] = out[1]
    return ref


def _oracle(V, O, tex, dim, cam, W, H, got, what):
    for mode in (V.MODE_PRIMARY, V.MODE_PRIMARY_SHADOW):
        rgba, idd, _, _ = O.render(O.make_scene(tex, dim, *cam), W, H, mode)
        _same(got[mode], (np.asarray(rgba).reshape(H, W, 4), np.asarray(idd).reshape(H, W, 2)), f"{what} mode {mode} vs oracle")


@pytest.mark.parametrize("name", sorted(K.FEW))
def test_few_voxel_worlds(V, O, name):
    views = [v for v in K.grazing_views() + K.axis_views() if v[0] == name]
    assert views
    w = K.few_voxel_world(V, name)
    ctx = None
    try:
        for k, (_, pose, W, H) in enumerate(views):
            cam = V.camera_block(pose[:3], pose[3], pose[4], W, H)[:3]
            if ctx is None:
                ctx, tex, dim = _context(V, w, cam, W, H)
            ctx.set_camera(*cam)
            got = _on_off(ctx, V, W, H, f"{name} view {k}")
            if k == 0:
                _oracle(V, O, tex, dim, cam, W, H, got, f"{name} view {k}")
    finally:
        if ctx is not None:
            ctx.close()
        w.close()


@pytest.mark.parametrize("name", K.LONG)
def test_long_paths(V, O, name):
    w, pose, stop = K.long_path_world(V, name)
    W, H = K.LONG_W, K.LONG_H
    cam = K.long_path_camera(V, pose, stop)
    ctx = None
    try:
        ctx, tex, dim = _context(V, w, cam, W, H)
        got = _on_off(ctx, V, W, H, name)
        _oracle(V, O, tex, dim, cam, W, H, got, name)
    finally:
        if ctx is not None:
            ctx.close()
        w.close()
