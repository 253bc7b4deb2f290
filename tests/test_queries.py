"""World queries on the device tree (vrt_cast_rays, vrt_cast_rays_device, vrt_find_voxels): what holds without a GPU --
the library exports them and the Python wrappers refuse bad arguments before
any device is involved. The answers themselves are checked on the MI355X (test_gpu_queries.py)."""
import subprocess

import numpy as np
import pytest


def test_library_exports_the_query_calls(V):
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in ("vrt_cast_rays", "vrt_cast_rays_device", "vrt_find_voxels"):
        assert n in names, f"{n} is not exported by libvrt_hip.so"


def _unopened(V):
    # a Context whose vrt_create never ran: a wrapper that reached the library would fail on the missing handle
    return object.__new__(V.Context)


@pytest.mark.parametrize("origins,dirs,box,exc", [
    (np.zeros(3, np.float32), np.zeros((4, 2), np.float32), None, ValueError),       # dirs not (n, 3)
    (np.zeros(3, np.float32), np.zeros(12, np.float32), None, ValueError),           # flat dirs
    (np.zeros((3, 3), np.float32), np.zeros((4, 3), np.float32), None, ValueError),  # origins neither (3,) nor (n, 3)
    (np.zeros(2, np.float32), np.zeros((4, 3), np.float32), None, ValueError),
    (np.zeros(3, np.float32), np.zeros((4, 3), np.complex64), None, TypeError),
    (np.array(["a", "b", "c"]), np.zeros((4, 3), np.float32), None, TypeError),
    (np.zeros(3, np.float32), np.zeros((4, 3), np.float32), ((0, 0), (1, 1)), ValueError),
])
def test_cast_rays_rejects_bad_arguments_before_the_device(V, origins, dirs, box, exc):
    ctx = _unopened(V)
    with pytest.raises(exc):
        if box is None:
            ctx.cast_rays(origins, dirs)
        else:
            ctx.cast_rays(origins, dirs, box=box)


@pytest.mark.parametrize("coords,exc", [
    (np.zeros((4, 2), np.int32), ValueError),
    (np.zeros(3, np.int32), ValueError),
    (np.zeros((4, 3), np.float32), TypeError),
    (np.array([[0, 0, 2 ** 40]], np.int64), ValueError),
])
def test_find_voxels_rejects_bad_arguments_before_the_device(V, coords, exc):
    with pytest.raises(exc):
        _unopened(V).find_voxels(coords)


def test_query_arguments_convert_as_documented(V):
    o, stride, d, bmin, bmax = V.query_ray_args((1, 2, 3), np.ones((5, 3), np.float64))
    assert stride == 0 and o.shape == (1, 3) and o.dtype == np.float32 and d.dtype == np.float32 and d.shape == (5, 3)
    assert np.array_equal(bmin, [0, 0, 0]) and np.array_equal(bmax, [1024, 1024, 1024])   # src/main.cpp:827
    o, stride, _, _, _ = V.query_ray_args(np.zeros((5, 3)), np.ones((5, 3)), box=((-1, -2, -3), (4, 5, 6)))
    assert stride == 3 and o.shape == (5, 3)
    c = V.query_point_args(np.array([[1, -2, 3]], np.int64))
    assert c.dtype == np.int32 and c.tolist() == [[1, -2, 3]]


@pytest.mark.parametrize("kw,exc", [
    ({"n": -1}, ValueError),
    ({"n": 2 ** 31}, ValueError),
    ({"n": 4.0}, ValueError),
    ({"origin_stride": 1}, ValueError),
    ({"box": ((0, 0), (1, 1))}, ValueError),
])
def test_cast_rays_device_rejects_bad_arguments_before_the_device(V, kw, exc):
    args = {"n": 4, "d_origins": None, "origin_stride": 3, "d_dirs": None, "d_out": None}
    args.update(kw)
    with pytest.raises(exc):
        _unopened(V).cast_rays_device(**args)
