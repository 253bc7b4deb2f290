"""Shading caller-supplied ray batches (vrt_shade_rays): what holds without a GPU. The checker (tests/oracle_rays.c: the oracle's
path_trace per ray, seeded as pixel (i % width, i / width)) agrees with the oracle's own frames and with the sample checker
(tests/oracle_samples.c) when the batch is a frame's rays; the library declares and exports the two calls; the gfx950 code object
holds the new kernels; the wrappers refuse bad arguments before any device is involved. The kernels are held to the checker on
the MI355X (test_gpu_shade_rays.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_rays
import oracle_samples
from conftest import ROOT

SCENES = {   # name -> (map, W, H, pose): the small committed scenes
    "dragon": ("dragon", 96, 64, (63.5, 60.5, 140.5, -90.0, -10.0)),
    "monu9": ("monu9", 90, 53, (48.5, 60.5, 170.5, -90.0, -12.0)),
    "nature": ("nature", 96, 64, (60.5, 80.5, 200.5, -90.0, -20.0)),
    "room_inside": ("room", 96, 64, (14.5, 30.5, 16.5, 32.0, -10.0)),
    "room_outside": ("room", 96, 64, (98.5, 34.5, 52.5, 197.0, -8.0)),
    "terrain": ("terrain", 240, 136, (512.5, 420.5, 1000.5, -90.0, -20.0)),
}


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_rays"))


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    return oracle_samples.build(tmp_path_factory.mktemp("oracle_samples"))


def _scene(O, V, product_scenes, name):
    m, W, H, pose = SCENES[name]
    tex, dim = product_scenes[m]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    return O.make_scene(tex, dim, ip, iv, cp), W, H


@pytest.mark.parametrize("name", sorted(SCENES))
def test_checker_on_a_frames_rays_is_the_oracle_frame(R, S, O, V, product_scenes, name):
    s, W, H = _scene(O, V, product_scenes, name)
    o, d = oracle_rays.frame_rays(R, s, W, H)
    assert np.array_equal(o, np.tile(np.array(s.cam_pos[:3], np.float32), (W * H, 1)))
    for mode in (0, 1, 2):
        ref_rgba, ref_id, _, st = O.render(s, W, H, mode)
        assert st["hits"] > 500
        for origins in (o, o[0]):   # per-ray origins, and the one shared origin
            rgba, idd = oracle_rays.shade(R, s, origins, d, mode, width=W)
            assert np.array_equal(rgba.reshape(H, W, 4), ref_rgba), f"{name} mode {mode} rgba8"
            assert np.array_equal(idd.reshape(H, W, 2), ref_id), f"{name} mode {mode} id_dist"
    for k in (1, 7, 2 ** 32 - 1):
        ref_rgba, ref_id = oracle_samples.render_sample(S, s, W, H, 2, k)
        rgba, idd = oracle_rays.shade(R, s, o, d, 2, width=W, sample=k)
        assert np.array_equal(rgba.reshape(H, W, 4), ref_rgba), f"{name} sample {k} rgba8"
        assert np.array_equal(idd.reshape(H, W, 2), ref_id), f"{name} sample {k} id_dist"


def test_checker_width_selects_the_random_numbers_and_mean_is_the_resolve_rule(R, O, V, product_scenes):
    s, W, H = _scene(O, V, product_scenes, "dragon")
    o, d = oracle_rays.frame_rays(R, s, W, H)
    a, ida = oracle_rays.shade(R, s, o, d, 2, width=W)
    b, idb = oracle_rays.shade(R, s, o, d, 2, width=7)
    assert np.array_equal(ida, idb) and not np.array_equal(a, b)
    for mode in (0, 1):   # no random number drawn
        assert np.array_equal(oracle_rays.shade(R, s, o, d, mode, width=W)[0], oracle_rays.shade(R, s, o, d, mode, width=7, sample=9)[0])
    one, _ = oracle_rays.mean(R, s, o, d, 2, width=W, first_sample=5, n_samples=1)
    assert np.array_equal(one, oracle_rays.shade(R, s, o, d, 2, width=W, sample=5)[0])
    m, _ = oracle_rays.mean(R, s, o, d, 2, width=W, first_sample=2 ** 32 - 1, n_samples=2)   # wraps to sample 0
    x = oracle_rays.shade(R, s, o, d, 2, width=W, sample=2 ** 32 - 1)[0].astype(np.uint32)
    y = a.astype(np.uint32)
    want = (x + y + 1) // 2
    want[:, 3] = 255
    assert np.array_equal(m, want.astype(np.uint8))


def test_header_declares_and_library_exports_shade_rays(V):
    text = open(os.path.join(ROOT, "include", "vrt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = C.CDLL(V.HIP_LIB)
    for n in ("vrt_shade_rays", "vrt_shade_rays_device"):
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"include/vrt.h does not declare {n}"
        assert n in names and hasattr(lib, n), f"{n} is not exported by libvrt_hip.so"


def test_hip_code_object_holds_the_ray_batch_kernels(V):
    blob = open(V.HIP_LIB, "rb").read()
    assert b"gfx950" in blob
    assert b"shade_rays_kernel" in blob and b"shade_rays_full_kernel" in blob


def test_shade_ray_args_checks_shapes_before_the_device(V):
    o, stride, d = V.shade_ray_args((1.0, 2.0, 3.0), [[0, 0, 1], [0, 1, 0]])
    assert stride == 0 and o.shape == (1, 3) and d.shape == (2, 3) and d.dtype == np.float32
    o, stride, d = V.shade_ray_args(np.zeros((2, 3)), np.ones((2, 3)))
    assert stride == 3 and o.dtype == np.float32
    for bad in [((1.0, 2.0), np.ones((2, 3))), (np.zeros((3, 3)), np.ones((2, 3))), (np.zeros(3), np.ones((2, 2))),
                (np.zeros(3), np.ones(3))]:
        with pytest.raises(ValueError):
            V.shade_ray_args(*bad)
    with pytest.raises(TypeError):
        V.shade_ray_args(np.zeros(3), np.array([["a", "b", "c"]]))
