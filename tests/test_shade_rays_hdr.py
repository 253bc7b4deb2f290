"""Ray batches in HDR (vrt_shade_rays_hdr): what holds without a GPU. The checker's floats (tests/oracle_rays_hdr.c) store the
bytes of the byte checker (tests/oracle_rays.c) in every mode; on the room seen from outside the mean of the unclamped colours is
not the mean of the clamped bytes; the primary modes' one multiply and one add equal the sequential adds; the library declares
and exports the two calls, the gfx950 code object holds the kernels' HDR forms, and the wrappers refuse bad values before any
device is involved. The kernels are held to the checker on the MI355X (test_gpu_shade_rays_hdr.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_hdr
import oracle_rays
import oracle_rays_hdr
from conftest import ROOT
from test_shade_rays import SCENES

SMALL = sorted(SCENES)   # at 48 x 30, to stay quick


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_rays"))


@pytest.fixture(scope="module")
def RH(tmp_path_factory):
    return oracle_rays_hdr.build(tmp_path_factory.mktemp("oracle_rays_hdr"))


def _scene(O, V, product_scenes, name, W=None, H=None):
    m, w, h, pose = SCENES[name]
    W, H = W or w, H or h
    tex, dim = product_scenes[m]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    return O.make_scene(tex, dim, ip, iv, cp), W, H


@pytest.mark.parametrize("name", SMALL)
def test_unorm8_of_the_checkers_floats_is_the_byte_checkers_batch(R, RH, O, V, product_scenes, name):
    s, W, H = _scene(O, V, product_scenes, name, 48, 30)
    o, d = oracle_rays.frame_rays(R, s, W, H)
    for mode in (0, 1, 2):
        for k in (0, 7, 2 ** 32 - 1):
            ref_rgba, ref_id = oracle_rays.shade(R, s, o, d, mode, width=W, sample=k)
            rgb, idd = oracle_rays_hdr.shade(RH, s, o, d, mode, width=W, sample=k)
            assert np.array_equal(oracle_hdr.unorm8(RH, rgb), ref_rgba[:, :3]), (name, mode, k, "rgba8")
            assert np.array_equal(idd, ref_id), (name, mode, k, "id_dist")
    rgb0, _ = oracle_rays_hdr.shade(RH, s, o[0], d, 2, width=W, sample=7)   # the one shared origin
    assert np.array_equal(rgb0.view(np.uint32), oracle_rays_hdr.shade(RH, s, o, d, 2, width=W, sample=7)[0].view(np.uint32))


def test_the_room_from_outside_is_what_the_clamped_mean_loses(R, RH, O, V, product_scenes):
    s, W, H = _scene(O, V, product_scenes, "room_outside", 48, 30)
    o, d = oracle_rays.frame_rays(R, s, W, H)
    above = 0
    for k in range(8):
        above += int((oracle_rays_hdr.shade(RH, s, o, d, 2, width=W, sample=k)[0] > np.float32(1.0)).sum())
    assert above > 0, "no sample above 1: the scene does not show the clamp"
    b = oracle_rays_hdr.Batch(RH, s, o, d, 2, width=W).add(0, 8)
    hdr_bytes = oracle_rays_hdr.tonemap(RH, b.mean(), "clamp", 1.0)
    clamped, idd = oracle_rays.mean(R, s, o, d, 2, width=W, first_sample=0, n_samples=8)
    differ = np.any(hdr_bytes != clamped, axis=1)
    print(f"room from outside 48 x 30, 8 samples: {above} channel samples above 1, {int(differ.sum())} of {W * H} rays differ")
    assert differ.any()
    assert np.array_equal(b.id_dist, idd)
    # the clamp only ever darkens: where they differ by more than the two means' roundings the HDR mean is the brighter
    assert np.all(hdr_bytes[:, :3].astype(int) - clamped[:, :3].astype(int) >= -1)


EDGE = np.array([np.nan, -np.nan, np.inf, -1.0, -0.0, 0.0, 1e-45, 1e-39, 1.17549435e-38, 0.5, 1.0, 1.0000001, 10.0, 65503.996, 65504.0,
                 65504.004, 65536.0, 1e30, 3.4028235e38], np.float32)


def test_one_multiply_and_one_add_are_the_sequential_adds(RH):
    """vrt_shade_rays_hdr, point 2, the primary modes: onto a sum holding m * h(c), (double)h(c) * n added once is n adds of
    (double)h(c), for m + n <= 2^24. The adds are tests/oracle_hdr.c's own (o_hdr_add: every value n times; o_hdr_sum_repeat:
    from +0.0 up to the cap)."""
    rng = np.random.default_rng(11)
    vals = np.concatenate([EDGE, rng.integers(0, 2 ** 32, 3000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                           rng.random(1000, dtype=np.float32) * np.float32(12.0)])
    prod = lambda k: np.array([RH.o_hdr_product(C.c_float(v.item()), k) for v in vals], np.float64)
    for m, n in ((0, 1), (0, 5), (3, 5), (1, 300), (2 ** 24 - 300, 300), (2 ** 23 + 1, 257), (12345677, 123)):
        assert m + n <= 2 ** 24
        seq = prod(m)
        for _ in range(n):
            RH.o_hdr_add(seq.ctypes.data, vals.ctypes.data, None, vals.size)
        once = prod(m) + prod(n)   # numpy's float64 add: IEEE, one rounding
        assert np.array_equal(seq.view(np.uint64), once.view(np.uint64)), (m, n)
        assert np.array_equal(once.view(np.uint64), prod(m + n).view(np.uint64)), (m, n)
    # n up to 2^24 - m, from +0.0 and in two parts, on a handful of values (16.7 M adds each)
    for c in (np.float32(1.0 / 3.0), np.float32(9.999999), np.float32(65504.0), np.float32(1e-45), np.float32(1e9), np.float32(np.nan)):
        whole = RH.o_hdr_sum_repeat(C.c_float(c.item()), 2 ** 24)
        for m in (1, 2 ** 23, 2 ** 24 - 1, 5000001):
            parts = np.float64(RH.o_hdr_product(C.c_float(c.item()), m)) + np.float64(RH.o_hdr_product(C.c_float(c.item()), 2 ** 24 - m))
            assert np.float64(whole).view(np.uint64) == parts.view(np.uint64), (c, m)


def test_header_declares_and_library_exports_the_hdr_calls(V):
    text = open(os.path.join(ROOT, "include", "vrt.h")).read()
    assert "vrt_shade_rays have no float output" not in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = C.CDLL(V.HIP_LIB)
    for n in ("vrt_shade_rays_hdr", "vrt_shade_rays_hdr_device"):
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"include/vrt.h does not declare {n}"
        assert n in names and hasattr(lib, n), f"{n} is not exported by libvrt_hip.so"


def test_hip_code_object_holds_the_hdr_forms(V):
    """shade_rays_kernel<MODE, TRAV, WPE, HDR> and shade_rays_full_kernel<TRAV, WPE, LOOP, HDR, X...> over rays::HdrArgs: the mangled
    names end their template arguments in Lb1E (HDR = true) -- and, the full kernel's, in the empty pack JE of a family that takes no
    argument -- in both modes' kernels and both LOOP forms"""
    blob = open(V.HIP_LIB, "rb").read()
    assert b"gfx950" in blob
    names = set(re.findall(rb"_ZN3vrt4rays\d+shade_rays_(?:full_)?kernelI[A-Za-z0-9_]+", blob))
    hdr = {n for n in names if re.search(rb"Lb1E(?:JE)?EEv", n)}
    assert any(b"shade_rays_kernelILi0E" in n for n in hdr) and any(b"shade_rays_kernelILi1E" in n for n in hdr), sorted(names)
    assert any(b"full_kernel" in n and b"Lb1ELb1EJEEEv" in n for n in hdr), sorted(names)
    assert any(b"full_kernel" in n and b"Lb0ELb1EJEEEv" in n for n in hdr), sorted(names)


def test_wrappers_refuse_bad_values_before_the_device(V):
    ctx = V.Context.__new__(V.Context)   # no device, no library handle: any call into the library would raise AttributeError
    o, d = np.zeros(3, np.float32), np.array([[0.0, 0.0, 1.0]], np.float32)
    bad = [dict(tonemap="aces"), dict(tonemap=1), dict(exposure=0.0), dict(exposure=-1.0), dict(exposure=float("nan")),
           dict(exposure=float("inf")), dict(exposure=1e39), dict(exposure="1"), dict(exposure=True),
           dict(n_samples=0), dict(n_samples=2 ** 24 + 1), dict(n_samples=1.5), dict(n_samples=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            ctx.shade_rays_hdr(o, d, **kw)
        with pytest.raises(ValueError):
            ctx.shade_rays_hdr_device(1, 1, 0, 1, 1, None, None, **kw)
    with pytest.raises(ValueError):
        ctx.shade_rays_hdr(np.zeros((3, 3)), np.ones((2, 3)))
    for kw in (dict(n_prior=1), dict(n_prior=-1, d_sums=1), dict(n_prior=2 ** 24, d_sums=1), dict(n_prior=2 ** 24 - 1, n_samples=2, d_sums=1),
               dict(n_prior=1.0, d_sums=1), dict(n_prior=True, d_sums=1)):
        with pytest.raises(ValueError):
            ctx.shade_rays_hdr_device(1, 1, 0, 1, 1, None, None, **kw)
    for n in (-1, 2 ** 30 + 1, 1.0, True):
        with pytest.raises(ValueError):
            ctx.shade_rays_hdr_device(n, 1, 0, 1, 1, None, None)
