"""Bloom without a device (include/vrt.h vrt_bloom_hdr, points B0-B8): the struct mirror against a compiled probe of the header, the
defaults, the exports and the signature table, vrt_bloom_workspace_bytes against a Python restatement, the scalar C checker
(tests/oracle_bloom.c) against the float32 numpy restatement (tests/oracle_bloom.py py_run) bit for bit, every planted misreading of
the checker caught, the three identities that follow from the weights, what the Python wrapper refuses, and the shared layout
(csrc/vrt_bloom.h) as a program of its own under the host sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_bloom as B
from conftest import ROOT
from test_meter import nasty_pixels

CSRC = os.path.join(ROOT, "voxel-raytracer_amd", "csrc")
f32 = np.float32
FUNCTIONS = ("vrt_bloom_default", "vrt_bloom_workspace_bytes", "vrt_bloom_hdr", "vrt_bloom_hdr_host", "vrt_accum_resolve_hdr_bloomed",
             "vrt_accum_resolve_hdr_bloomed_device")


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return B.build(tmp_path_factory.mktemp("oracle_bloom"))


def image(seed, h, w, lo=-14.0, hi=12.0):
    """channels over 26 octaves"""
    rng = np.random.default_rng(seed)
    return (2.0 ** rng.uniform(lo, hi, (h, w, 3))).astype(f32)


def same(got, want, what):
    """two results of run() / py_run(), bit for bit"""
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), f"{what}: f"
    assert np.array_equal(got[1], want[1]), f"{what}: the bytes"
    if len(want) > 2:
        for l, (a, b) in enumerate(zip(got[2], want[2])):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: D_{l + 1}"
        assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32)), f"{what}: B"


# ---- the interface ----

def test_the_struct_mirror_is_the_headers(V, tmp_path):
    """the header's text field by field, and a compiled probe of it for size and offsets"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrt.h")).read(), flags=re.S)
    ctypes_of = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    body = re.search(r"struct\s+vrt_bloom\s*\{(.*?)\}\s*;", text, flags=re.S).group(1)
    assert re.search(r"typedef\s+struct\s+vrt_bloom\s+vrt_bloom\s*;", text)
    fields = [(n.strip(), ctypes_of[d.split(None, 1)[0]]) for d in (d.strip() for d in body.split(";")) if d
              for n in d.split(None, 1)[1].split(",")]
    for mirror in (V.Bloom, B.Bloom):
        assert fields == list(mirror._fields_)
    assert V.BLOOM_MAX_LEVELS == B.MAX_LEVELS == int(re.search(r"#define VRT_BLOOM_MAX_LEVELS (\d+)", text).group(1))
    assert V.BLOOM_KARIS == B.KARIS == int(re.search(r"#define VRT_BLOOM_KARIS (\d+)u", text).group(1))
    probe = tmp_path / "probe.c"
    rows = ['printf("vrt_bloom %zu\\n", sizeof(vrt_bloom));'] + [f'printf("vrt_bloom.{n} %zu\\n", offsetof(vrt_bloom, {n}));' for n, _ in V.Bloom._fields_]
    probe.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vrt.h"\nint main(void) {\n' + "\n".join(rows) + "\nreturn 0;\n}\n")
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(probe)], check=True)
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    want = {"vrt_bloom": C.sizeof(V.Bloom)}
    want.update({f"vrt_bloom.{n}": getattr(V.Bloom, n).offset for n, _ in V.Bloom._fields_})
    assert {k: int(v) for k, v in got.items()} == want and want["vrt_bloom"] == 20


def test_the_defaults(V):
    b = V.Bloom()
    V.hip_lib().vrt_bloom_default(C.byref(b))
    made = B.make()
    for k, _ in V.Bloom._fields_:
        assert getattr(b, k) == getattr(made, k), k
    assert (b.levels, b.flags, b.threshold, b.knee, b.intensity) == (5, 1, 1.0, 0.5, float(f32(0.2)))
    assert V.default_bloom() == B.keys(made) and tuple(V.default_bloom()) == B.KEYS
    V.hip_lib().vrt_bloom_default(None)   # a NULL pointer is ignored


def test_header_declares_and_library_exports_the_functions(V):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrt.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for fn in FUNCTIONS:
        assert re.search(r"\b" + fn + r"\s*\(", text), fn
        assert fn in names and fn in V.HIP_API, fn
    blob = open(V.HIP_LIB, "rb").read()
    for kernel in (b"bloom_down_kernel", b"bloom_up_kernel"):
        assert re.search(rb"_ZN3vrt5bloom\d+" + kernel, blob), f"no device function vrt::bloom::{kernel.decode()}"
    for method in ("bloom_hdr", "bloom_hdr_device", "accum_resolve_hdr_bloomed", "accum_resolve_hdr_bloomed_device"):
        assert callable(getattr(V.Context, method)), method
    assert callable(V.default_bloom) and callable(V.bloom_workspace_bytes)


def test_workspace_bytes_is_the_restatement(V):
    lib = V.hip_lib()
    for levels in range(1, B.MAX_LEVELS + 1):
        for w in range(1, 71):
            for h in range(1, 71):
                assert lib.vrt_bloom_workspace_bytes(w, h, levels) == B.workspace_bytes(w, h, levels), (w, h, levels)
        big = lib.vrt_bloom_workspace_bytes(1 << 15, 1 << 15, levels)
        assert big == B.workspace_bytes(1 << 15, 1 << 15, levels) and big >= (1 << 28) * 16
    assert B.workspace_bytes(1, 1, 8) == 8 * 256 and B.workspace_bytes(3, 1, 2) == 512 and B.workspace_bytes(67, 33, 1) == 37 * 256   # 34 x 17 pixels: 9,248 bytes
    assert V.bloom_workspace_bytes(1920, 1080, 5) == B.workspace_bytes(1920, 1080, 5) > 0
    # 0 for what the call would refuse
    for w, h, levels in ((0, 4, 1), (4, 0, 1), (-1, 4, 1), (4, 4, 0), (4, 4, 9), (4, 4, -1), ((1 << 15) + 1, 1 << 15, 1), (1 << 16, 1 << 15, 3)):
        assert lib.vrt_bloom_workspace_bytes(w, h, levels) == 0 == B.workspace_bytes(w, h, levels), (w, h, levels)
    assert lib.vrt_bloom_workspace_bytes(1 << 30, 1, 8) == B.workspace_bytes(1 << 30, 1, 8) > 0


def test_what_the_wrapper_refuses(V):
    nan, inf = float("nan"), float("inf")
    for kw in (dict(levels=0), dict(levels=9), dict(levels=2.0), dict(levels=True), dict(karis=2), dict(karis="yes"), dict(threshold=-1.0),
               dict(threshold=65505.0), dict(threshold=nan), dict(knee=-0.5), dict(knee=1.5), dict(knee=nan), dict(threshold=0.25, knee=0.5),
               dict(intensity=-0.1), dict(intensity=inf), dict(intensity=nan), dict(intensity=7e4), dict(nonsense=1)):
        with pytest.raises(ValueError):
            V._bloom(kw)
    b = V._bloom(dict(levels=8, karis=False, threshold=65504.0, knee=65504.0, intensity=0.0))
    assert (b.levels, b.flags, b.threshold, b.knee, b.intensity) == (8, 0, 65504.0, 65504.0, 0.0)
    assert V._bloom(None) is None and V._bloom({}).levels == 5
    with pytest.raises(ValueError):
        V.bloom_workspace_bytes(4.0, 4, 1)


# ---- the two restatements ----

CASES = [   # (Bloom, op, tm exposure, record exposure or None)
    (B.make(), "clamp", 1.0, None),
    (B.make(levels=1, karis=False), "reinhard", 0.7, None),
    (B.make(levels=2, karis=True, threshold=0.5, knee=0.5, intensity=1.0), "clamp", 2.0, 0.37),
    (B.make(levels=8, karis=False, threshold=0.0, knee=0.0, intensity=0.5), "reinhard", 1.0, 3.0),
    (B.make(levels=3, karis=True, threshold=4.0, knee=0.0, intensity=65504.0), None, 1.0, 2.0 ** -10),
    (B.make(levels=4, karis=False, threshold=65504.0, knee=65504.0, intensity=0.25), "clamp", 3e30, 3e30),
]


def state_of(e):
    return None if e is None else {"exposure": e, "metered": 1.0, "window": 1, "frames": 1}


@pytest.mark.parametrize("size", [(1, 1), (2, 1), (3, 1), (1, 9), (67, 33), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_checker_is_the_numpy_restatement_on_random_images(L, size):
    w, h = size
    rgb = image(w * 100 + h, h, w)
    for i, (b, op, e, rec) in enumerate(CASES):
        same(B.run(L, rgb, b, op, e, state_of(rec), detail=True), B.py_run(rgb, b, op, e, state_of(rec), detail=True), f"{size}, case {i}")


def test_the_checker_is_the_numpy_restatement_on_nasty_pixels(L):
    px = nasty_pixels()
    rgb = px[:len(px) // 7 * 7].reshape(7, -1, 3)
    for i, (b, op, e, rec) in enumerate(CASES):
        got = B.run(L, rgb, b, op, e, state_of(rec), detail=True)
        same(got, B.py_run(rgb, b, op, e, state_of(rec), detail=True), f"case {i}")
        assert np.isfinite(got[0]).all() and got[0].min() >= 0 and got[0].max() <= 65504.0 and not np.signbit(got[0]).any()
    # ... and in a frame with more than one row of tiles: the same pixels as 43 rows
    rgb = px[:len(px) // 43 * 43].reshape(43, -1, 3)
    same(B.run(L, rgb, B.make(), "reinhard", 1.5, state_of(0.8)), B.py_run(rgb, B.make(), "reinhard", 1.5, state_of(0.8)), "43 rows")


# ---- the planted misreadings ----

def test_every_planted_misreading_is_caught(L):
    rgb = image(5, 33, 67, -6.0, 6.0)

    def differs(b, plant, e=1.0, rec=None, op="clamp"):
        got, want = B.run(L, rgb, b, op, e, state_of(rec), plant), B.py_run(rgb, b, op, e, state_of(rec))
        return not np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))

    soft = B.make(levels=3, karis=False, threshold=1.0, knee=0.5, intensity=1.0)
    karis = B.make(levels=3, karis=True, threshold=1.0, knee=0.5, intensity=1.0)
    assert differs(soft, "far_near_swapped") and differs(B.make(levels=1, karis=False, intensity=1.0), "far_near_swapped")
    assert differs(soft, "tent_by_multiplying")
    assert differs(karis, "karis_weight_at_level_2") and differs(B.make(levels=1, intensity=1.0), "karis_weight_at_level_2")
    assert differs(soft, "threshold_against_y", e=0.5) and differs(soft, "threshold_against_y", rec=4.0)
    assert differs(soft, "inv_levels_left_out") and differs(B.make(levels=2, karis=False, intensity=1.0), "inv_levels_left_out")
    # ... and none of them is seen where it cannot matter: the checker with a plant is the rule there
    assert not differs(soft, "karis_weight_at_level_2")
    assert not differs(soft, "threshold_against_y") and not differs(karis, "threshold_against_y")
    assert not differs(B.make(levels=1, karis=False, intensity=1.0), "inv_levels_left_out")
    for plant in B.PLANT:
        assert not differs(B.make(levels=2, intensity=0.0), plant), plant   # no gain: f is h(x)
    # the bytes see the record: e, not tm->exposure alone
    got = B.run(L, rgb, soft, "clamp", 0.5, state_of(0.25))
    assert np.array_equal(got[1], B.py_run(rgb, soft, "clamp", 0.5, state_of(0.25))[1])
    assert not np.array_equal(got[1], B.py_run(rgb, soft, "clamp", 0.5, None)[1])


# ---- the identities ----

@pytest.mark.parametrize("size", [(1, 1), (3, 1), (67, 33), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_constant_image_stays_constant(L, size):
    """threshold = knee = 0, no KARIS, eb = 1: every D_l and B are exactly k for a dyadic k"""
    w, h = size
    k = f32(0.75)
    rgb = np.full((h, w, 3), k, f32)
    for levels in (1, 2, 4, 8):
        b = B.make(levels=levels, karis=False, threshold=0.0, knee=0.0, intensity=0.5)
        for f, _, ds, glow in (B.run(L, rgb, b, detail=True), B.py_run(rgb, b, detail=True)):
            for l, d in enumerate(ds):
                assert (d[..., :3] == k).all() and (d[..., 3] == 1.0).all(), (levels, l + 1)
            assert (glow == k).all(), levels
            assert (f == f32(k + f32(0.5) * k)).all()


def test_scaling_by_a_power_of_two_is_exact(L):
    """the image, the threshold and the knee scaled by 2^j scale B and f exactly where no clamp of h and not the 2^-16 floor is met"""
    rgb = image(3, 31, 45, -6.0, 4.0)
    base = B.make(levels=4, karis=False, threshold=1.0, knee=0.5, intensity=0.75)
    f0, _, d0, glow0 = B.run(L, rgb, base, detail=True)
    assert glow0.max() > 0.01 and (glow0 > 0).mean() > 0.5
    for j in (-4, -1, 1, 2, 5):
        s = f32(2.0 ** j)
        b = B.make(levels=4, karis=False, threshold=float(s), knee=float(f32(0.5) * s), intensity=0.75)
        for run in (lambda *a, **k: B.run(L, *a, **k), B.py_run):
            f, _, d, glow = run((rgb * s).astype(f32), b, detail=True)
            assert np.array_equal(glow, glow0 * s) and np.array_equal(f, f0 * s), j
            for a, a0 in zip(d, d0):
                assert np.array_equal(a[..., :3], a0[..., :3] * s), j


def test_one_pixel_keeps_its_energy(L):
    """a single pixel of value 8 in a black 256 x 256 frame: 4^l * sum(D_l) == 8 exactly for l = 1..4, and the total of B within
    1e-6 relative, summed in float64"""
    rgb = np.zeros((256, 256, 3), f32)
    rgb[77, 101] = 8.0
    b = B.make(levels=4, karis=False, threshold=0.0, knee=0.0, intensity=1.0)
    for f, _, ds, glow in (B.run(L, rgb, b, detail=True), B.py_run(rgb, b, detail=True)):
        for l, d in enumerate(ds, 1):
            for ch in range(3):
                assert 4 ** l * d[..., ch].sum(dtype=np.float64) == 8.0, (l, ch)
        for ch in range(3):
            assert abs(glow[..., ch].sum(dtype=np.float64) - 8.0) <= 8e-6, ch
        assert glow.max() < 8.0 and (glow > 0).sum() > 3 * 30 * 30, "the glow spills over the neighbours"


# ---- the shared layout under the host sanitizers ----

def test_the_shared_layout_runs_clean_under_the_host_sanitizers(tmp_path):
    """tests/bloom_layout_main.cpp, a program of its own over csrc/vrt_bloom.h, built with -fsanitize=address,undefined and run as a
    program: sizes, offsets and bytes against the Python restatement, every level written where the layout puts it"""
    exe = str(tmp_path / "bloom_layout_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "bloom_layout_main.cpp")], check=True)
    cases = [(w, h, l) for l in (1, 2, 5, 8) for (w, h) in ((1, 1), (2, 1), (3, 1), (1, 9), (67, 33), (257, 5), (130, 70), (1024, 768))]
    cases += [(1 << 15, 1 << 15, 8), (1 << 30, 1, 8), (1, 1 << 30, 1), (0, 1, 1), (1, 1, 0), (1, 1, 9), ((1 << 15) + 1, 1 << 15, 1), (-5, 3, 2),
              (0x7fffffff, 0x7fffffff, 8)]
    want = []
    for w, h, l in cases:
        total = B.workspace_bytes(w, h, l)
        if total == 0:
            want.append("refused")
            continue
        row, at = [f"ok {total}"], 0
        for lw, lh in B.sizes(w, h, l)[1:]:
            row.append(f"{lw} {lh} {at}")
            at += (lw * lh * 16 + 255) // 256 * 256
        want.append(" ".join(row))
    path = tmp_path / "cases.bin"
    path.write_bytes(np.array(cases, np.int32).tobytes())
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)   # the sanitizers' runtimes are linked statically: the environment as it is
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    assert run.stdout.splitlines() == want
