"""Light metering without a device (include/vrt.h vrt_meter_hdr, points E1-E9): the two struct mirrors against a compiled probe of
the header, the defaults, vrt_meter_resolve against the Python big-integer restatement and the scalar C checker (tests/oracle_meter.py)
bit for bit on the histograms that can go wrong, every refused parameter, every planted misreading of the checker caught, the exact
scaling that E2 and E6 imply, the adaptation chained over 32 frames without overshoot, and the shared inline rule (csrc/vrt_meter.h) as
a program of its own under the host sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_meter as M
from conftest import ROOT

CSRC = os.path.join(ROOT, "voxel-raytracer_amd", "csrc")
f32 = np.float32


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return M.build(tmp_path_factory.mktemp("oracle_meter"))


def hist_of(**bins):
    h = np.zeros(M.BINS, np.uint32)
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


def all_bins():
    return (1 + (np.arange(M.BINS) * 7919) % 101).astype(np.uint32)


# name -> (histogram, Meter): the histograms the issue names
CASES = {
    "empty": (hist_of(), M.make()),
    "all black": (hist_of(b0=1000), M.make()),
    "one pixel": (hist_of(b77=1), M.make(low=0, high=1000)),
    "one pixel, default window": (hist_of(b77=1), M.make()),           # a = 0, b = 0: nothing metered
    "bin 1": (hist_of(b1=12345), M.make()),
    "bin 128": (hist_of(b128=12345), M.make()),
    "bin 255": (hist_of(b255=12345), M.make()),
    "all 256 bins": (all_bins(), M.make()),
    "2^30 in one bin": (hist_of(b200=1 << 30), M.make(low=0, high=1000)),
    "2^30 in the last bin": (hist_of(b255=1 << 30), M.make(low=0, high=1000)),
    "a window that cuts through a bin": (hist_of(b10=100, b20=100, b30=100), M.make(low=250, high=750)),
    "black below the window": (hist_of(b0=600, b40=300, b90=100), M.make(low=500, high=950)),
    "low 0": (all_bins(), M.make(low=0, high=500)),
    "high 1000": (all_bins(), M.make(low=900, high=1000)),
    "low 0, high 1000": (all_bins(), M.make(low=0, high=1000)),
    "low 999, high 1000": (all_bins(), M.make(low=999, high=1000)),
    "clamped below": (hist_of(b255=10), M.make(low=0, high=1000, min_exposure=0.5)),
    "clamped above": (hist_of(b1=10), M.make(low=0, high=1000, max_exposure=4.0)),
}


def product_resolve(V, hist, m, state=None):
    return V.meter_resolve(hist, M.keys(m), state)


def same_record(got, want, what):
    assert M.bits(got) == M.bits(want), f"{what}: {got} != {want}"


# ---- the interface ----

def test_the_struct_mirrors_are_the_headers(V, tmp_path):
    """the header's text field by field, and a compiled probe of it for sizes and offsets"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrt.h")).read(), flags=re.S)
    ctypes_of = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    for name, mirrors in (("vrt_meter", (V.Meter, M.Meter)), ("vrt_exposure", (V.Exposure, M.Exposure))):
        body = re.search(r"struct\s+" + name + r"\s*\{(.*?)\}\s*;", text, flags=re.S).group(1)
        assert re.search(r"typedef\s+struct\s+" + name + r"\s+" + name + r"\s*;", text)
        fields = [(n.strip(), ctypes_of[d.split(None, 1)[0]]) for d in (d.strip() for d in body.split(";")) if d
                  for n in d.split(None, 1)[1].split(",")]
        for mirror in mirrors:
            assert fields == list(mirror._fields_), name
    assert V.METER_BINS == M.BINS == int(re.search(r"#define VRT_METER_BINS (\d+)", text).group(1))
    probe = tmp_path / "probe.c"
    rows = [f'printf("{s} %zu\\n", sizeof({s}));' for s in ("vrt_meter", "vrt_exposure")]
    rows += [f'printf("{s}.{n} %zu\\n", offsetof({s}, {n}));' for s, mirror in (("vrt_meter", V.Meter), ("vrt_exposure", V.Exposure))
             for n, _ in mirror._fields_]
    probe.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vrt.h"\nint main(void) {\n' + "\n".join(rows) + "\nreturn 0;\n}\n")
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(probe)], check=True)
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    want = {"vrt_meter": C.sizeof(V.Meter), "vrt_exposure": C.sizeof(V.Exposure)}
    for s, mirror in (("vrt_meter", V.Meter), ("vrt_exposure", V.Exposure)):
        want.update({f"{s}.{n}": getattr(mirror, n).offset for n, _ in mirror._fields_})
    assert {k: int(v) for k, v in got.items()} == want
    assert want["vrt_meter"] == 40 and want["vrt_exposure"] == 16


def test_the_defaults(V):
    m = V.Meter()
    V.hip_lib().vrt_meter_default(C.byref(m))
    made = M.make()
    for k, _ in V.Meter._fields_:
        assert getattr(m, k) == getattr(made, k), k
    assert (m.key, m.low_permille, m.high_permille, m.min_exposure, m.max_exposure, m.adapt) == (float(f32(0.18)), 500, 950, 2.0 ** -10, 2.0 ** 10, 1.0)
    assert (m.x0, m.y0, m.x1, m.y1) == (0, 0, 0, 0)
    assert V.default_meter() == M.keys(made) and set(V.default_meter()) == set(M.KEYS)
    V.hip_lib().vrt_meter_default(None)   # a NULL pointer is ignored


def test_header_declares_and_library_exports_the_eight_functions(V):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrt.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for fn in ("vrt_meter_default", "vrt_meter_resolve", "vrt_meter_hdr", "vrt_meter_hdr_host", "vrt_tonemap_hdr", "vrt_tonemap_hdr_host",
               "vrt_accum_resolve_hdr_metered", "vrt_accum_resolve_hdr_metered_device"):
        assert re.search(r"\b" + fn + r"\s*\(", text), fn
        assert fn in names and fn in V.HIP_API, fn
    blob = open(V.HIP_LIB, "rb").read()
    for kernel in (b"histogram_kernel", b"finish_kernel", b"tonemap_kernel"):
        assert re.search(rb"_ZN3vrt5meter\d+" + kernel, blob), f"no device function vrt::meter::{kernel.decode()}"


# ---- the rule ----

@pytest.mark.parametrize("name", list(CASES))
def test_resolve_is_the_big_integer_restatement_bit_for_bit(V, L, name):
    hist, m = CASES[name]
    want = M.py_resolve(hist, m)
    same_record(product_resolve(V, hist, m), want, name)
    same_record(M.resolve(L, hist, m), want, name + ": the C checker")
    # ... and as a later frame of a chain, with and without adaptation
    prev = {"exposure": 3.0, "metered": 0.25, "window": 5, "frames": 7}
    for adapt in (1.0, 0.25):
        m2 = M.make(m.key, m.low_permille, m.high_permille, m.min_exposure, m.max_exposure, adapt)
        want = M.py_resolve(hist, m2, prev)
        same_record(product_resolve(V, hist, m2, prev), want, f"{name}: frame 8, adapt {adapt}")
        same_record(M.resolve(L, hist, m2, prev), want, f"{name}: frame 8, adapt {adapt}: the C checker")


def test_what_the_cases_must_show(V):
    r = {n: product_resolve(V, *CASES[n]) for n in CASES}
    for n in ("empty", "all black", "one pixel, default window"):
        assert M.bits(r[n]) == M.bits({"exposure": 1.0, "metered": 0.0, "window": 0, "frames": 1}), n   # M = 0 on a first frame
    assert r["one pixel"]["window"] == 1
    for k in (1, 128, 255):   # every pixel in one bin: Ym is the bin's centre
        centre = np.array([((888 + k) << 20) + (1 << 19)], np.uint32).view(f32)[0]
        assert r[f"bin {k}"]["metered"] == float(centre) and r[f"bin {k}"]["window"] == 12345 * 950 // 1000 - 12345 * 500 // 1000
    assert r["bin 128"]["metered"] == 1.0625 and r["bin 255"]["metered"] == 2.0 ** 15 * 1.9375 and r["bin 1"]["metered"] == 2.0 ** -16 * 1.1875
    assert r["2^30 in one bin"]["window"] == 1 << 30 and r["2^30 in the last bin"]["metered"] == 2.0 ** 15 * 1.9375
    cut = r["a window that cuts through a bin"]   # ranks 75..225 of 300: 25 of bin 10, all of bin 20, 25 of bin 30
    assert cut["window"] == 150 and cut["metered"] == float(np.array([((888 + 20) << 20) + (1 << 19)], np.uint32).view(f32)[0])
    black = r["black below the window"]           # ranks 500..950 of 1000: 100 black ranks that count for nothing, 300 of bin 40, 50 of bin 90
    assert black["window"] == 350
    assert r["clamped below"]["exposure"] == 0.5 and r["clamped above"]["exposure"] == 4.0
    # a zeroed record with M = 0 under exposure bounds that leave 1 out
    m = M.make(min_exposure=2.0, max_exposure=8.0)
    assert product_resolve(V, hist_of(), m)["exposure"] == 2.0
    assert product_resolve(V, hist_of(), M.make(min_exposure=0.125, max_exposure=0.5))["exposure"] == 0.5
    # M = 0 on a later frame keeps the exposure, whatever adapt says, and counts the frame
    kept = product_resolve(V, hist_of(b0=5), M.make(adapt=0.5), {"exposure": 3.5, "metered": 1.0, "window": 9, "frames": 0xfffffffe})
    assert M.bits(kept) == M.bits({"exposure": 3.5, "metered": 0.0, "window": 0, "frames": 0xffffffff})
    again = product_resolve(V, hist_of(b100=5), M.make(low=0, high=1000), kept)
    assert again["frames"] == 0xffffffff, "frames saturates"


def test_random_histograms(V, L):
    rng = np.random.default_rng(11)
    for i in range(200):
        hist = np.zeros(M.BINS, np.uint32)
        n = int(rng.integers(1, 40))
        hist[rng.integers(0, M.BINS, n)] = rng.integers(0, 1 << int(rng.integers(1, 22)), n)
        low = int(rng.integers(0, 1000))
        m = M.make(float(f32(rng.uniform(0.01, 2.0))), low, int(rng.integers(low + 1, 1001)), 2.0 ** -int(rng.integers(0, 12)),
                   2.0 ** int(rng.integers(0, 12)), float(f32(rng.uniform(0.01, 1.0))))
        state = None if i % 3 == 0 else {"exposure": float(f32(rng.uniform(0.01, 50))), "metered": 0.5, "window": 3, "frames": int(rng.integers(0, 3))}
        want = M.py_resolve(hist, m, state)
        same_record(product_resolve(V, hist, m, state), want, f"case {i}")
        same_record(M.resolve(L, hist, m, state), want, f"case {i}: the C checker")


# ---- what is refused ----

def test_every_refused_parameter(V):
    lib = V.hip_lib()
    hist = all_bins()

    def call(h=hist.ctypes.data, io=True, **kw):
        m = M.make(**kw)
        e = M.Exposure()
        return lib.vrt_meter_resolve(h, C.byref(V.Meter.from_buffer_copy(bytes(m))), C.byref(V.Exposure.from_buffer_copy(bytes(e))) if io else None)

    assert call() == 0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(key=0.0), dict(key=-1.0), dict(key=nan), dict(key=inf),
               dict(low=-1), dict(low=500, high=500), dict(low=600, high=500), dict(high=1001), dict(low=1000, high=1000),
               dict(min_exposure=0.0), dict(min_exposure=-1.0), dict(min_exposure=nan), dict(min_exposure=inf, max_exposure=inf),
               dict(max_exposure=inf), dict(max_exposure=nan), dict(min_exposure=2.0, max_exposure=1.0),
               dict(adapt=0.0), dict(adapt=-0.5), dict(adapt=1.5), dict(adapt=nan)):
        assert call(**kw) == -1, kw
    assert call(min_exposure=1.0, max_exposure=1.0) == 0 and call(low=0, high=1) == 0 and call(adapt=2.0 ** -20) == 0
    assert call(h=None) == -1 and call(io=False) == -1
    over = hist_of(b3=1 << 30, b4=1)
    assert call(h=over.ctypes.data) == -1                                    # more than 2^30 pixels
    with pytest.raises(V.VrtError):
        V.meter_resolve(over)
    # the wrapper refuses the same values before the library is called
    for kw in (dict(key=0.0), dict(key=nan), dict(low_permille=-1), dict(low_permille=500, high_permille=500), dict(high_permille=1001),
               dict(low_permille=2.5), dict(min_exposure=0.0), dict(max_exposure=inf), dict(min_exposure=2.0, max_exposure=1.0),
               dict(adapt=0.0), dict(adapt=1.5), dict(adapt=True), dict(x0=-1), dict(x0=4, x1=4, y0=0, y1=2), dict(x1=3), dict(nonsense=1)):
        with pytest.raises(ValueError):
            V.meter_resolve(hist, kw)
    for bad in (np.zeros(255, np.uint32), np.zeros((2, 128), np.uint32), np.full(256, -1), np.full(256, 0.5)):
        with pytest.raises(ValueError):
            V.meter_resolve(bad)
    with pytest.raises(ValueError):
        V.meter_resolve(hist, None, {"exposure": 1.0, "other": 2})


# ---- the planted misreadings ----

def test_every_planted_misreading_is_caught(L):
    def differs(hist, m, plant, state=None):
        return M.bits(M.resolve(L, hist, m, state, plant)) != M.bits(M.py_resolve(hist, m, state))

    assert differs(*CASES["bin 128"], "centre_left_out") and differs(*CASES["all 256 bins"], "centre_left_out")
    assert differs(*CASES["black below the window"], "black_in_sums")
    assert differs(*CASES["black below the window"], "window_over_non_black")
    assert differs(CASES["bin 128"][0], M.make(adapt=0.25), "adapt_on_first_frame")
    # ... and none of them is seen where it cannot matter: the checker with a plant is the rule there
    assert not differs(*CASES["bin 128"], "black_in_sums") and not differs(*CASES["bin 128"], "window_over_non_black")
    assert not differs(*CASES["bin 128"], "adapt_on_first_frame")
    rgb = np.array([[[0.5, 2.0, 0.25], [1.0, 1.0, 1.0]]], f32)
    state = {"exposure": 0.75, "metered": 1.0, "window": 1, "frames": 1}
    assert not np.array_equal(M.tonemap(L, rgb, "clamp", 0.5, state, "tm_exposure_ignored"), M.py_tonemap(rgb, "clamp", 0.5, state))
    for op in ("clamp", "reinhard"):
        assert np.array_equal(M.tonemap(L, rgb, op, 0.5, state), M.py_tonemap(rgb, op, 0.5, state))
        assert np.array_equal(M.tonemap(L, rgb, op, 0.5, None, "tm_exposure_ignored"), M.py_tonemap(rgb, op, 0.5))


# ---- E1, E2 and E9 of the checker against the Python restatement ----

def nasty_pixels():
    """channels holding NaN, +-inf, negatives, 65504 and above, and luminances on both sides of every bin edge"""
    vals = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0, 0.0, 65504.0, 65505.0, 7e4, 1e30, 3.4e38, 1e-30, 1e-45, 2.0 ** -16, 2.0 ** -17], f32)
    rng = np.random.default_rng(5)
    odd = vals[rng.integers(0, len(vals), (300, 3))]
    edges = (np.arange(888 - 16, 888 + 257, dtype=np.uint32) << 20).view(f32)      # the first float of a bin, from two octaves below
    below = (edges.view(np.uint32) - 1).view(f32)
    grey = np.repeat(np.concatenate([edges, below]), 3).reshape(-1, 3)            # r = g = b = v: Y is v to within a rounding or two
    green = np.zeros_like(grey)
    green[:, 1] = grey[:, 1]
    return np.concatenate([odd, grey, green, (rng.random((500, 3)) * 8).astype(f32) ** 8]).astype(f32)


def test_the_checkers_luminance_bins_and_bytes_are_the_python_restatement(L):
    px = nasty_pixels()
    y = np.array([L.o_meter_luminance(*map(float, p)) for p in px], f32)
    assert np.array_equal(y.view(np.uint32), M.py_luminance(px).view(np.uint32))
    assert np.isfinite(y).all() and (y >= 0).all() and not np.signbit(y).any() and y.max() == 65504.0
    k = np.array([L.o_meter_bin(float(v)) for v in y])
    assert np.array_equal(k, M.py_bins(y)) and k.min() == 0 and k.max() == 255
    assert L.o_meter_bin(float(L.o_meter_luminance(65504.0, 65504.0, 65504.0))) == 255       # E2: the largest Y lands in the last bin
    assert L.o_meter_bin(float(f32(2.0 ** -16 * 1.125))) == 1 and L.o_meter_bin(float(np.nextafter(f32(2.0 ** -16 * 1.125), f32(0)))) == 0
    img = px[:len(px) // 7 * 7].reshape(7, -1, 3)
    assert M.histogram(L, img).tolist() == M.py_histogram(img)
    rect = (3, 1, img.shape[1] - 5, 6)
    assert M.histogram(L, img, rect).tolist() == M.py_histogram(img, rect)
    assert len(set(np.nonzero(M.histogram(L, img))[0])) == 256, "the pixels fill every bin"
    for op in ("clamp", "reinhard"):
        for state in (None, {"exposure": 0.37, "metered": 1.0, "window": 1, "frames": 1}, {"exposure": 3e38, "metered": 1.0, "window": 1, "frames": 1}):
            assert np.array_equal(M.tonemap(L, img, op, 1.7, state), M.py_tonemap(img, op, 1.7, state)), (op, state)


# ---- exact scaling ----

def test_scaling_by_a_power_of_two_is_exact(V, L):
    """E2, E6: an image scaled by 2^j shifts every bin by 8 j, makes Ym exactly 2^j times larger and e* exactly 2^-j times, where no
    clamp of h, bin 0 or the exposure range is met"""
    rng = np.random.default_rng(3)
    img = (2.0 ** rng.uniform(-6, 4, (24, 31, 3))).astype(f32)
    m = M.make(low=100, high=900)
    base_hist = M.histogram(L, img)
    base = product_resolve(V, base_hist, m)
    assert base["window"] > 0 and 2.0 ** -7 < base["metered"] < 2.0 ** 5
    for j in (-5, -2, -1, 1, 3, 6):
        scaled = (img * f32(2.0 ** j)).astype(f32)
        hist = M.histogram(L, scaled)
        assert hist.tolist() == M.py_histogram(scaled)
        assert np.array_equal(hist, np.roll(base_hist, 8 * j)) and hist.sum() == base_hist.sum(), j
        r = product_resolve(V, hist, m)
        assert r["metered"] == base["metered"] * 2.0 ** j and r["exposure"] == base["exposure"] * 2.0 ** -j and r["window"] == base["window"], j


# ---- adaptation ----

@pytest.mark.parametrize("adapt", (0.25, 0.5, 0.03125, 0.7))
def test_chained_records_are_the_checkers_and_never_overshoot(V, L, adapt):
    rng = np.random.default_rng(int(adapt * 1000))
    m = M.make(low=0, high=1000, adapt=adapt)
    got = want = py = None
    for frame in range(32):
        hist = np.zeros(M.BINS, np.uint32)
        hist[int(rng.integers(1, 256))] = 1000       # the scene jumps by octaves from frame to frame
        hist[int(rng.integers(1, 256))] += 500
        if frame in (9, 20):
            hist[:] = 0
            hist[0] = 77                             # a black frame keeps the exposure
        target = M.py_resolve(hist, M.make(low=0, high=1000), py)["exposure"]   # e*: the same frame without adaptation
        prev = None if py is None else py["exposure"]
        got, want, py = product_resolve(V, hist, m, got), M.resolve(L, hist, m, want), M.py_resolve(hist, m, py)
        same_record(got, py, f"frame {frame}")
        same_record(want, py, f"frame {frame}: the C checker")
        e = got["exposure"]
        if prev is None:
            assert e == target
        else:
            assert prev <= e <= target or target <= e <= prev, (frame, prev, e, target)
        assert got["frames"] == frame + 1


# ---- the shared inline rule under the host sanitizers ----

def test_the_shared_rule_runs_clean_under_the_host_sanitizers(tmp_path):
    """tests/meter_resolve_main.cpp, a program of its own over csrc/vrt_meter.h, built with -fsanitize=address,undefined and run as a
    program on the histograms above, chained a second time with adaptation, and on one whose counts sum past 2^30"""
    exe = str(tmp_path / "meter_resolve_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "meter_resolve_main.cpp")], check=True)
    cases, want = [], []
    for name, (hist, m) in CASES.items():
        first = M.py_resolve(hist, m)
        m2 = M.make(m.key, m.low_permille, m.high_permille, m.min_exposure, m.max_exposure, 0.25)
        cases += [(hist, m, M.Exposure()), (np.roll(hist, 3), m2, M.from_record(first))]
        want += ["ok %u %u %u %u" % M.bits(first), "ok %u %u %u %u" % M.bits(M.py_resolve(np.roll(hist, 3), m2, first))]
    cases.append((hist_of(b3=1 << 30, b4=1), M.make(), M.Exposure()))
    want.append("refused")
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for hist, m, e in cases:
            f.write(np.ascontiguousarray(hist, np.uint32).tobytes() + bytes(m) + bytes(e))
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)   # the sanitizers' runtimes are linked statically: the environment as it is
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    assert run.stdout.splitlines() == want
