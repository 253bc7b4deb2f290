"""Emitter importance (include/vrt.h vrt_set_emitter_importance, VRT_EMIT_POWER): what holds without a GPU. The host's weights and
thresholds are a Python big-integer restatement's, up to weights in the 2^57 range; the checker (tests/oracle_paths.c through oracle_emit_power) is
oracle_emit at mode 0 and oracle_sun with an empty list, bit for bit; at mode 1 its log shows the rule's tick, emitter, visible
faces, point and weight; the estimator has the expectation of the uniform one and of sampling off at less variance than the uniform
one, and a planted misreading of the weight fails that test; the host's table code runs clean under the host sanitizers as a program
of its own. The kernels are held to the checker on the MI355X (test_gpu_emit_power.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import emit_power_worlds as pw
import emit_worlds as ew
import oracle_emit as oe
import oracle_emit_power as op
import oracle_rays
import oracle_sun as osun
from conftest import ROOT
from test_sun_disc import _stream

F = np.float32
W, H = pw.W, pw.H
SAMPLE = 5
CSRC = os.path.join(ROOT, "voxel-raytracer_amd", "csrc")


@pytest.fixture(scope="module")
def P(tmp_path_factory):
    return op.build(tmp_path_factory.mktemp("oracle_emit_power"))


@pytest.fixture(scope="module")
def E(tmp_path_factory):
    return oe.build(tmp_path_factory.mktemp("oracle_emit"))


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    return osun.build(tmp_path_factory.mktemp("oracle_sun"))


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_rays"))


def _scene(O, V, world, pose=pw.POSE):
    tex, dim = world.flatten()
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    return O.make_scene(tex, dim, ip, iv, cp)


@pytest.fixture(scope="module")
def room(O, V, R):
    """the fixture with its pane -> (scene, frame origins, frame dirs, list, weights uint64, thresholds uint32)"""
    w = pw.room(V)
    s = _scene(O, V, w)
    lst, words = op.walk(w.records()[0])
    w.close()
    wt = op.weights(lst, words)
    return (s,) + oracle_rays.frame_rays(R, s, W, H) + (lst, np.array(wt, np.uint64), np.array(op.thresholds(wt), np.uint32))


# ---- the fixture ----

def test_the_fixture_holds_257_emitters_and_the_lamp_most_of_the_power(room):
    lst, wt, T = room[3:]
    assert len(lst) == pw.N_EMITTERS == 257 and lst.tolist() == pw.expected_list()
    assert (len(lst) - 1).bit_length() == 9, "nine search steps"
    lamp = int(np.argmax(lst[:, 3]))
    assert lst[lamp].tolist() == list(pw.LAMP[0]) + [4]
    assert 2 * int(wt[lamp]) > int(wt.sum()), f"the lamp holds {int(wt[lamp])} of {int(wt.sum())}"
    assert len(set(wt.tolist())) > 100, "the panel's weights vary"


# ---- thresholds ----

def _host_cdf(V, records, world_min=(-1023, -1023, -1023), world_max=(1024, 1024, 1024), max_entries=1 << 20):
    T = V.test_lib()
    T.vrt_test_emitter_cdf.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t]
    T.vrt_test_emitter_cdf.restype = C.c_long
    rec = np.ascontiguousarray(records, np.uint32)
    mn, mx = np.array(world_min, np.int32), np.array(world_max, np.int32)
    n = T.vrt_test_emitter_cdf(rec.ctypes.data, len(rec), mn.ctypes.data, mx.ctypes.data, max_entries, None, None, 0)
    assert n >= 0
    wt, cdf = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    if n:
        assert T.vrt_test_emitter_cdf(rec.ctypes.data, len(rec), mn.ctypes.data, mx.ctypes.data, max_entries, wt.ctypes.data, cdf.ctypes.data, n) == n
    return wt, cdf


def _host_cdf_list(V, lst, words):
    T = V.test_lib()
    T.vrt_test_emitter_cdf_list.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    T.vrt_test_emitter_cdf_list.restype = C.c_long
    lst, words = np.ascontiguousarray(lst, np.int32), np.ascontiguousarray(words, np.uint32)
    n = len(lst)
    wt, cdf = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    assert T.vrt_test_emitter_cdf_list(lst.ctypes.data, words.ctypes.data, n, wt.ctypes.data, cdf.ctypes.data) == n
    return wt, cdf


def _check_table(cdf, what):
    c = cdf.astype(np.int64)
    assert c[-1] == 1 << 24, f"{what}: the last threshold is {c[-1]}"
    assert c[0] >= 1 and np.all(np.diff(c) >= 1), f"{what}: not strictly increasing"


def _big_list():
    """2^20 leaves of size 1024, every fourth one black (tests/emit_cdf_main.cpp's first case): the sum of weights is in the 2^57 range"""
    n = 1 << 20
    lst = np.zeros((n, 4), np.int32)
    lst[:, 0] = np.arange(n)
    lst[:, 3] = 1024
    words = np.zeros((n, 2), np.uint32)
    words[:, 0] = np.where(np.arange(n) % 4 == 3, 0xff000000, 0xffffffff)
    words[:, 1] = 0x0000ffff
    return lst, words


def test_host_weights_and_thresholds_are_the_big_integer_restatement(V, P):
    worlds = {"fixture": pw.room(V), "lamp room": ew.lamp_room(V)}
    one = V.World()
    one.insert(3, 4, 5, 0x102030ff, 3.0, 0.5, 0.0)
    worlds["N = 1"] = one
    black = V.World()
    for i in range(5):   # emitters whose colour is black: every weight 0, the equal split
        black.insert(2 * i, 1, 7, 0x000000ff, 3.0, (i + 1) / 255.0, 0.0)
    worlds["all black"] = black
    for name, w in worlds.items():
        rec = w.records()[0]
        w.close()
        lst, words = op.walk(rec)
        want_w = op.weights(lst, words)
        want_t = op.thresholds(want_w)
        got_w, got_t = _host_cdf(V, rec)
        assert got_w.tolist() == want_w, f"{name}: weights"
        assert got_t.tolist() == want_t, f"{name}: thresholds"
        assert op.checker_thresholds(P, got_w).tolist() == want_t, f"{name}: the checker's own table"
        _check_table(got_t, name)
        n = len(lst)
        if name == "all black":
            assert n == 5 and not any(want_w) and want_t == [(j + 1) * (1 << 24) // 5 for j in range(5)]
        if name == "N = 1":
            assert want_t == [1 << 24]
        if name == "lamp room":
            assert n == 4
    # weights in the 2^57 range, through the host functions on a list
    lst, words = _big_list()
    want_w = op.weights(lst[:8], words[:8])
    assert want_w[0] == 1024 * 1024 * 255 * 765 and want_w[3] == 0
    want_w = want_w[:4] * (len(lst) // 4)
    assert 1 << 57 <= sum(want_w) < 1 << 58
    want_t = op.thresholds(want_w)
    got_w, got_t = _host_cdf_list(V, lst, words)
    assert got_w.tolist() == want_w and got_t.tolist() == want_t, "2^20 leaves of size 1024"
    assert op.checker_thresholds(P, got_w).tolist() == want_t
    _check_table(got_t, "2^20 leaves of size 1024")
    assert np.all(np.diff(np.concatenate([[0], got_t.astype(np.int64)]))[3::4] == 1), "a black emitter holds one tick"


# ---- the checker at mode 0 and with an empty list ----

@pytest.mark.parametrize("D", (1, 3))
@pytest.mark.parametrize("radius", (0.0, 0.05))
def test_mode_0_is_oracle_emit_and_an_empty_list_is_oracle_sun_bit_for_bit(P, E, S, room, D, radius):
    s, o, d, lst, wt, _ = room
    for k in (0, 5):
        ref = oe.shade(E, s, o, d, D, radius, lst, width=W, sample=k)
        sun = osun.shade(S, s, o, d, D, radius, width=W, sample=k)
        for what, got, want in (("mode 0", op.shade(P, s, o, d, D, radius, lst, wt, op.UNIFORM, width=W, sample=k), ref),
                                ("mode 0 without weights", op.shade(P, s, o, d, D, radius, lst, None, op.UNIFORM, width=W, sample=k), ref),
                                ("an empty list at mode 0", op.shade(P, s, o, d, D, radius, None, None, op.UNIFORM, width=W, sample=k), sun),
                                ("an empty list at mode 1", op.shade(P, s, o, d, D, radius, None, None, op.POWER, width=W, sample=k), sun)):
            assert np.array_equal(got[0], want[0]), f"{what} D={D} radius {radius} sample {k} rgba8"
            assert np.array_equal(got[1], want[1]), f"{what} D={D} radius {radius} sample {k} id_dist"
            assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), f"{what} D={D} radius {radius} sample {k} float bits"
    # the log of mode 0 is oracle_emit's, field for field
    ref = oe.shade(E, s, o, d, D, radius, lst, width=W, sample=SAMPLE, log=True)[3]
    got = op.shade(P, s, o, d, D, radius, lst, wt, op.UNIFORM, width=W, sample=SAMPLE, log=True)[3]
    assert len(ref) == len(got)
    for name in ref.dtype.names:
        assert np.array_equal(ref[name].view(np.uint32), got[name].view(np.uint32)), f"log field {name}"
    assert not np.any(got["t"]) and not np.any(got["ticks"]) and not np.any(got["m"])


# ---- the log against the contract ----

@pytest.mark.parametrize("D", (1, 3))
@pytest.mark.parametrize("radius", (0.0, 0.05))
def test_log_shows_the_rule(P, room, D, radius):
    s, o, d, lst, wt, T = room
    Tl = np.concatenate([[0], T.astype(np.int64)])
    rgba, idd, rgb, log = op.shade(P, s, o, d, D, radius, lst, wt, op.POWER, width=W, sample=SAMPLE, log=True)
    direct = log[log["kind"] == op.DIRECT]
    assert len(direct) > 1000
    assert not np.any(log["kind"] == op.EMIT), "a ray of depth >= 1 added an emissive term with sampling on"
    assert np.any(log["kind"] == op.EMIT0), "no pixel sees an emitter directly"
    sun = 2 if radius > 0.0 else 0
    used = {}
    marched = contributed = none_visible = 0
    m_seen = set()
    picked = set()
    for v in direct:
        ray = int(v["ray"])
        at = used.get(ray, 0)
        draws = _stream(ray % W, ray // W, SAMPLE, at + sun + 6)[at:]
        if sun:
            assert (v["u1"], v["u2"]) == tuple(draws[:2]), f"ray {ray}: the sun's draws at {at}"
        assert (v["u0"], v["uf"], v["ua"], v["ub"]) == tuple(draws[sun:sun + 4]), f"ray {ray}: the four draws at {at + sun}"
        assert (v["rx"], v["ry"]) == tuple(draws[sun + 4:]), f"ray {ray}: the bounce's draws at {at + sun + 4}"
        used[ray] = at + sun + 6
        # (1) the tick, the emitter and its ticks, in float32 and exact integers
        t = min(int(F(v["u0"] * F(16777216.0))), 16777215)
        j = int(np.searchsorted(T, t, side="right"))
        ticks = int(Tl[j + 1] - Tl[j])
        assert (int(v["t"]), int(v["j"]), int(v["ticks"])) == (t, j, ticks), f"ray {ray}: tick, emitter and ticks"
        assert Tl[j] <= t < Tl[j + 1]
        picked.add(j)
        p = F(F(ticks) * F(2.0 ** -24))
        # (2) the faces x sees, in axis order
        lo, sz = lst[j, :3], F(lst[j, 3])
        faces = []
        for k in range(3):
            if v["x"][k] < F(lo[k]):
                faces.append(2 * k)
            elif v["x"][k] > F(F(lo[k]) + sz):
                faces.append(2 * k + 1)
        m = len(faces)
        assert int(v["m"]) == m, f"ray {ray}: m"
        m_seen.add(m)
        if m == 0:
            none_visible += 1
            assert v["conn_steps"] == 0 and v["conn_hit"] == 0 and v["g"] == 0.0 and not np.any(v["E"]) and not np.any(v["q"]), f"ray {ray}: m == 0"
            continue
        f = faces[min(int(F(v["uf"] * F(m))), m - 1)]
        assert int(v["f"]) == f, f"ray {ray}: face"
        ax, side = f >> 1, f & 1
        q = np.zeros(3, F)
        q[ax] = F(lo[ax]) + (sz if side else F(0.0))
        q[(ax + 1) % 3] = F(lo[(ax + 1) % 3]) + F(v["ua"] * sz)
        q[(ax + 2) % 3] = F(lo[(ax + 2) % 3]) + F(v["ub"] * sz)
        assert np.array_equal(q.view(np.uint32), v["q"].view(np.uint32)), f"ray {ray}: q {v['q']} against {q}"
        # (3) nothing is marched below either horizon
        if not (v["cs"] > 0.0 and v["cl"] > 0.0):
            assert v["conn_steps"] == 0 and v["conn_hit"] == 0 and v["g"] == 0.0 and not np.any(v["E"]), f"ray {ray}: marched at cs {v['cs']} cl {v['cl']}"
        else:
            assert v["conn_steps"] > 0
            marched += 1
        if v["in_box"]:
            assert v["conn_hit"] == 1
            g = F(F(F(v["cs"] * v["cl"]) * F(F(m) * F(sz * sz))) / F(F(F(3.14159265359) * v["r2"]) * p))
            assert g.view(np.uint32) == v["g"].view(np.uint32), f"ray {ray}: g {v['g']} against {g}"
            assert np.all(v["E"] > 0.0)
            contributed += 1
        else:
            assert v["g"] == 0.0 and not np.any(v["E"])
    print(f"D={D} radius {radius}: {len(direct)} shadowing vertices, {none_visible} see no face, {marched} connections marched, "
          f"{contributed} contributed, {len(picked)} emitters picked")
    assert contributed > 100 and marched >= contributed
    assert m_seen >= {1, 2, 3}, f"visible-face counts seen: {sorted(m_seen)}"
    assert len(picked) > 50, "the panel is picked too"
    other = log[log["kind"] != op.DIRECT]
    assert not np.any(other["u0"]) and not np.any(other["q"]) and not np.any(other["E"]) and not np.any(other["ticks"])
    # the float colour is the sum of the logged contributions (tests/test_emitters.py's bound)
    want = op.restate(log, W * H, s.global_light)
    scale = np.maximum(np.abs(want).max(axis=1), np.finfo(np.float32).tiny)
    err = np.abs(rgb.astype(np.float64) - want).max(axis=1) / scale
    print(f"largest relative difference to the restated sum {err.max():.3g}, {len(log)} contributions")
    assert err.max() <= 1e-5
    # and what does not move: (voxel ID, dist)
    assert np.array_equal(idd, op.shade(P, s, o, d, D, radius, None, None, op.UNIFORM, width=W, sample=SAMPLE)[1])


# ---- the same expectation, less variance ----

K = 16384
Z = 4.5   # tests/test_emitters.py's bound


def _within(a, b):
    """per ray and channel |mean_a - mean_b| <= Z sqrt((var_a + var_b) / K) -> (all within, largest |z|)"""
    (m_a, v_a), (m_b, v_b) = a, b
    se = np.sqrt((v_a + v_b) / K)
    z = np.abs(m_a - m_b) / np.maximum(se, 1e-300)
    return bool(np.all(np.abs(m_a - m_b) <= Z * se)), float(z.max())


def test_power_has_the_expectation_of_uniform_and_of_off_at_less_variance(P, O, V):
    """The fixture without its pane; 16 rays from (36.5, 44.5, 50.5), K = 16384 samples, D in {1, 2}; per ray and channel the means of
    power and uniform, and of power and sampling off, differ by at most 4.5 standard errors of the difference (the run's own sample
    variances); the summed sample variance of power is below that of uniform. The planted misreadings (6 in m's place; p left out)
    fail the same test."""
    w = pw.room(V, pane=False)
    s = _scene(O, V, w)
    lst, words = op.walk(w.records()[0])
    w.close()
    assert len(lst) == 257
    wt = np.array(op.weights(lst, words), np.uint64)
    o, d = pw.probe_rays()

    def run(D, emitters, mode, debug=0):
        rgb = np.stack([op.shade(P, s, o, d, D, 0.0, emitters, wt if emitters is not None else None, mode, sample=k, debug=debug)[2]
                        for k in range(K)]).astype(np.float64)
        return rgb.mean(axis=0), rgb.var(axis=0, ddof=1)

    for D in (1, 2):
        off = run(D, None, op.UNIFORM)
        uni = run(D, lst, op.UNIFORM)
        pwr = run(D, lst, op.POWER)
        ok_u, z_u = _within(pwr, uni)
        ok_o, z_o = _within(pwr, off)
        ratio = uni[1].sum() / pwr[1].sum()
        print(f"D={D}: max |z| power against uniform {z_u:.2f}, against off {z_o:.2f}; summed variance off {off[1].sum():.4g}, "
              f"uniform {uni[1].sum():.4g}, power {pwr[1].sum():.4g}: uniform / power {ratio:.1f}")
        assert ok_u, f"D={D}: power against uniform, max |z| {z_u:.2f}"
        assert ok_o, f"D={D}: power against sampling off, max |z| {z_o:.2f}"
        assert pwr[1].sum() < uni[1].sum(), f"D={D}: variance power {pwr[1].sum()} uniform {uni[1].sum()}"
        if D == 1:   # the test can tell: a misread weight is caught by the same bound
            for debug, what in ((1, "6 in m's place"), (2, "p left out")):
                ok, z = _within(run(D, lst, op.POWER, debug), uni)
                print(f"D={D} planted misreading ({what}): max |z| against uniform {z:.2f}")
                assert not ok, f"the expectation test does not catch the misreading '{what}' (max |z| {z:.2f})"


# ---- the interface ----

def test_header_declares_and_library_exports_the_functions_and_constants(V):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrt.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert re.search(r"\bint\s+vrt_set_emitter_importance\s*\(\s*vrt_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)", text)
    assert re.search(r"\blong\s+vrt_emitter_cdf\s*\(\s*vrt_ctx\s*\*\s*\w*\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\)", text)
    assert re.search(r"#define\s+VRT_EMIT_UNIFORM\s+0\b", text) and re.search(r"#define\s+VRT_EMIT_POWER\s+1\b", text)
    assert (V.EMIT_UNIFORM, V.EMIT_POWER) == (0, 1)
    L = C.CDLL(V.HIP_LIB)
    for name in ("vrt_set_emitter_importance", "vrt_emitter_cdf"):
        assert name in names and hasattr(L, name), f"libvrt_hip.so does not export {name}"


def test_hip_code_object_holds_the_power_kernels(V):
    """the kernels of VRT_EMIT_POWER are instantiations over EmitPowerPaths<...> (csrc/vrt_common.hip.h), for both traversals"""
    blob = open(V.HIP_LIB, "rb").read()
    assert b"gfx950" in blob
    names = set(re.findall(rb"_ZN3vrt[0-9A-Za-z_]*EmitPowerPaths[0-9A-Za-z_]*", blob))
    for kernel in (b"full_accum_kernel", b"shade_rays_full_kernel"):
        for trav in (b"v4", b"v1"):
            assert any(kernel in n and b"EmitPowerPathsINS_2" + trav in n for n in names), f"no {kernel.decode()} over EmitPowerPaths<{trav.decode()}::...>"


def test_wrapper_refuses_other_values_without_touching_the_library(V):
    class Fake(V.Context):
        def __init__(self):   # no device: the checks under test come before the library is called
            self._h = None
    c = Fake()
    assert c.emitter_importance == V.EMIT_UNIFORM
    for bad in (2, -1, "1", None, 0.5, [1], True):
        with pytest.raises(ValueError):
            c.set_emitter_importance(bad)
    assert c.emitter_importance == V.EMIT_UNIFORM


# ---- the host's table code under the host sanitizers ----

def _fnv(cdf):
    h = 1469598103934665603
    for b in np.asarray(cdf, "<u4").tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_host_table_code_runs_clean_under_the_host_sanitizers(tmp_path):
    """tests/emit_cdf_main.cpp, a program of its own over csrc/vrt_emitters.h, built with -fsanitize=address,undefined and run as a
    program: 2^20 weights summing into the 2^57 range, the all-black split at N = 2^20, a walked tree"""
    exe = str(tmp_path / "emit_cdf_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "emit_cdf_main.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)   # the sanitizers' runtimes are linked statically: the environment as it is
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    rows = {r.split()[0]: [int(x) for x in r.split()[1:]] for r in run.stdout.splitlines()}
    lst, words = _big_list()
    n = len(lst)
    big_w = op.weights(lst[:4], words[:4]) * (n // 4)
    cases = {"big": big_w, "black": [0] * n, "walk": [1 * 0x20 * (0x30 + 0x20 + 0x10), 1 * 0xff * 0xff]}
    for name, wts in cases.items():
        T = op.thresholds(wts)
        assert rows[name] == [len(T), sum(wts), T[0], T[len(T) // 2], T[-1], _fnv(T)], f"{name}: {rows[name]}"
