"""Emitter sampling (include/vrt.h vrt_set_emitter_sampling): what holds without a GPU. The checker (tests/oracle_paths.c through oracle_emit: oracle_sun's
loop with the rule applied at the shadowing vertices and at the emissive hits of depth >= 1) is oracle_sun with an empty list; its log
shows the rule's draws, emitter, face, point and cosines; its float colour is the sum of the contributions it logs; the estimator with
sampling on has the expectation of the one with sampling off, at a fraction of its variance; and the host's list builder gives the
list of a Python walk. The kernels are held to the checker on the MI355X (test_gpu_emitters.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import emit_worlds as ew
import oracle_emit as oe
import oracle_rays
import oracle_sun as osun
import sun_worlds as sw
from conftest import ROOT
from test_sun_disc import _stream

F = np.float32
W, H = ew.W, ew.H
SAMPLE = 5


@pytest.fixture(scope="module")
def E(tmp_path_factory):
    return oe.build(tmp_path_factory.mktemp("oracle_emit"))


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    return osun.build(tmp_path_factory.mktemp("oracle_sun"))


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_rays"))


def _scene(O, V, world, pose=ew.POSE):
    tex, dim = world.flatten()
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    return O.make_scene(tex, dim, ip, iv, cp)


@pytest.fixture(scope="module")
def room(O, V, R):
    """the lamp room with the pane -> (scene, frame origins, frame dirs, emitter list by the Python walk)"""
    w = ew.lamp_room(V)
    s = _scene(O, V, w)
    lst = oe.walk(w.records()[0])
    w.close()
    return (s,) + oracle_rays.frame_rays(R, s, W, H) + (lst,)


# ---- an empty list is oracle_sun ----

@pytest.mark.parametrize("world", sw.WORLDS)
@pytest.mark.parametrize("D", (1, 3))
@pytest.mark.parametrize("radius", (0.0, 0.05))
def test_an_empty_list_is_oracle_sun_bit_for_bit(E, S, R, O, V, product_scenes, world, D, radius):
    s = sw.scenes(O, V, product_scenes)[world][3]
    o, d = oracle_rays.frame_rays(R, s, W, H)
    for k in (0, 5):
        ref = osun.shade(S, s, o, d, D, radius, width=W, sample=k)
        for lst in (None, np.zeros((0, 4), np.int32)):
            got = oe.shade(E, s, o, d, D, radius, lst, width=W, sample=k)
            assert np.array_equal(got[0], ref[0]), f"{world} D={D} radius {radius} sample {k} rgba8"
            assert np.array_equal(got[1], ref[1]), f"{world} D={D} radius {radius} sample {k} id_dist"
            assert np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32)), f"{world} D={D} radius {radius} sample {k} float bits"


# ---- the log against the contract ----

def test_the_lamp_room_holds_a_merged_lamp_and_three_singles(room):
    lst = room[3]
    assert lst.tolist() == sorted([list(ew.LAMP[0]) + [2]] + [list(p) + [1] for p, _ in ew.SINGLES])


@pytest.mark.parametrize("D", (1, 3))
@pytest.mark.parametrize("radius", (0.0, 0.05))
def test_log_shows_the_rule(E, room, D, radius):
    s, o, d, lst = room
    N = len(lst)
    rgba, idd, rgb, log = oe.shade(E, s, o, d, D, radius, lst, width=W, sample=SAMPLE, log=True)
    direct = log[log["kind"] == oe.DIRECT]
    assert len(direct) > 1000
    # (7) no depth >= 1 emissive contribution; the depth-0 one stays
    assert not np.any(log["kind"] == oe.EMIT), "a ray of depth >= 1 added an emissive term with sampling on"
    assert np.any(log["kind"] == oe.EMIT0), "no pixel sees an emitter directly"
    assert np.any(log["kind"] == oe.GLASS) or np.any(direct["chain"] > 1), "the pane is not in the picture"
    sun = 2 if radius > 0.0 else 0
    used = {}
    marched = contributed = 0
    for v in direct:
        ray = int(v["ray"])
        at = used.get(ray, 0)
        draws = _stream(ray % W, ray // W, SAMPLE, at + sun + 6)[at:]
        if sun:
            assert (v["u1"], v["u2"]) == tuple(draws[:2]), f"ray {ray}: the sun's draws at {at}"
        else:
            assert v["u1"] == 0.0 and v["u2"] == 0.0
        assert (v["u0"], v["uf"], v["ua"], v["ub"]) == tuple(draws[sun:sun + 4]), f"ray {ray}: the four draws at {at + sun}"
        assert (v["rx"], v["ry"]) == tuple(draws[sun + 4:]), f"ray {ray}: the bounce's draws at {at + sun + 4}"
        used[ray] = at + sun + 6
        # (2) j, f and q follow from them, in float32
        j = min(int(F(v["u0"] * F(N))), N - 1)
        f = min(int(F(v["uf"] * F(6.0))), 5)
        assert (int(v["j"]), int(v["f"])) == (j, f), f"ray {ray}: emitter and face"
        ax, side = f >> 1, f & 1
        lo, sz = lst[j, :3], F(lst[j, 3])
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
            area = F(F(F(N) * F(6.0)) * F(sz * sz))
            g = F(F(F(v["cs"] * v["cl"]) * area) / F(F(3.14159265359) * v["r2"]))
            assert g.view(np.uint32) == v["g"].view(np.uint32), f"ray {ray}: g {v['g']} against {g}"
            assert np.all(v["E"] > 0.0)
            contributed += 1
        else:
            assert v["g"] == 0.0 and not np.any(v["E"])
    print(f"D={D} radius {radius}: {len(direct)} shadowing vertices, {marched} connections marched, {contributed} contributed")
    assert contributed > 100 and marched > contributed
    other = log[log["kind"] != oe.DIRECT]
    assert not np.any(other["u0"]) and not np.any(other["q"]) and not np.any(other["E"])
    # the float colour is the sum of the logged contributions (tests/test_sun_disc.py's bound)
    want = oe.restate(log, W * H, s.global_light)
    scale = np.maximum(np.abs(want).max(axis=1), np.finfo(np.float32).tiny)
    err = np.abs(rgb.astype(np.float64) - want).max(axis=1) / scale
    print(f"largest relative difference to the restated sum {err.max():.3g}, {len(log)} contributions")
    assert err.max() <= 1e-5
    # and what does not move: (voxel ID, dist)
    assert np.array_equal(idd, oe.shade(E, s, o, d, D, radius, None, width=W, sample=SAMPLE)[1])


# ---- the same expectation ----

def test_sampling_on_has_the_expectation_of_sampling_off(E, O, V):
    """The lamp room without the pane and the three singles; 16 rays from (36.5, 44.5, 50.5), K = 16384 samples, D in {1, 2, 3};
    per ray and channel |mean_on - mean_off| <= 4.5 sqrt((var_on + var_off) / K) with the run's own sample variances, for the lamp
    as one size-2 box and as eight size-1 boxes; the summed sample variance with sampling on is below that with sampling off."""
    K = 16384
    w = ew.lamp_room(V, pane=False, singles=False)
    s = _scene(O, V, w)
    walked = oe.walk(w.records()[0])
    w.close()
    assert walked.tolist() == ew.lamp_list(1).tolist()
    o, d = ew.probe_rays()

    def run(D, lst):
        rgb = np.stack([oe.shade(E, s, o, d, D, 0.0, lst, sample=k)[2] for k in range(K)]).astype(np.float64)
        return rgb.mean(axis=0), rgb.var(axis=0, ddof=1)

    for D in (1, 2, 3):
        m_off, v_off = run(D, None)
        assert m_off[0, 0] == 10.0 and not v_off[0].any(), "ray 0 sees the lamp: its red channel is 10.0 in every sample"
        for boxes in (1, 8):
            m_on, v_on = run(D, ew.lamp_list(boxes))
            assert np.array_equal(m_on[0], m_off[0]), "the ray that sees the lamp is the depth-0 term in both estimators"
            z = np.abs(m_on - m_off) / np.maximum(np.sqrt((v_on + v_off) / K), 1e-300)
            ratio = v_off.sum() / v_on.sum()
            print(f"D={D} {boxes} box(es): max |z| {z.max():.2f}, summed variance off / on {ratio:.1f}")
            assert np.all(np.abs(m_on - m_off) <= 4.5 * np.sqrt((v_on + v_off) / K)), f"D={D} {boxes} box(es): max |z| {z.max():.2f}"
            assert v_on.sum() < v_off.sum(), f"D={D} {boxes} box(es): variance on {v_on.sum()} off {v_off.sum()}"


# ---- the host's list builder ----

def _host_list(V, records, world_min=(-1023, -1023, -1023), world_max=(1024, 1024, 1024), max_entries=1 << 20, cap=None):
    T = V.test_lib()
    T.vrt_test_emitter_list.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]
    T.vrt_test_emitter_list.restype = C.c_long
    rec = np.ascontiguousarray(records, np.uint32)
    mn, mx = np.array(world_min, np.int32), np.array(world_max, np.int32)
    n = T.vrt_test_emitter_list(rec.ctypes.data, len(rec), mn.ctypes.data, mx.ctypes.data, max_entries, None, 0)
    assert n >= 0
    out = np.zeros((n if cap is None else cap, 4), np.int32)
    got = T.vrt_test_emitter_list(rec.ctypes.data, len(rec), mn.ctypes.data, mx.ctypes.data, max_entries, out.ctypes.data if len(out) else None, len(out))
    assert got == n
    return n, out


def test_host_list_builder_is_the_python_walk(V):
    # the lamp room: membership, sizes (the merged lamp is one entry of size 2), order
    w = ew.lamp_room(V)
    rec = w.records()[0]
    w.close()
    n, got = _host_list(V, rec)
    want = oe.walk(rec)
    assert n == 4 and np.array_equal(got, want)
    assert got.tolist() == sorted(got.tolist()) and [ew.LAMP[0][0], ew.LAMP[0][1], ew.LAMP[0][2], 2] in got.tolist()
    # record order does not matter: the same world inserted in another order, and cut short by the caller's capacity
    assert _host_list(V, rec, cap=2)[1].tolist() == want[:2].tolist()
    assert _host_list(V, rec, max_entries=3)[0] == 4 and not np.any(_host_list(V, rec, max_entries=3, cap=4)[1]), "above max_entries nothing is kept"
    # an emitter with alpha 0 is not listed
    w = ew.lamp_room(V, lamp_alpha=0)
    rec = w.records()[0]
    w.close()
    n, got = _host_list(V, rec)
    assert n == 3 and np.array_equal(got, oe.walk(rec)) and np.all(got[:, 3] == 1)
    # an emitter at the world's minimum corner, and bounds that are no power of two
    for mn, mx in (((0, 0, 0), (64, 64, 64)), ((-3, -3, -3), (10, 10, 10)), ((-1023, -1023, -1023), (1024, 1024, 1024))):
        w = V.World(mn, mx)
        w.insert(mn[0], mn[1], mn[2], 0xffffffff, 3.0, 0.5, 0.0)
        w.insert(mx[0] - 1, mx[1] - 1, mx[2] - 1, 0xffffffff, 3.0, 0.0, 0.0)   # not an emitter
        w.insert(mn[0] + 2, mn[1] + 1, mn[2] + 3, 0x10203040, 1.5, 1.0 / 255.0, 0.0)   # translucent, the smallest illumination
        rec = w.records()[0]
        w.close()
        n, got = _host_list(V, rec, mn, mx)
        assert np.array_equal(got, oe.walk(rec, mn, mx)), f"bounds {mn} {mx}"
        assert got.tolist() == [[mn[0], mn[1], mn[2], 1], [mn[0] + 2, mn[1] + 1, mn[2] + 3, 1]], f"bounds {mn} {mx}: {got.tolist()}"
    # no emitter at all
    w = V.World()
    w.insert(1, 2, 3, 0xffffffff, 3.0, 0.0, 0.0)
    rec = w.records()[0]
    w.close()
    assert _host_list(V, rec)[0] == 0


# ---- the interface ----

def test_header_declares_and_library_exports_the_two_functions(V):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrt.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert re.search(r"\bint\s+vrt_set_emitter_sampling\s*\(\s*vrt_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)", text)
    assert re.search(r"\blong\s+vrt_emitters\s*\(\s*vrt_ctx\s*\*\s*\w*\s*,\s*int32_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\)", text)
    assert re.search(r"#define\s+VRT_MAX_EMITTERS\s+\(1u\s*<<\s*20\)", text) and V.MAX_EMITTERS == 1 << 20
    L = C.CDLL(V.HIP_LIB)
    for name in ("vrt_set_emitter_sampling", "vrt_emitters"):
        assert name in names and hasattr(L, name), f"libvrt_hip.so does not export {name}"


def test_hip_code_object_holds_the_emit_kernels(V):
    """the kernels that sample the emitter list are instantiations over EmitPaths<...> (csrc/vrt_common.hip.h)"""
    blob = open(V.HIP_LIB, "rb").read()
    assert b"gfx950" in blob
    names = set(re.findall(rb"_ZN3vrt[0-9A-Za-z_]*EmitPaths[0-9A-Za-z_]*", blob))
    for kernel in (b"full_accum_kernel", b"shade_rays_full_kernel"):
        assert any(kernel in n for n in names), f"no {kernel.decode()} over EmitPaths in libvrt_hip.so"
    for trav in (b"v4", b"v1"):
        assert any(trav in n for n in names), f"no kernel over EmitPaths<{trav.decode()}::...>"


def test_wrapper_refuses_values_other_than_0_and_1(V):
    class Fake(V.Context):
        def __init__(self):   # no device: the checks under test come before the library is called
            self._h = None
    c = Fake()
    assert c.emitter_sampling is False
    for bad in (2, -1, "1", None, 0.5, [1]):
        with pytest.raises(ValueError):
            c.set_emitter_sampling(bad)
    assert c.emitter_sampling is False
