"""Emitter MIS (include/vrt.h vrt_set_emitter_mis): what holds without a GPU. The checker (tests/oracle_paths.c through oracle_emit_mis) is
oracle_emit_power at flag 0, bit for bit; at flag 1 its log shows the density and the two weights of the balance heuristic, which a
numpy float32 restatement reproduces bit for bit and which sum to one; the estimator has the expectation of the power rule and of
sampling off, both planted misreadings of the bounce side fail that test, every connection weight g * wn is bounded where the power
rule's g runs past 10, and next to emitters the variance falls. The kernels are held to the checker on the MI355X
(test_gpu_emit_mis.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import emit_mis_worlds as mw
import oracle_emit_mis as om
import oracle_emit_power as op
import oracle_rays
from conftest import ROOT

F = np.float32
W, H = mw.W, mw.H
SAMPLE = 5


@pytest.fixture(scope="module")
def M(tmp_path_factory):
    return om.build(tmp_path_factory.mktemp("oracle_emit_mis"))


@pytest.fixture(scope="module")
def P(tmp_path_factory):
    return op.build(tmp_path_factory.mktemp("oracle_emit_power"))


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_rays"))


def _world(O, V, pane):
    """-> (scene, list, words, weights uint64)"""
    w = mw.room(V, pane=pane)
    tex, dim = w.flatten()
    ip, iv, cp, _ = V.camera_block(mw.POSE[:3], mw.POSE[3], mw.POSE[4], W, H)
    s = O.make_scene(tex, dim, ip, iv, cp)
    lst, words = op.walk(w.records()[0])
    w.close()
    return s, lst, words, np.array(op.weights(lst, words), np.uint64)


@pytest.fixture(scope="module")
def room(O, V, R):
    """the fixture with its pane -> (scene, frame origins, frame dirs, list, words, weights)"""
    s, lst, words, wt = _world(O, V, True)
    return (s,) + oracle_rays.frame_rays(R, s, W, H) + (lst, words, wt)


# ---- the fixture ----

def test_the_fixture_holds_the_lamp_as_one_entry_three_singles_and_a_black_emitter(room):
    lst, words, wt = room[3:]
    assert lst.tolist() == mw.expected_list() and len(lst) == mw.N_EMITTERS
    lamp = lst.tolist().index(list(mw.LAMP[0]) + [2])
    assert int(lst[:, 3].sum()) == 2 + 4, "the lamp is one entry of size 2, not its unit cells"
    singles = [lst.tolist().index(list(p) + [1]) for p, _, _ in mw.SINGLES]
    assert [(int(words[j, 1]) >> 8) & 0xff for j in singles] == [i for _, _, i in mw.SINGLES] and len({i for _, _, i in mw.SINGLES}) == 3
    black = lst.tolist().index(list(mw.BLACK[0]) + [1])
    assert int(wt[black]) == 0 and (int(words[black, 1]) >> 8) & 0xff == mw.BLACK[2] > 0, "the black emitter: colour 0, illumination > 0"
    assert 2 * int(wt[lamp]) > int(wt.sum())


def test_host_inv_power_is_the_restatement(V, room):
    T = V.test_lib()
    T.vrt_test_emitter_inv_power.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    T.vrt_test_emitter_inv_power.restype = C.c_long
    lst, words, wt = room[3:]
    cases = [(lst, words, [int(x) for x in wt]), (lst[-1:], words[-1:], [0])]
    big = np.zeros((4096, 4), np.int32)
    big[:, 3] = 1024
    bw = np.tile(np.array([[0xffffffff, 0x0000ffff]], np.uint32), (4096, 1))
    cases.append((big, bw, op.weights(big, bw)))
    for l, wd, wts in cases:
        l, wd = np.ascontiguousarray(l, np.int32), np.ascontiguousarray(wd, np.uint32)
        tot, inv = np.zeros(1, np.uint64), np.zeros(1, F)
        assert T.vrt_test_emitter_inv_power(l.ctypes.data, wd.ctypes.data, len(l), tot.ctypes.data, inv.ctypes.data) == len(l)
        assert int(tot[0]) == sum(wts)
        assert inv.view(np.uint32)[0] == om.inv_power(wts).view(np.uint32), f"inv_power of Wtot = {sum(wts)}"
    assert om.inv_power([0]) == 0.0


# ---- flag 0 ----

@pytest.mark.parametrize("D", (1, 3))
@pytest.mark.parametrize("radius", (0.0, 0.05))
def test_flag_0_is_oracle_emit_power_bit_for_bit(M, P, room, D, radius):
    s, o, d, lst, _, wt = room
    for mode in (op.UNIFORM, op.POWER):
        for k in (0, 5):
            want = op.shade(P, s, o, d, D, radius, lst, wt, mode, width=W, sample=k)
            flags = (0, 1) if mode == op.UNIFORM else (0,)   # the flag is not read at VRT_EMIT_UNIFORM
            for mis in flags:
                got = om.shade(M, s, o, d, D, radius, lst, wt, mode, mis, width=W, sample=k)
                what = f"mode {mode} flag {mis} D={D} radius {radius} sample {k}"
                assert np.array_equal(got[0], want[0]), f"{what} rgba8"
                assert np.array_equal(got[1], want[1]), f"{what} id_dist"
                assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), f"{what} float bits"
        ref = op.shade(P, s, o, d, D, radius, lst, wt, mode, width=W, sample=SAMPLE, log=True)[3]
        got = om.shade(M, s, o, d, D, radius, lst, wt, mode, 0, width=W, sample=SAMPLE, log=True)[3]
        assert len(ref) == len(got)
        for name in ref.dtype.names:
            assert np.array_equal(ref[name].view(np.uint32), got[name].view(np.uint32)), f"mode {mode}: log field {name}"
        assert not np.any(got["has_mis"]) and not np.any(got["pl"]) and not np.any(got["wt"])
    # an empty list: the flag is not read
    a = om.shade(M, s, o, d, D, radius, None, None, op.POWER, 1, width=W, sample=0)
    b = op.shade(P, s, o, d, D, radius, None, None, op.POWER, width=W, sample=0)
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


# ---- the log against the contract ----

def _restate(rec, inv):
    """the density and both weights of the logged inputs, in numpy float32 -> (pl, pb, m, w, wn, wb)"""
    rgb = rec["mrgb"].astype(np.int64)
    w = rec["millum"].astype(np.int64) * ((rgb & 0xff) + ((rgb >> 8) & 0xff) + ((rgb >> 16) & 0xff))
    pl, pb, m = om.density(rec["mx"], rec["mdir"], rec["mcs"], rec["mpoint"], rec["maxis"], rec["mcell"], w, inv)
    wn, wb = om.weights_of(pl, pb)
    return pl, pb, m, w, wn, wb


def _check_log(log, lst, words, inv, what):
    """every record with MIS fields against the restatement, bit for bit; -> (connections that contributed, emissive bounce hits)"""
    rec = log[log["has_mis"] == 1]
    assert set(np.unique(rec["kind"]).tolist()) <= {om.DIRECT, om.EMIT}
    pl, pb, m, w, wn, wb = _restate(rec, inv)
    assert np.array_equal(m, rec["mm"]) and np.array_equal(w, rec["mw"]), f"{what}: m or w"
    assert np.array_equal(pl.view(np.uint32), rec["pl"].view(np.uint32)), f"{what}: pl"
    assert np.array_equal(pb.view(np.uint32), rec["pb"].view(np.uint32)), f"{what}: pb"
    conn = rec["kind"] == om.DIRECT
    assert np.array_equal(wn[conn].view(np.uint32), rec["wt"][conn].view(np.uint32)), f"{what}: wn"
    assert np.array_equal(wb[~conn].view(np.uint32), rec["wt"][~conn].view(np.uint32)), f"{what}: wb"
    # the words are those of the list entry that holds the hit cell, as W_j reads them
    for r in rec[:: max(1, len(rec) // 200)]:
        j = [i for i, e in enumerate(lst.tolist()) if all(e[k] <= int(r["mcell"][k]) < e[k] + e[3] for k in range(3))]
        assert len(j) == 1, f"{what}: the hit cell {r['mcell']} lies in no list cube"
        w0, w1 = (int(x) for x in words[j[0]])
        assert int(r["mrgb"]) == w0 & 0xffffff and int(r["millum"]) == (w1 >> 8) & 0xff
    # connections: the log's x is the vertex, the hit lies in the picked cube, and wn + wb = 1 where something was added
    c = rec[conn]
    assert np.array_equal(c["mx"].view(np.uint32), c["x"].view(np.uint32)) and np.all(c["in_box"] == 1) and np.all(c["g"] > 0)
    added = c["pl"] > 0
    s = wn[conn][added].astype(np.float64) + wb[conn][added].astype(np.float64)
    assert np.all(np.abs(s - 1.0) <= 2.0 ** -22), f"{what}: wn + wb off one by {np.abs(s - 1.0).max()}"
    # records without the fields carry zeros
    other = log[log["has_mis"] == 0]
    assert not np.any(other["pl"]) and not np.any(other["pb"]) and not np.any(other["wt"]) and not np.any(other["mw"])
    return int(conn.sum()), int((~conn).sum())


@pytest.mark.parametrize("D", (1, 3))
@pytest.mark.parametrize("radius", (0.0, 0.05))
def test_log_shows_the_rule(M, room, D, radius):
    s, o, d, lst, words, wt = room
    inv = om.inv_power(wt)
    n_conn = n_bounce = 0
    for k in range(SAMPLE, SAMPLE + 4):
        rgba, idd, rgb, log = om.shade(M, s, o, d, D, radius, lst, wt, op.POWER, 1, width=W, sample=k, log=True)
        a, b = _check_log(log, lst, words, inv, f"D={D} radius {radius} sample {k}")
        n_conn += a
        n_bounce += b
        # the same draws as at flag 0: the DIRECT records agree in every field the power rule logs up to g
        ref = om.shade(M, s, o, d, D, radius, lst, wt, op.POWER, 0, width=W, sample=k, log=True)[3]
        dm, dr = log[log["kind"] == om.DIRECT], ref[ref["kind"] == om.DIRECT]
        assert len(dm) == len(dr)
        for name in ("ray", "depth", "u0", "uf", "ua", "ub", "rx", "ry", "j", "f", "q", "cs", "cl", "r2", "g", "E", "t", "ticks", "m", "x"):
            assert np.array_equal(dm[name].view(np.uint32), dr[name].view(np.uint32)), f"flag 1 against flag 0: {name}"
        assert np.array_equal(idd, ref_id(M, s, o, d, D, radius, k))
    print(f"D={D} radius {radius}: {n_conn} connections and {n_bounce} emissive bounce hits checked")
    assert n_conn > 200 and n_bounce > 20


def ref_id(M, s, o, d, D, radius, k):
    return om.shade(M, s, o, d, D, radius, None, None, op.UNIFORM, 0, width=W, sample=k)[1]


# ---- the same expectation, bounded weights, less variance next to emitters ----

K = 16384
Z = 4.5   # tests/test_emitters.py's bound


def _within(a, b):
    """per ray and channel |mean_a - mean_b| <= Z sqrt((var_a + var_b) / K) -> (all within, largest |z|)"""
    (m_a, v_a), (m_b, v_b) = a[:2], b[:2]
    se = np.sqrt((v_a + v_b) / K)
    z = np.abs(m_a - m_b) / np.maximum(se, 1e-300)
    return bool(np.all(np.abs(m_a - m_b) <= Z * se)), float(z.max())


def test_mis_has_the_expectation_of_power_and_of_off_with_bounded_weights(M, O, V):
    """The fixture without its pane; the near rays (EYE to surface points 0.15 .. 1.5 voxels from the lamp's foot and beside singles)
    and the far rays (emit_worlds.probe_rays()) together, K = 16384 samples, D in {1, 2}. Per ray and channel the means of MIS and
    power, and of MIS and sampling off, differ by at most 4.5 standard errors of the difference (the run's own sample variances);
    both planted misreadings of the bounce side (weight 1: light counted twice; nothing added) fail the same test. Over the run every
    logged g * wn is at most 1.01 / (1 - N * 2^-24) while the power rule's largest g on the same rays and samples is above 10. On
    the near rays the summed sample variance with MIS is below power's; the ratios are printed."""
    s, lst, words, wt = _world(O, V, False)
    assert len(lst) == mw.N_EMITTERS
    inv = om.inv_power(wt)
    o, d, n_near = mw.all_rays()
    near, far = slice(0, n_near), slice(n_near, None)

    def run(D, emitters, mis, debug=0, log=False):
        out, g_max, gw_max = [], 0.0, 0.0
        for k in range(K):
            r = om.shade(M, s, o, d, D, 0.0, emitters, wt if emitters is not None else None, op.POWER, mis, sample=k, debug=debug, log=log)
            out.append(r[2])
            if log:
                c = r[3][r[3]["kind"] == om.DIRECT]
                if len(c):
                    g_max = max(g_max, float(c["g"].max()))
                    gw_max = max(gw_max, float((c["g"] * c["wt"]).max()))   # float32, as the kernel's (E * g) * wn scales E
                if mis and k % 512 == 0:
                    _check_log(r[3], lst, words, inv, f"D={D} sample {k}")
        rgb = np.stack(out).astype(np.float64)
        return rgb.mean(axis=0), rgb.var(axis=0, ddof=1), g_max, gw_max

    bound = 1.01 / (1.0 - len(lst) * 2.0 ** -24)
    for D in (1, 2):
        off = run(D, None, 0)
        pwr = run(D, lst, 0, log=True)
        mis = run(D, lst, 1, log=True)
        ok_p, z_p = _within(mis, pwr)
        ok_o, z_o = _within(mis, off)
        print(f"D={D}: max |z| MIS against power {z_p:.2f}, against off {z_o:.2f}; largest g with power {pwr[2]:.4g}, largest g * wn with MIS {mis[3]:.4g} "
              f"(bound {bound:.6f})")
        for name, sl in (("near", near), ("far", far)):
            v_o, v_p, v_m = off[1][sl].sum(), pwr[1][sl].sum(), mis[1][sl].sum()
            print(f"D={D} {name}: summed variance off {v_o:.4g}, power {v_p:.4g}, MIS {v_m:.4g}: power / MIS {v_p / v_m:.2f}, off / MIS {v_o / v_m:.2f}")
        assert ok_p, f"D={D}: MIS against power, max |z| {z_p:.2f}"
        assert ok_o, f"D={D}: MIS against sampling off, max |z| {z_o:.2f}"
        assert pwr[2] > 10.0, f"D={D}: the fixture's largest g in power mode is {pwr[2]}: the near rays are not near enough"
        assert mis[3] <= bound, f"D={D}: a connection weight g * wn of {mis[3]} exceeds {bound}"
        assert mis[1][near].sum() < pwr[1][near].sum(), f"D={D}: near-set variance MIS {mis[1][near].sum()} power {pwr[1][near].sum()}"
        if D == 1:   # the test can tell: a misread bounce side is caught by the same bound
            for debug, what in ((1, "the bounce keeps weight 1"), (2, "the bounce adds nothing")):
                x = run(D, lst, 1, debug)
                ok_a, z_a = _within(x, pwr)
                ok_b, z_b = _within(x, off)
                print(f"D={D} planted misreading ({what}): max |z| against power {z_a:.2f}, against off {z_b:.2f}")
                assert not ok_a and not ok_b, f"the expectation test does not catch the misreading '{what}' (max |z| {z_a:.2f}, {z_b:.2f})"


# ---- the interface ----

def test_header_declares_and_library_exports_the_function(V):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrt.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert re.search(r"\bint\s+vrt_set_emitter_mis\s*\(\s*vrt_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)", text)
    assert "vrt_set_emitter_mis" in names and hasattr(C.CDLL(V.HIP_LIB), "vrt_set_emitter_mis"), "libvrt_hip.so does not export vrt_set_emitter_mis"


def test_hip_code_object_holds_the_mis_kernels(V):
    """the kernels of vrt_set_emitter_mis are instantiations over EmitMisPaths<...> (csrc/vrt_common.hip.h), for both traversals"""
    blob = open(V.HIP_LIB, "rb").read()
    assert b"gfx950" in blob
    names = set(re.findall(rb"_ZN3vrt[0-9A-Za-z_]*EmitMisPaths[0-9A-Za-z_]*", blob))
    for kernel in (b"full_accum_kernel", b"shade_rays_full_kernel"):
        for trav in (b"v4", b"v1"):
            assert any(kernel in n and b"EmitMisPathsINS_2" + trav in n for n in names), f"no {kernel.decode()} over EmitMisPaths<{trav.decode()}::...>"


def test_wrapper_refuses_other_values_without_touching_the_library(V):
    class Fake(V.Context):
        def __init__(self):   # no device: the checks under test come before the library is called
            self._h = None
    c = Fake()
    assert c.emitter_mis == 0
    for bad in (2, -1, "1", None, 0.5, [1]):
        with pytest.raises(ValueError):
            c.set_emitter_mis(bad)
    assert c.emitter_mis == 0
