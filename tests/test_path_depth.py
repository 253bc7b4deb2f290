"""Path depth (include/vrt.h vrt_set_path_depth): what holds without a GPU. The checker (tests/oracle_paths.c through oracle_path_depth: the oracle's
path_trace loop with the rule applied to its one branch) is the oracle at depth 1, its float colour is the sum of the
contributions it logs by the rule's formulas, its paths have the structure the rule gives them, the feature is not vacuous
and (voxel ID, dist) do not depend on the depth; the library declares and exports the call and holds the new kernels. The
kernels are held to the checker on the MI355X (test_gpu_path_depth.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_path_depth as opd
import oracle_rays
from conftest import ROOT

W, H = 72, 44
SCENES = {   # name -> (map, pose)
    "dragon": ("dragon", (63.5, 60.5, 140.5, -90.0, -10.0)),
    "monu9": ("monu9", (48.5, 60.5, 170.5, -90.0, -12.0)),
    "room_inside": ("room", (14.5, 30.5, 16.5, 32.0, -10.0)),
}
DEPTHS = (1, 2, 3, 8)


@pytest.fixture(scope="module")
def P(tmp_path_factory):
    return opd.build(tmp_path_factory.mktemp("oracle_path_depth"))


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return oracle_rays.build(tmp_path_factory.mktemp("oracle_rays"))


@pytest.fixture(scope="module")
def frames(R, O, V, product_scenes):
    """name -> (scene, origins, dirs): the frame rays of the 72 x 44 frame"""
    out = {}
    for name, (m, pose) in SCENES.items():
        tex, dim = product_scenes[m]
        ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
        s = O.make_scene(tex, dim, ip, iv, cp)
        out[name] = (s,) + oracle_rays.frame_rays(R, s, W, H)
    return out


@pytest.fixture(scope="module")
def room_logs(P, frames):
    """depth -> (rgba, id_dist, rgb, log) of the room seen from inside at sample 0: computed once, read by several tests"""
    s, o, d = frames["room_inside"]
    return {D: opd.shade(P, s, o, d, D, width=W, sample=0, log=True) for D in DEPTHS}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_depth_1_is_the_oracle_byte_for_byte(P, R, frames, name):
    s, o, d = frames[name]
    for k in (0, 1, 0xFFFFFFFF):
        ref_rgba, ref_id = oracle_rays.shade(R, s, o, d, 2, width=W, sample=k)
        rgba, idd, _ = opd.shade(P, s, o, d, 1, width=W, sample=k)
        assert np.array_equal(rgba, ref_rgba), f"{name} sample {k} rgba8"
        assert np.array_equal(idd, ref_id), f"{name} sample {k} id_dist"


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("D", DEPTHS)
def test_float_colour_is_the_sum_of_the_logged_contributions(P, frames, name, D):
    """A float64 sum of the logged contributions by the rule's formulas against the checker's float32 colour: each term is
    five or six float32 products and a quotient, and a ray adds a dozen of them, every operation rounded to 2^-24 relative --
    a dozen float32 roundings against float64, so the difference stays far below 1e-5 of the colour's largest channel."""
    s, o, d = frames[name]
    _, _, rgb, log = opd.shade(P, s, o, d, D, width=W, sample=3, log=True)
    want = opd.restate(log, o.shape[0], s.global_light)
    scale = np.maximum(np.abs(want).max(axis=1), np.finfo(np.float32).tiny)
    err = np.abs(rgb.astype(np.float64) - want).max(axis=1) / scale
    print(f"{name} D={D}: largest relative difference {err.max():.3g}, {len(log)} contributions")
    assert err.max() <= 1e-5


def _chains(log):
    """(ray, chain) -> list of that bounce chain's records of depth >= 1, in the order they were added"""
    out = {}
    for v in log[log["depth"] >= 1]:
        out.setdefault((int(v["ray"]), int(v["chain"])), []).append(v)
    return out


@pytest.mark.parametrize("D", DEPTHS)
def test_structure_of_the_paths_in_the_room(room_logs, D):
    log = room_logs[D][3]
    chains = _chains(log)
    assert len(chains) > 1000
    reached = 0
    for key, vs in chains.items():
        assert all(int(v["chain"]) > 0 for v in vs)
        opaque = [v for v in vs if v["kind"] in (opd.DIRECT, opd.AMBIENT, opd.EMIT)]
        assert len(opaque) <= D, f"{key}: {len(opaque)} opaque vertices below depth 0 at D = {D}"
        depths = [int(v["depth"]) for v in vs]
        assert depths == list(range(1, len(vs) + 1)), f"{key}: a bounce chain is linear"
        ambient = [v for v in vs if v["kind"] == opd.AMBIENT]
        inner = [v for v in vs if v["kind"] == opd.DIRECT]
        assert all(int(v["depth"]) < D for v in inner), f"{key}: an inner vertex at depth D"
        assert all(int(v["depth"]) == D for v in ambient), f"{key}: an ambient term above depth D"
        last = vs[-1]
        if int(last["depth"]) == D and last["kind"] not in (opd.SKY, opd.EMIT):   # reached depth D on a non-emissive surface
            reached += 1
            assert len(ambient) == 1 and last["kind"] == opd.AMBIENT, f"{key}: not exactly one ambient term"
        else:
            assert not ambient, f"{key}: an ambient term on a path that ended before depth D"
    assert reached > 100
    # no inner vertex carries an ambient term: a (ray, chain, depth) holds one record
    keys = np.stack([log["ray"].astype(np.int64), log["chain"].astype(np.int64), log["depth"].astype(np.int64)], axis=1)
    deep = keys[log["depth"] >= 1]
    assert len(np.unique(deep, axis=0)) == len(deep)
    # depth-0 records only ever are depth-0 kinds, and the terminal kind never appears at depth 0
    assert not np.any((log["depth"] == 0) & np.isin(log["kind"], (opd.SKY, opd.EMIT, opd.AMBIENT)))
    assert not np.any((log["depth"] >= 1) & np.isin(log["kind"], (opd.SKY0, opd.EMIT0, opd.GLASS)))


def test_depth_2_changes_the_room(room_logs):
    a, b = room_logs[1][0], room_logs[2][0]
    changed = int(np.any(a != b, axis=1).sum())
    print(f"room 72 x 44: {changed} of {a.shape[0]} pixels differ between D = 1 and D = 2")
    assert changed >= 1


@pytest.mark.parametrize("name", sorted(SCENES))
def test_id_dist_does_not_depend_on_the_depth(P, frames, name):
    s, o, d = frames[name]
    ref = opd.shade(P, s, o, d, 1, width=W, sample=5)[1]
    for D in DEPTHS[1:]:
        assert np.array_equal(opd.shade(P, s, o, d, D, width=W, sample=5)[1], ref), f"{name} D = {D}"


def test_mean_is_the_resolve_rule(P, frames):
    s, o, d = frames["dragon"]
    m, idd = opd.mean(P, s, o, d, 3, width=W, first_sample=2 ** 32 - 1, n_samples=2)   # wraps to sample 0
    x = opd.shade(P, s, o, d, 3, width=W, sample=2 ** 32 - 1)
    y = opd.shade(P, s, o, d, 3, width=W, sample=0)
    want = (x[0].astype(np.uint32) + y[0].astype(np.uint32) + 1) // 2
    want[:, 3] = 255
    assert np.array_equal(m, want.astype(np.uint8)) and np.array_equal(idd, x[1])


def test_header_declares_and_library_exports_set_path_depth(V):
    text = open(os.path.join(ROOT, "include", "vrt.h")).read()
    assert re.search(r"#define\s+VRT_MAX_PATH_DEPTH\s+8\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert re.search(r"\bint\s+vrt_set_path_depth\s*\(\s*vrt_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)", text), "include/vrt.h does not declare vrt_set_path_depth"
    assert "vrt_set_path_depth" in names and hasattr(C.CDLL(V.HIP_LIB), "vrt_set_path_depth")
    assert V.MAX_PATH_DEPTH == 8 and opd.MAX_DEPTH == 8


def test_hip_code_object_holds_the_deep_kernels(V):
    """the kernels that honour the depth are instantiations over DeepPaths<...> (csrc/vrt_common.hip.h)"""
    blob = open(V.HIP_LIB, "rb").read()
    assert b"gfx950" in blob
    names = set(re.findall(rb"_ZN3vrt[0-9A-Za-z_]*DeepPaths[0-9A-Za-z_]*", blob))
    for kernel in (b"full_accum_kernel", b"opaque_accum_kernel", b"bounce_accum_kernel", b"shade_rays_full_kernel"):
        assert any(kernel in n for n in names), f"no {kernel.decode()} over DeepPaths in libvrt_hip.so"


def test_wrapper_refuses_a_depth_that_is_no_integer(V):
    class Fake(V.Context):
        def __init__(self):   # no device: the checks under test come before the library is called
            self._h = None
    c = Fake()
    assert c.path_depth == 1
    for bad in (True, 2.0, "3", None):
        with pytest.raises(ValueError):
            c.set_path_depth(bad)
    assert c.path_depth == 1
