"""Sun disc (include/vrt.h vrt_set_sun_disc): what holds without a GPU. The checker (tests/oracle_paths.c through oracle_sun: the depth
loop with the rule applied at the shadowing vertices) is oracle_path_depth at radius 0; its log shows the rule's draws, map, direction
and n.l; its float colour is the sum of the contributions it logs; and the penumbra of a straight edge has the area of the
visible part of the disc. The kernels are held to the checker on the MI355X (test_gpu_sun_disc.py)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_path_depth as opd
import oracle_rays
import oracle_sun as osun
import sun_worlds as sw
from conftest import ROOT

F = np.float32
W, H = sw.W, sw.H


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    return osun.build(tmp_path_factory.mktemp("oracle_sun"))


@pytest.fixture(scope="module")
def P(tmp_path_factory):
    return opd.build(tmp_path_factory.mktemp("oracle_path_depth"))


@pytest.fixture(scope="module")
def frames(tmp_path_factory, O, V, product_scenes):
    """world -> (scene, origins, dirs): the rays of the 72 x 44 frame"""
    R = oracle_rays.build(tmp_path_factory.mktemp("oracle_rays"))
    return {name: (s,) + oracle_rays.frame_rays(R, s, W, H) for name, (_, _, _, s) in sw.scenes(O, V, product_scenes).items()}


@pytest.fixture(scope="module")
def logs(S, frames):
    """(world, D, radius) -> (rgba, id_dist, rgb, log) at sample 5: computed once, read by several tests"""
    cache = {}

    def get(world, D, radius):
        if (world, D, radius) not in cache:
            s, o, d = frames[world]
            cache[(world, D, radius)] = osun.shade(S, s, o, d, D, radius, width=W, sample=5, log=True)
        return cache[(world, D, radius)]
    return get


@pytest.mark.parametrize("world", sw.WORLDS)
@pytest.mark.parametrize("D", (1, 2, 3, 8))
def test_radius_0_is_oracle_path_depth_bit_for_bit(S, P, frames, world, D):
    s, o, d = frames[world]
    for k in (0, 5):
        ref = opd.shade(P, s, o, d, D, width=W, sample=k)
        got = osun.shade(S, s, o, d, D, 0.0, width=W, sample=k)
        assert np.array_equal(got[0], ref[0]), f"{world} D={D} sample {k} rgba8"
        assert np.array_equal(got[1], ref[1]), f"{world} D={D} sample {k} id_dist"
        assert np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32)), f"{world} D={D} sample {k} float bits"


# ---- the log against the contract ----

def _stream(px, py, sample, n):
    """the first n draws of initRNG(px, py, sample) (comp:380-399) in Python integers -> float32"""
    M = 0xFFFFFFFF
    seed = (px + py * 1920 + 123456 + sample * 78901) & M
    st = (seed * 747796405 + 2891336453) & M
    w = (((st >> ((st >> 28) + 4)) ^ st) * 277803737) & M
    state = (w >> 22) ^ w
    out = []
    for _ in range(n):
        state = (state * 747796405 + 2891336453) & M
        w = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & M
        state = (w >> 22) ^ w
        out.append(F(state) / F(4294967296.0))   # (float)state: the integer rounded to nearest even, then an exact division
    return out


def _disc_map(S, u1, u2):
    """the concentric map in float32, one operation per step; sin / cos from the library's probes"""
    a = F(F(2.0) * u1) - F(1.0)
    b = F(F(2.0) * u2) - F(1.0)
    if a == 0.0 and b == 0.0:
        return F(0.0), F(0.0)
    if abs(a) > abs(b):
        r, phi = a, F(F(0.785398163) * F(b / a))
    else:
        r, phi = b, F(F(1.57079633) - F(F(0.785398163) * F(a / b)))
    return F(r * F(S.o_det_cosf(float(phi)))), F(r * F(S.o_det_sinf(float(phi))))


@pytest.mark.parametrize("world", sw.WORLDS)
@pytest.mark.parametrize("D", (1, 3))
@pytest.mark.parametrize("radius", (0.05, 1.0))
def test_log_shows_the_rule(S, frames, logs, world, D, radius):
    s = frames[world][0]
    log = logs(world, D, radius)[3]
    direct = log[log["kind"] == osun.DIRECT]
    assert len(direct) > (100 if world != "unit" else 0)
    _, ll, Ln, T, B = osun.basis(S, s.light_dir, radius)
    Ln64, ll64 = Ln.astype(np.float64), float(ll)
    # four draws per shadowing vertex, consecutive in the pixel's stream, in the order the vertices were shaded
    used = {}
    for v in direct:
        ray = int(v["ray"])
        at = used.get(ray, 0)
        draws = _stream(ray % W, ray // W, 5, at + 4)[at:]
        assert (v["u1"], v["u2"], v["rx"], v["ry"]) == tuple(draws), f"ray {ray} vertex at draw {at}"
        used[ray] = at + 4
        dx, dy = _disc_map(S, v["u1"], v["u2"])
        assert (dx.view(np.uint32), dy.view(np.uint32)) == (v["dx"].view(np.uint32), v["dy"].view(np.uint32)), f"ray {ray}: the disc map"
    lp = direct["lp"].astype(np.float64)
    cross = np.linalg.norm(np.cross(lp, Ln64), axis=1)
    along = lp @ Ln64
    assert np.all(cross <= radius * along * (1.0 + 1e-5)), "L' outside the cone of the disc"
    assert np.all(np.abs(np.linalg.norm(lp, axis=1) / ll64 - 1.0) <= 4.0 * 2.0 ** -23), "|L'| is not lightDir's length"
    n, l32 = direct["normal"], direct["lp"]
    dot = F(F(n[:, 0] * l32[:, 0]) + F(n[:, 1] * l32[:, 1])) + F(n[:, 2] * l32[:, 2])
    assert np.array_equal(direct["ndotl"], np.maximum(dot.astype(F), F(0.0))), "the logged ndotl is not max(dot(normal, L'), 0)"
    if radius == 1.0 and world != "unit":
        below = (direct["ndotl"] == 0.0) & (direct["normal"].astype(np.float64) @ Ln64 > 0.0)
        print(f"{world} D={D}: {int(below.sum())} of {len(direct)} vertices take a direction below their horizon")
        assert below.any()
    # the other kinds draw nothing and log no direction
    other = log[log["kind"] != osun.DIRECT]
    assert not np.any(other["u1"]) and not np.any(other["lp"])


@pytest.mark.parametrize("world", sw.WORLDS)
@pytest.mark.parametrize("D", (1, 3))
def test_float_colour_is_the_sum_of_the_logged_contributions(frames, logs, world, D):
    """tests/test_path_depth.py's bound for its own restatement: a dozen float32 roundings against float64, far below 1e-5 of the
    colour's largest channel"""
    s, o, _ = frames[world]
    _, _, rgb, log = logs(world, D, 0.05)
    want = osun.restate(log, o.shape[0] if o.ndim == 2 else W * H, s.global_light)
    scale = np.maximum(np.abs(want).max(axis=1), np.finfo(np.float32).tiny)
    err = np.abs(rgb.astype(np.float64) - want).max(axis=1) / scale
    print(f"{world} D={D}: largest relative difference {err.max():.3g}, {len(log)} contributions")
    assert err.max() <= 1e-5


def test_the_sun_disc_changes_the_dragon_and_keeps_id_dist(logs):
    a, b = logs("dragon", 1, 0.05), logs("dragon", 1, 1.0)
    assert np.any(a[0] != b[0])
    assert np.array_equal(a[1], b[1])


# ---- the penumbra of a straight edge ----

def _visible(t):
    t = min(max(t, -1.0), 1.0)
    return 0.5 + (t * math.sqrt(1.0 - t * t) + math.asin(t)) / math.pi


def test_penumbra_is_the_visible_area_of_the_disc(S, O, V):
    """17 floor points across the shadow edge of a slab 8 voxels up, light straight down the y axis, tan_radius 0.25, D = 1:
    the fraction of N = 4096 samples whose depth-0 shadow ray is unoccluded against F(t) = 1/2 + (t sqrt(1 - t^2) + asin t) / pi,
    t = (x - x0) / (tan_radius (h' - 2e-3)), within the binomial 4.5 sigma. h' is the height of the edge that decides: under the
    slab (x < x0) a ray is lit iff it has passed x0 when it reaches the bottom face, h' = h = 8; outside it (x > x0) a ray is
    blocked iff it is inside x0 anywhere between the slab's bottom and top face, and it moves one way, so the top edge decides:
    h' = h + 1, the slab being one voxel thick. (With h' = h on both sides the closed form describes a slab of no thickness, which
    no voxel world holds: the checker then lies 0.02-0.03 below it at every x > x0, on the side face's account.)"""
    N, radius = 4096, 0.25
    w = sw.slab_world(V)
    tex, dim = w.flatten()
    w.close()
    ip, iv, cp, _ = V.camera_block((0.5, 0.5, 0.5), 0.0, 0.0, 8, 8)
    s = O.make_scene(tex, dim, ip, iv, cp)
    s.light_dir[:] = sw.SLAB_LIGHT
    _, _, _, T, B = osun.basis(S, s.light_dir, radius)
    assert tuple(T) == (-1.0, 0.0, 0.0) and tuple(B) == (0.0, 0.0, 1.0)
    offsets = np.linspace(-2.5, 2.5, 17)
    o, d = sw.slab_rays(offsets)
    lit = np.zeros(len(offsets), np.int64)
    for k in range(N):
        log = osun.shade(S, s, o, d, 1, radius, sample=k, log=True)[3]
        v = log[(log["kind"] == osun.DIRECT) & (log["depth"] == 0)]
        assert np.array_equal(v["ray"], np.arange(len(offsets))), "every ray has one depth-0 shadowing vertex, on the floor"
        assert not np.any((v["lit"] == 1) & (v["shadow_steps"] >= 64)), "an unoccluded shadow ray ended by the 64-step cap"
        lit += v["lit"]
    for dx, m in zip(offsets, lit):
        Fv = _visible(dx / (radius * (sw.SLAB_H + (1.0 if dx > 0.0 else 0.0) - 2e-3)))
        tol = min(4.5 * math.sqrt(max(Fv * (1.0 - Fv), 1.0 / N) / N), 0.036)
        print(f"x - x0 = {dx:+.4f}: lit {m / N:.4f}, visible area {Fv:.4f}, tolerance {tol:.4f}")
        assert abs(m / N - Fv) <= tol, f"x - x0 = {dx}: {m / N} against {Fv}"
    # Radius 0: nothing is drawn and nothing softens, so every sample gives a point the same lit. (lightDir = (0, 1, 0) has two zero
    # components, the shader's degenerate shadow ray, so that lit is not the geometric edge's; only its constancy is asserted.)
    hard = [osun.shade(S, s, o, d, 1, 0.0, sample=k, log=True)[3] for k in (0, 1, 2, 77, 4095)]
    hard = [h[(h["kind"] == osun.DIRECT) & (h["depth"] == 0)] for h in hard]
    print(f"radius 0: lit {hard[0]['lit'].tolist()}")
    for h in hard:
        assert np.array_equal(h["ray"], np.arange(len(offsets))) and set(h["lit"].tolist()) <= {0, 1}, "radius 0: lit in {0, 1}"
        assert np.array_equal(h["lit"], hard[0]["lit"]), "radius 0: lit changes with the sample"
        assert not np.any(h["u1"]) and not np.any(h["u2"]) and not np.any(h["dx"]) and not np.any(h["dy"]), "radius 0 drew a number"
        assert np.array_equal(h["lp"], np.tile(np.array(sw.SLAB_LIGHT, F), (len(offsets), 1))), "radius 0: L' is not lightDir"
    # ... and the bounce's two draws are then the stream's first two
    for r, v in enumerate(hard[0]):
        assert (v["rx"], v["ry"]) == tuple(_stream(r, 0, 0, 2)), f"radius 0, ray {r}: the bounce does not take the first two draws"


# ---- the host's basis ----

def test_host_basis_is_the_checkers(S, V):
    """sun_block() (csrc/vrt_sun.h), what the dispatcher hands the kernels, against the checker's basis bit for bit: the default
    light, axis directions, both sides of the |Ln.z| < 0.999 switch of `up`, un-normalised and tiny lights"""
    T = V.test_lib()
    T.vrt_test_sun_block.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
    T.vrt_test_sun_block.restype = None
    rng = np.random.default_rng(7)
    lights = [(0.3481553, 0.870388, 0.3481553), (0, 1, 0), (1, 0, 0), (0, 0, 1), (0, 0, -1), (0, -1, 0), (-1, 0, 0),
              (0.04, 0.02, 0.999), (0.05, 0.0, 0.9987), (0.03, 0.03, -0.9991), (0.0447, 0.0, 0.999), (3.0, -40.0, 2.5), (1e-4, 2e-4, -3e-4)]
    lights += [tuple(v) for v in rng.normal(0, 1, (40, 3))]
    switched = 0
    for light in lights:
        ld = np.array(light, F)
        for radius in (0.00465, 0.25, 1.0):
            got = np.zeros(11, F)
            T.vrt_test_sun_block(ld.ctypes.data, radius, got.ctypes.data)
            r, ll, Ln, Tn, Bn = osun.basis(S, ld, radius)
            want = np.concatenate([[r, ll], Ln, Tn, Bn]).astype(F)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"light {light} radius {radius}: {got} against {want}"
        switched += int(abs(float(Ln[2])) >= 0.999)
    assert 3 <= switched < len(lights), "both sides of the `up` switch are exercised"


# ---- the interface ----

def test_header_declares_and_library_exports_set_sun_disc(V):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrt.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert re.search(r"\bint\s+vrt_set_sun_disc\s*\(\s*vrt_ctx\s*\*\s*\w*\s*,\s*float\s+\w+\s*\)", text), "include/vrt.h does not declare vrt_set_sun_disc"
    assert "vrt_set_sun_disc" in names and hasattr(C.CDLL(V.HIP_LIB), "vrt_set_sun_disc")


def test_hip_code_object_holds_the_sun_kernels(V):
    """the kernels that honour the sun disc are instantiations over SunPaths<...> (csrc/vrt_common.hip.h)"""
    blob = open(V.HIP_LIB, "rb").read()
    assert b"gfx950" in blob
    names = set(re.findall(rb"_ZN3vrt[0-9A-Za-z_]*SunPaths[0-9A-Za-z_]*", blob))
    for kernel in (b"full_accum_kernel", b"opaque_accum_kernel", b"bounce_accum_kernel", b"shade_rays_full_kernel"):
        assert any(kernel in n for n in names), f"no {kernel.decode()} over SunPaths in libvrt_hip.so"


def test_wrapper_refuses_a_radius_that_is_no_number(V):
    class Fake(V.Context):
        def __init__(self):   # no device: the checks under test come before the library is called
            self._h = None
    c = Fake()
    assert c.sun_disc == 0.0
    for bad in (True, "0.1", None, [0.1]):
        with pytest.raises(ValueError):
            c.set_sun_disc(bad)
    assert c.sun_disc == 0.0
