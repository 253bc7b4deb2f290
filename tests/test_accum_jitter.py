"""Anti-aliased progressive accumulation (vrt_accum_begin_ex, VRT_ACCUM_JITTER): what holds without a GPU. The jitter sequence
is the header's (a literal table, exact multiples of 2^-24, one point per elementary interval), the checker
(tests/oracle_jitter.c) reproduces the oracle's frame at jittered sample 0 in every mode and moves silhouettes at other samples,
the library exports the call and the Python wrapper refuses bad modes and flags before any device is involved. The kernels are
held to the checker on the MI355X (test_gpu_accum_jitter.py)."""
import subprocess

import numpy as np
import pytest

import oracle_jitter

POSES = {   # the golden frames' poses (tests/golden/frames.json), at sizes the CPU renders in a moment
    "dragon": ("dragon", (63.5, 60.5, 140.5, -90.0, -10.0)),
    "nature": ("nature", (60.5, 80.5, 200.5, -90.0, -20.0)),
    "room_inside": ("room", (14.5, 30.5, 16.5, 32.0, -10.0)),
    "room_outside": ("room", (98.5, 34.5, 52.5, 197.0, -8.0)),
    "terrain": ("terrain", (512.5, 420.5, 1000.5, -90.0, -20.0)),
}

# include/vrt.h: the first eight (jx, jy)
TABLE = [(0.0, 0.0), (0.5, 0.5), (0.25, 0.75), (0.75, 0.25), (0.125, 0.625), (0.625, 0.125), (0.375, 0.375), (0.875, 0.875)]


@pytest.fixture(scope="module")
def J(tmp_path_factory):
    return oracle_jitter.build(tmp_path_factory.mktemp("oracle_jitter"))


def _scene(O, V, product_scenes, name, W, H):
    m, pose = POSES[name]
    tex, dim = product_scenes[m]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    return O.make_scene(tex, dim, ip, iv, cp)


def test_sequence_is_the_headers_table(J):
    for k, (x, y) in enumerate(TABLE):
        assert oracle_jitter.offsets(J, k) == (np.float32(x), np.float32(y)), f"sample {k}"


def test_sequence_values_are_exact_multiples_of_2_to_minus_24(J):
    for k in list(range(4096)) + [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1, 123456789]:
        for t in oracle_jitter.offsets(J, k):
            assert 0.0 <= t < 1.0
            q = float(t) * 2 ** 24
            assert q == int(q), f"sample {k}: {t} is not a multiple of 2^-24"


@pytest.mark.parametrize("block", [0, 3])
def test_first_2m_samples_stratify_every_elementary_interval(J, block):
    for m in range(9):
        n = 1 << m
        pts = [oracle_jitter.offsets(J, block * n + k) for k in range(n)]
        for a in range(m + 1):
            cells = {(int(float(x) * (1 << a)), int(float(y) * (1 << (m - a)))) for x, y in pts}
            assert len(cells) == n, f"m={m}, a={a}, block {block}: {n} points in {len(cells)} intervals of 2^-{a} x 2^-{m - a}"


@pytest.mark.parametrize("name", sorted(POSES))
def test_checker_jittered_sample0_is_the_oracle_frame(J, O, V, product_scenes, name):
    W, H = 90, 60
    s = _scene(O, V, product_scenes, name, W, H)
    for mode in (O.MODE_PRIMARY, O.MODE_PRIMARY_SHADOW, O.MODE_FULL):
        ref_rgba, ref_id, _, st = O.render(s, W, H, mode)
        assert st["hits"] > 300
        rgba, idd = oracle_jitter.render(J, s, W, H, mode, 0, jitter=True)
        assert np.array_equal(rgba, ref_rgba), f"{name} mode {mode}"
        assert np.array_equal(idd, ref_id), f"{name} mode {mode}"


def test_checker_without_jitter_is_the_frame_in_modes_0_and_1(J, O, V, product_scenes):
    W, H = 64, 40
    s = _scene(O, V, product_scenes, "dragon", W, H)
    for mode in (O.MODE_PRIMARY, O.MODE_PRIMARY_SHADOW):
        ref_rgba, ref_id, _, _ = O.render(s, W, H, mode)
        for k in (1, 7, 2 ** 32 - 1):
            rgba, idd = oracle_jitter.render(J, s, W, H, mode, k, jitter=False)
            assert np.array_equal(rgba, ref_rgba) and np.array_equal(idd, ref_id), f"mode {mode} sample {k}"


def _edge_world(V):
    """one opaque wall x in [0, 16), y in [0, 8), z = 0: a straight top edge and two side edges against the sky"""
    w = V.World()
    for x in range(16):
        for y in range(8):
            w.insert(x, y, 0, 0xC08040FF, 3.0, 0.0, 0.0)
    out = w.flatten()
    w.close()
    return out


def test_jittered_samples_move_the_silhouette_only(J, O, V):
    tex, dim = _edge_world(V)
    W, H = 61, 37
    ip, iv, cp, _ = V.camera_block((8.3, 6.2, 30.7), -87.3, -6.0, W, H)   # no axis-parallel ray
    s = O.make_scene(tex, dim, ip, iv, cp)
    for mode in (O.MODE_PRIMARY, O.MODE_PRIMARY_SHADOW):
        f0, id0 = oracle_jitter.render(J, s, W, H, mode, 0)
        hit = id0[..., 1] < 1024
        assert 0.1 < hit.mean() < 0.9
        # where sample 0 changes between a pixel's corner and the next corners to the right / below: the edges
        diff = np.zeros((H, W), bool)
        rgb = f0[..., :3].astype(int)
        near = np.zeros((H, W), bool)
        for dy, dx in ((0, 1), (1, 0), (1, 1)):
            d = np.any(rgb[dy:, dx:] != rgb[:H - dy, :W - dx], axis=-1)
            near[:H - dy, :W - dx] |= d
        near[-1, :] = True   # the last row and column have no corner below / to the right in the frame
        near[:, -1] = True
        for k in range(1, 8):
            fk, _ = oracle_jitter.render(J, s, W, H, mode, k)
            diff |= np.any(fk != f0, axis=-1)
        assert diff.sum() >= 20, f"mode {mode}: the jitter should move the wall's silhouette"
        assert not (diff & ~near).any(), f"mode {mode}: pixels away from any edge changed"


def test_library_exports_begin_ex(V):
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "vrt_accum_begin_ex" in names


def _unopened(V):
    # a Context whose vrt_create never ran: a wrapper that reached the library would fail on the missing handle
    return object.__new__(V.Context)


@pytest.mark.parametrize("kw", [{"mode": 3}, {"mode": -1}, {"mode": True}, {"mode": 1.0}, {"mode": "full"}, {"mode": None},
                                {"jitter": 2}, {"jitter": -1}, {"jitter": "yes"}, {"jitter": None}, {"jitter": 1.0},
                                {"mode": 0, "jitter": 3}])
def test_accum_begin_rejects_bad_mode_and_jitter_before_the_device(V, kw):
    with pytest.raises(ValueError):
        _unopened(V).accum_begin(64, 48, 0, **kw)


def test_accum_begin_keeps_its_checks_with_the_new_keywords(V):
    with pytest.raises(ValueError):
        _unopened(V).accum_begin(0, 48, 0, mode=V.MODE_PRIMARY, jitter=True)
    with pytest.raises(ValueError):
        _unopened(V).accum_begin(64, 48, 1 << 32, mode=V.MODE_FULL, jitter=True)
