"""Progressive accumulation of VRT_MODE_FULL (vrt_accum_*): what holds without a GPU. The checker (tests/oracle_samples.c, the
oracle's frame at any initRNG sample index) reproduces the oracle's own frame at sample 0, its id_dist does not depend on the
sample while its colours do, the library exports the calls and the Python wrappers refuse bad arguments before any device is
involved. The kernels are held to the checker on the MI355X (test_gpu_accumulate.py)."""
import subprocess

import numpy as np
import pytest

import oracle_samples

POSES = {   # the golden frames' poses (tests/golden/frames.json), at sizes the CPU renders in a moment
    "dragon": ("dragon", (63.5, 60.5, 140.5, -90.0, -10.0)),
    "nature": ("nature", (60.5, 80.5, 200.5, -90.0, -20.0)),
    "room_inside": ("room", (14.5, 30.5, 16.5, 32.0, -10.0)),
    "room_outside": ("room", (98.5, 34.5, 52.5, 197.0, -8.0)),
    "terrain": ("terrain", (512.5, 420.5, 1000.5, -90.0, -20.0)),
}


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    return oracle_samples.build(tmp_path_factory.mktemp("oracle_samples"))


def _scene(O, V, product_scenes, name, W, H):
    m, pose = POSES[name]
    tex, dim = product_scenes[m]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    return O.make_scene(tex, dim, ip, iv, cp)


@pytest.mark.parametrize("name", sorted(POSES))
def test_checker_sample0_is_the_oracle_frame(S, O, V, product_scenes, name):
    W, H = 96, 64
    s = _scene(O, V, product_scenes, name, W, H)
    ref_rgba, ref_id, _, st = O.render(s, W, H, O.MODE_FULL)
    rgba, idd = oracle_samples.render_sample(S, s, W, H, O.MODE_FULL, 0)
    assert st["hits"] > 500
    assert np.array_equal(rgba, ref_rgba)
    assert np.array_equal(idd, ref_id)


@pytest.mark.parametrize("name", ["dragon", "room_outside"])
def test_id_dist_is_the_same_for_every_sample_and_colours_are_not(S, O, V, product_scenes, name):
    W, H = 64, 40
    s = _scene(O, V, product_scenes, name, W, H)
    rgba0, id0 = oracle_samples.render_sample(S, s, W, H, O.MODE_FULL, 0)
    hit = id0[..., 0] != 0
    assert hit.sum() > 200
    changed = np.zeros((H, W), bool)
    for k in list(range(1, 16)) + [2 ** 31 - 1, 2 ** 32 - 1]:
        rgba, idd = oracle_samples.render_sample(S, s, W, H, O.MODE_FULL, k)
        assert np.array_equal(idd, id0), f"sample {k}: id_dist differs from sample 0"
        assert np.array_equal(rgba[..., 3], rgba0[..., 3])
        changed |= np.any(rgba != rgba0, axis=-1)
    assert changed[hit].mean() > 0.2, "the samples should differ where the diffuse bounce reads the RNG"
    assert not changed[~hit].any() if name == "dragon" else True   # sky: no random number is drawn


def test_checker_row_range_matches_the_whole_frame(S, O, V, product_scenes):
    W, H = 80, 48
    s = _scene(O, V, product_scenes, "dragon", W, H)
    full, full_id = oracle_samples.render_sample(S, s, W, H, O.MODE_FULL, 37)
    part, part_id = oracle_samples.render_sample(S, s, W, H, O.MODE_FULL, 37, row0=20, row1=30)
    assert np.array_equal(part[20:30], full[20:30]) and np.array_equal(part_id[20:30], full_id[20:30])
    assert not part[:20].any() and not part[30:].any()


def test_library_exports_the_accumulation_calls(V):
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in ("vrt_accum_begin", "vrt_accum_add", "vrt_accum_resolve", "vrt_accum_resolve_device"):
        assert n in names, f"{n} is not exported by libvrt_hip.so"


def _unopened(V):
    # a Context whose vrt_create never ran: a wrapper that reached the library would fail on the missing handle
    return object.__new__(V.Context)


@pytest.mark.parametrize("args", [(0, 64), (64, 0), (-1, 64), (64.0, 64), (True, 64), (1 << 16, 1 << 15), (64, 64, -1),
                                  (64, 64, 1 << 32), (64, 64, 1.5)])
def test_accum_begin_rejects_bad_arguments_before_the_device(V, args):
    with pytest.raises(ValueError):
        _unopened(V).accum_begin(*args)


@pytest.mark.parametrize("n", [0, -1, (1 << 24) + 1, 2.0, True, None])
def test_accum_add_rejects_bad_arguments_before_the_device(V, n):
    with pytest.raises(ValueError):
        _unopened(V).accum_add(n)


def test_accum_resolve_before_begin_is_refused_before_the_device(V):
    with pytest.raises(V.VrtError):
        _unopened(V).accum_resolve()
