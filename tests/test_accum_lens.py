"""Thin-lens progressive accumulation (vrt_set_lens): what holds without a GPU. The lens sequence is the header's (direction
numbers restated here in Python, the first points, its net properties alone and together with the pixel jitter), the checker
(tests/oracle_lens.c) reproduces oracle_jitter.c's sample at the lens centre and at aperture 0 in every mode, its rays start on
the lens and meet on the plane of focus, and a lens blurs only away from that plane. The dispatcher's proofs (vrt_test_lens_select)
take both sides of every one-eye shortcut. The library exports the call and the Python wrapper refuses bad values before any
device is involved. The kernels are held to the checker on the MI355X (test_gpu_accum_lens.py)."""
import itertools
import subprocess

import numpy as np
import pytest

import oracle_jitter
import oracle_lens

POSES = {   # tests/test_accum_jitter.py's poses
    "dragon": ("dragon", (63.5, 60.5, 140.5, -90.0, -10.0)),
    "nature": ("nature", (60.5, 80.5, 200.5, -90.0, -20.0)),
    "room_inside": ("room", (14.5, 30.5, 16.5, 32.0, -10.0)),
    "room_outside": ("room", (98.5, 34.5, 52.5, 197.0, -8.0)),
    "terrain": ("terrain", (512.5, 420.5, 1000.5, -90.0, -20.0)),
}

# include/vrt.h vrt_set_lens: the first eight (lu, lv)
FIRST = [(0.5, 0.5), (0.0, 0.0), (0.75, 0.25), (0.25, 0.75), (0.125, 0.625), (0.625, 0.125), (0.375, 0.375), (0.875, 0.875)]


def _dirs(poly, m):
    v = [m[0] << 31, m[1] << 30, m[2] << 29]
    for i in range(3, 32):
        x = v[i - 3] ^ (v[i - 3] >> 3)
        if poly & 2:
            x ^= v[i - 1]
        if poly & 1:
            x ^= v[i - 2]
        v.append(x & 0xFFFFFFFF)
    return v


U_DIRS, V_DIRS = _dirs(1, (1, 1, 5)), _dirs(2, (1, 3, 1))


def _g(D, k):
    y = 0
    for i in range(32):
        if (k >> i) & 1:
            y ^= D[i]
    return y


def _lens24(k):
    """(lu, lv) of sample k as 24-bit integers"""
    return (_g(U_DIRS, k) >> 8) ^ 0x800000, (_g(V_DIRS, k) >> 8) ^ 0x800000


def _jitter24(k):
    x = int(f"{k:032b}"[::-1], 2) >> 8
    y, v, i = 0, 1 << 31, k
    while i:
        if i & 1:
            y ^= v
        i >>= 1
        v ^= v >> 1
    return x, y >> 8


def _t_of(points, m, n_dims):
    """the smallest t for which `points` (2^m tuples of 24-bit integers) is a (t, m, n_dims)-net in base 2"""
    for t in range(m + 1):
        ok = True
        for ds in itertools.product(range(m - t + 1), repeat=n_dims):
            if sum(ds) != m - t:
                continue
            cells = {}
            for p in points:
                key = tuple(p[d] >> (24 - ds[d]) for d in range(n_dims))
                cells[key] = cells.get(key, 0) + 1
            if len(cells) != 1 << (m - t) or any(c != 1 << t for c in cells.values()):
                ok = False
                break
        if ok:
            return t
    return None


@pytest.fixture(scope="module")
def LL(tmp_path_factory):
    return oracle_lens.build(tmp_path_factory.mktemp("oracle_lens"))


@pytest.fixture(scope="module")
def J(tmp_path_factory):
    return oracle_jitter.build(tmp_path_factory.mktemp("oracle_jitter"))


def _scene(O, V, product_scenes, name, W, H):
    m, pose = POSES[name]
    tex, dim = product_scenes[m]
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    return O.make_scene(tex, dim, ip, iv, cp), (ip, iv, cp)


def test_direction_numbers_are_the_headers():
    assert U_DIRS[:6] == [0x80000000, 0x40000000, 0xA0000000, 0xD0000000, 0xE8000000, 0x64000000]
    assert V_DIRS[:6] == [0x80000000, 0xC0000000, 0x20000000, 0xB0000000, 0x68000000, 0x4C000000]


def test_checker_sequence_is_the_python_restatement(LL):
    for k, (u, v) in enumerate(FIRST):
        assert oracle_lens.uv(LL, k) == (np.float32(u), np.float32(v)), f"sample {k}"
    for k in list(range(2048)) + [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1, 123456789]:
        u, v = _lens24(k)
        assert oracle_lens.uv(LL, k) == (np.float32(u * 2.0 ** -24), np.float32(v * 2.0 ** -24)), f"sample {k}"


@pytest.mark.parametrize("block", [0, 5])
def test_lens_sequence_nets(block):
    for m in range(1, 11):
        pts = [_lens24((block << m) + k) for k in range(1 << m)]
        t = _t_of(pts, m, 2)
        assert t is not None and t <= 2, f"m={m}: t={t}"
        if m <= 5:
            assert t == 0, f"m={m}: an aligned block of 2^{m} samples is not a (0,{m},2)-net"


def test_lens_and_pixel_offsets_together():
    ts = [_t_of([_jitter24(k) + _lens24(k) for k in range(1 << m)], m, 4) for m in range(1, 10)]
    assert ts == [0, 1, 1, 1, 2, 2, 2, 3, 4]


def test_lens_points_lie_on_the_unit_disc(LL):
    assert oracle_lens.point(LL, 0) == (np.float32(0.0), np.float32(0.0))
    for k in range(1, 4096):
        x, y = oracle_lens.point(LL, k)
        assert float(x) ** 2 + float(y) ** 2 <= 1.0 + 1e-6, f"sample {k}"
    # the concentric map keeps the strata: the first 64 points hit every eighth of the disc's area
    ang = [np.arctan2(*oracle_lens.point(LL, k)[::-1]) for k in range(1, 65)]
    assert len({int(((a + np.pi) / (2 * np.pi)) * 8) % 8 for a in ang}) == 8


@pytest.mark.parametrize("name", sorted(POSES))
def test_checker_lens_centre_and_aperture_zero_are_the_jittered_sample(LL, J, O, V, product_scenes, name):
    W, H = 40, 28
    s, _ = _scene(O, V, product_scenes, name, W, H)
    for mode in (O.MODE_PRIMARY, O.MODE_PRIMARY_SHADOW, O.MODE_FULL):
        for jitter in (False, True):
            for k, ap in ((0, 2.5), (5, 0.0), (2 ** 32 - 1, 0.0)):
                ref = oracle_jitter.render(J, s, W, H, mode, k, jitter=jitter)
                got = oracle_lens.render(LL, s, W, H, mode, k, ap, 7.0, jitter=jitter)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), \
                    f"{name} mode {mode} jitter {jitter} sample {k} aperture {ap}"


@pytest.mark.parametrize("name", ["dragon", "room_inside"])
def test_lens_rays_start_on_the_lens_and_meet_on_the_focus_plane(LL, O, V, product_scenes, name):
    W, H = 32, 24
    s, (ip, iv, cp) = _scene(O, V, product_scenes, name, W, H)
    iv64 = np.array(iv, np.float64)
    R, Uv, Z = iv64[0:3], iv64[4:7], iv64[8:11]
    e = np.array(cp[:3], np.float64)
    aperture, focus = 1.75, 23.0
    moved_any = 0
    for px, py in ((0, 0), (31, 23), (16, 12), (5, 19)):
        hits = []
        for k in range(0, 33):
            for jitter in (False,):
                moved, o, d = oracle_lens.ray(LL, s, W, H, px, py, k, aperture, focus, jitter=jitter)
                o64, d64 = o.astype(np.float64), d.astype(np.float64)
                off = o64 - e
                tol = 4e-7 * (np.abs(e).max() + aperture)
                assert abs(off @ Z) <= tol, "the origin leaves the lens plane"
                assert np.linalg.norm(off) <= aperture * (1 + 1e-6) + tol, "the origin leaves the lens disc"
                assert abs(np.linalg.norm(d64) - 1.0) < 1e-6
                # where the ray meets the plane of focus: -(x - e) . Z = focus
                t = (focus + off @ Z) / -(d64 @ Z)
                hits.append(o64 + t * d64)
                moved_any += moved
                if k == 0:
                    assert not moved
        hits = np.array(hits)
        spread = np.abs(hits - hits[0]).max()
        assert spread <= 2e-5 * (focus + np.abs(e).max()), f"pixel ({px}, {py}): the rays miss each other by {spread}"
    assert moved_any > 100


def _focus_world(V):
    """a wall x in [0, 40), y in [0, 30), z = 0 and a block x in [12, 20), y in [10, 18), z in [18, 20) in front of it"""
    w = V.World()
    for x in range(40):
        for y in range(30):
            w.insert(x, y, 0, 0xC08040FF if (x + y) % 2 else 0x4080C0FF, 3.0, 0.0, 0.0)
    for x in range(12, 20):
        for y in range(10, 18):
            for z in (18, 19):
                w.insert(x, y, z, 0x30C030FF if (x + y + z) % 2 else 0xC03030FF, 3.0, 0.0, 0.0)
    out = w.flatten()
    w.close()
    return out


def test_lens_blurs_only_away_from_the_focus_plane(LL, O, V):
    tex, dim = _focus_world(V)
    W, H = 48, 36
    eye = (20.3, 15.2, 40.7)
    ip, iv, cp, _ = V.camera_block(eye, -90.0, 0.0, W, H)
    s = O.make_scene(tex, dim, ip, iv, cp)
    focus = eye[2] - 1.0                      # the wall's face z = 1
    _, id0 = oracle_lens.render(LL, s, W, H, O.MODE_PRIMARY, 0, 1.5, focus)
    ids = id0[..., 0]
    near = (id0[..., 1] < 30) & (ids != 0)    # the block, ~21 units away
    wall = (id0[..., 1] >= 30) & (ids != 0)
    # keep the wall's pixels away from the block's blur: the block's rays can cover the wall behind it
    ys, xs = np.nonzero(near)
    clear = wall.copy()
    clear[max(ys.min() - 4, 0):ys.max() + 5, max(xs.min() - 4, 0):xs.max() + 5] = False
    assert near.sum() > 60 and clear.sum() > 300
    same_wall, same_near, n = 0.0, 0.0, 0
    for k in range(1, 17):
        _, idk = oracle_lens.render(LL, s, W, H, O.MODE_PRIMARY, k, 1.5, focus)
        same_wall += (idk[..., 0] == ids)[clear].mean()
        same_near += (idk[..., 0] == ids)[near].mean()
        n += 1
    assert same_wall / n >= 0.97, f"the wall at the focus distance kept its voxel in {same_wall / n:.3f} of its pixels"
    assert same_near / n <= 0.6, f"the block away from the focus plane kept its voxel in {same_near / n:.3f} of its pixels"


def test_dispatcher_proofs_take_both_sides(V, product_scenes):
    """vrt_test_lens_select: a small lens inside one empty node shares everything the eye gives; a lens across node
    boundaries looks its media up per lane and loses the host's first lookup; one reaching into the room's glass leaves the v4
    primary kernels and the opaque chain; one reaching out of wide root 0's cube keeps the untightened root."""
    def choice(name, ap):
        m, pose = POSES[name]
        _, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], 64, 48)
        return V.lens_choice(product_scenes[m][0], cp, iv, ap)
    small = choice("dragon", 0.1)
    assert small["box_valid"] and small["eye_shared"] and small["first_shared"] and small["no_medium"] and small["empty"]
    assert small["lo"] == small["hi"] == (63, 60, 140)
    wide = choice("terrain", 3.0)
    assert wide["box_valid"] and not wide["eye_shared"] and not wide["first_shared"] and wide["no_medium"] and wide["empty"]
    glass = choice("room_inside", 40.0)
    assert not glass["no_medium"] and not glass["empty"] and glass["root_shift"] == 10
    assert choice("room_inside", 0.4)["root_shift"] == 8
    # a non-finite extent proves nothing
    _, iv, cp, _ = V.camera_block((63.5, 60.5, 140.5), -90.0, -10.0, 64, 48)
    huge = V.lens_choice(product_scenes["dragon"][0], cp, iv, 3.0e38)
    assert not huge["box_valid"] and not huge["eye_shared"] and not huge["first_shared"] and not huge["no_medium"]


def test_library_exports_set_lens(V):
    out = subprocess.run(["nm", "-D", "--defined-only", V.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "vrt_set_lens" in names
    assert "vrt_test_lens_select" not in names


def _unopened(V):
    # a Context whose vrt_create never ran: a wrapper that reached the library would fail on the missing handle
    return object.__new__(V.Context)


@pytest.mark.parametrize("args", [(-1.0, 5.0), (-1e-30, 5.0), (float("nan"), 5.0), (float("inf"), 5.0), (1e39, 5.0),
                                  (1.0, 0.0), (1.0, -2.0), (1.0, float("nan")), (1.0, float("inf")), (1.0, 1e39),
                                  (True, 5.0), (1.0, None), ("1", 5.0)])
def test_set_lens_rejects_bad_values_before_the_device(V, args):
    with pytest.raises(ValueError):
        _unopened(V).set_lens(*args)
