"""Adaptive accumulation on the MI355X (vrt_accum_begin_adaptive, vrt_accum_counts) against the round semantics of
tests/oracle_adaptive.py applied to the checker's samples (tests/oracle_lens.c, which is tests/oracle_jitter.c's sample at
aperture 0): per-pixel counts and resolved bytes in all three modes, with and without jitter and a lens, on every scene shape and
the records upload. min == max is the plain accumulation under every variant and option; chunking changes nothing; a 1080p
frame matches its own single-sample accumulations; the restart rule, the error codes and plain work around an adaptive one."""
import numpy as np
import pytest

import oracle_adaptive as A
import oracle_jitter
import oracle_lens
from test_gpu_accum_jitter import SCENES, _same, _setup
from test_gpu_accum_lens import LENS

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)
TOLS = (0, 24, 200)
ROUNDS = 16
FIRST = 3


@pytest.fixture(scope="module")
def LL(tmp_path_factory):
    return oracle_lens.build(tmp_path_factory.mktemp("oracle_lens"))


@pytest.fixture(scope="module")
def J(tmp_path_factory):
    return oracle_jitter.build(tmp_path_factory.mktemp("oracle_jitter"))


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def _adaptive(ctx, W, H, mode, first, chunks, jitter, rule):
    ctx.accum_begin(W, H, first, mode=mode, jitter=jitter, adaptive=rule)
    total = 0
    for n in chunks:
        total += n
        assert ctx.accum_add(n) == total
    counts, active = ctx.accum_counts()
    return counts, active, ctx.accum_resolve()


def _check_scene(ctx, LL, J, O, scene, W, H, what, lens):
    for mode in MODES:
        _, frame_id = oracle_jitter.render(J, scene, W, H, mode, 0, jitter=False)
        for jitter in (False, True):
            for ap, focus in ((0.0, 1.0), lens):
                cache = {}

                def sample(k):
                    if k not in cache:
                        cache[k] = oracle_lens.render(LL, scene, W, H, mode, k, ap, focus, jitter=jitter)[0]
                    return cache[k]

                ctx.set_lens(ap, focus)
                try:
                    for tol in TOLS:
                        rule = (2, 12, tol)
                        ref = A.accumulate(sample, H, W, FIRST, ROUNDS, rule)
                        counts, active, (rgba, idd, shown) = _adaptive(ctx, W, H, mode, FIRST, [ROUNDS], jitter, rule)
                        tag = f"{what} mode {mode} jitter {jitter} aperture {ap} tolerance {tol}"
                        assert np.array_equal(counts, ref.counts()), f"{tag}: counts differ at {np.argwhere(counts != ref.counts())[:3]}"
                        assert active == int(ref.active(rule).sum()), tag
                        want = ref.resolve()
                        _same(rgba, want, f"{tag} rgba8")
                        _same(idd, frame_id, f"{tag} id_dist")
                        _same(shown, O.denoise(want, frame_id), f"{tag} shown")
                finally:
                    ctx.set_lens(0.0, 1.0)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_counts_and_bytes_are_the_oracle_rounds(ctx, V, O, LL, J, product_scenes, name):
    m, W, H, pose = SCENES[name]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    _check_scene(ctx, LL, J, O, scene, W, H, name, LENS[name])


def test_record_only_upload(ctx, V, O, LL, J, product_scenes):
    import os
    from conftest import MAPS
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    rec = w.records()
    w.close()
    m, W, H, pose = SCENES["dragon"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose, records=rec)
    _check_scene(ctx, LL, J, O, scene, W, H, "records", LENS["dragon"])


def test_device_rule_is_the_host_rule(V):
    rng = np.random.default_rng(7)
    n = np.concatenate([rng.integers(0, 1 << 24, 4000), [0, 1, 2, 3, (1 << 24) - 1, 1 << 24]]).astype(np.uint32)
    # states samples can reach: two-valued samples a (n - j times) and b (j times)
    a = rng.integers(0, 766, n.size)
    b = rng.integers(0, 766, n.size)
    j = (rng.random(n.size) * (n.astype(np.float64) + 1)).astype(np.int64)
    nn = n.astype(object)
    s = [int(x) for x in (nn - j) * a + j * b]
    q = [int(x) for x in (nn - j) * a * a + j * b * b]
    for lo, hi, tol in ((2, 1 << 24, 0), (2, 1 << 24, 1), (16, 4096, 24), (2, 1 << 24, 65535), (1 << 24, 1 << 24, 7)):
        got = V.adaptive_rule_device(n, np.array(s, np.uint64), np.array(q, np.uint64), lo, hi, tol)
        want = [A.active(n[i], s[i], q[i], lo, hi, tol) for i in range(n.size)]
        assert list(got) == want, (lo, hi, tol)


def _plain(ctx, W, H, mode, first, chunks, jitter):
    ctx.accum_begin(W, H, first, mode=mode, jitter=jitter)
    for c in chunks:
        ctx.accum_add(c)
    return ctx.accum_resolve()


def _equal_to_plain(ctx, W, H, what, lens):
    for mode in MODES:
        for jitter in (False, True):
            for ap, focus in ((0.0, 1.0), lens):
                ctx.set_lens(ap, focus)
                try:
                    ref = _plain(ctx, W, H, mode, 11, [2, 3], jitter)
                    counts, active, got = _adaptive(ctx, W, H, mode, 11, [2, 3, 1], jitter, (5, 5, 0))
                finally:
                    ctx.set_lens(0.0, 1.0)
                tag = f"{what} mode {mode} jitter {jitter} aperture {ap}"
                assert (counts == 5).all() and active == 0, tag
                for a, b, w in zip(ref, got, ("rgba8", "id_dist", "shown")):
                    _same(b, a, f"{tag}: {w}")


def test_min_equal_max_is_the_plain_accumulation(ctx, V, O, product_scenes):
    settings = [(V.OPT_RAY_TABLES, 0), (V.OPT_EMPTY_OCTANTS, 0), (V.OPT_EMPTY_OCTANTS, 2), (V.OPT_FULL_OPAQUE, 0)]
    defaults = {V.OPT_RAY_TABLES: 1, V.OPT_EMPTY_OCTANTS: 1, V.OPT_FULL_OPAQUE: 1}
    for name in ("dragon", "room_outside"):   # the opaque path and the general one
        m, W, H, pose = SCENES[name]
        _setup(ctx, V, O, product_scenes, m, W, H, pose)
        try:
            _equal_to_plain(ctx, W, H, name, LENS[name])
            for opt, val in settings:
                ctx.set_option(opt, val)
                _equal_to_plain(ctx, W, H, f"{name} option {opt}={val}", LENS[name])
                ctx.set_option(opt, defaults[opt])
            for var in V.available_variants():
                ctx.set_variant(var)
                _equal_to_plain(ctx, W, H, f"{name} variant {var}", LENS[name])
        finally:
            ctx.set_variant(0)
            for opt, val in defaults.items():
                ctx.set_option(opt, val)


@pytest.mark.parametrize("name", ["nature", "room_inside"])
def test_chunking(ctx, V, O, product_scenes, name):
    m, W, H, pose = SCENES[name]
    _setup(ctx, V, O, product_scenes, m, W, H, pose)
    for mode in MODES:
        for jitter in (False, True):
            for ap, focus in ((0.0, 1.0), LENS[name]):
                ctx.set_lens(ap, focus)
                try:
                    runs = [_adaptive(ctx, W, H, mode, 5, chunks, jitter, (2, 12, 24)) for chunks in ([16], [1] * 16, [3, 5, 8])]
                finally:
                    ctx.set_lens(0.0, 1.0)
                tag = f"{name} mode {mode} jitter {jitter} aperture {ap}"
                for counts, active, res in runs[1:]:
                    assert np.array_equal(counts, runs[0][0]) and active == runs[0][1], tag
                    for a, b, w in zip(runs[0][2], res, ("rgba8", "id_dist", "shown")):
                        _same(b, a, f"{tag}: {w}")


@pytest.mark.parametrize("full_opaque", [1, 0])
def test_1080p_dragon_from_single_samples(ctx, V, O, product_scenes, full_opaque):
    W, H = 1920, 1080
    m, _, _, pose = SCENES["dragon"]
    _setup(ctx, V, O, product_scenes, m, W, H, pose)
    ctx.set_option(V.OPT_FULL_OPAQUE, full_opaque)
    try:
        first, rounds, rule = 100, 32, (4, 32, 24)
        frames = {}
        for k in range(rounds):
            ctx.accum_begin(W, H, first + k, mode=V.MODE_FULL, jitter=True)
            ctx.accum_add(1)
            frames[first + k] = ctx.accum_resolve()[0]
        ref = A.accumulate(lambda k: frames[k], H, W, first, rounds, rule, dtype=np.int64)
        counts, active, (rgba, _, _) = _adaptive(ctx, W, H, V.MODE_FULL, first, [rounds], True, rule)
    finally:
        ctx.set_option(V.OPT_FULL_OPAQUE, 1)
    assert np.array_equal(counts, ref.counts()), f"counts differ at {np.argwhere(counts != ref.counts())[:3]}"
    assert active == int(ref.active(rule).sum())
    _same(rgba, ref.resolve(), "1080p resolve")
    assert 4 <= counts.min() and counts.max() <= 32


def test_restart_rule(ctx, V, O, product_scenes):
    m, W, H, pose = SCENES["dragon"]
    _, cam = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    ctx.accum_begin(W, H, 0, mode=V.MODE_FULL, jitter=True, adaptive=(2, 8, 0))
    counts, active = ctx.accum_counts()
    assert (counts == 0).all() and active == W * H            # no round yet: every pixel active with zero samples
    assert ctx.accum_add(3) == 3
    c3, _ = ctx.accum_counts()
    assert c3.max() == 3 and c3.min() >= 2
    ctx.set_camera(*cam)                                       # the same camera and params again: no restart
    ctx.set_params(ctx.default_params())
    assert ctx.accum_add(2) == 5
    c5, _ = ctx.accum_counts()
    assert (c5 >= c3).all() and c5.max() == 5
    ip, iv, cp, _ = V.camera_block((63.5, 60.5, 141.5), -90.0, -10.0, W, H)
    ctx.set_camera(ip, iv, cp)                                 # moved: the next add starts again at `first`
    assert ctx.accum_add(1) == 1
    c1, active = ctx.accum_counts()
    assert (c1 == 1).all() and active == W * H
    # min == max == 1 round later: every pixel at 2, none active
    ctx.accum_begin(W, H, 0, mode=V.MODE_PRIMARY, jitter=False, adaptive=(2, 2, 0))
    ctx.accum_add(5)
    c, active = ctx.accum_counts()
    assert (c == 2).all() and active == 0


def test_error_codes(V, product_scenes):
    c = V.Context(0)
    try:
        L, h = c._L, c._h
        assert L.vrt_accum_counts(h, None) == -5                    # before any begin
        assert L.vrt_accum_counts(None, None) == -1
        for lo, hi, tol in ((1, 8, 0), (0, 8, 0), (9, 8, 0), (2, (1 << 24) + 1, 0), (2, 8, 65536), (2, 0xFFFFFFFF, 0)):
            assert L.vrt_accum_begin_adaptive(h, 16, 16, 2, 0, 0, lo, hi, tol) == -1, (lo, hi, tol)
        assert L.vrt_accum_begin_adaptive(h, 16, 16, 7, 0, 0, 2, 8, 0) == -1         # unknown mode
        assert L.vrt_accum_begin_adaptive(h, 16, 16, 2, 0, 2, 2, 8, 0) == -1         # unknown flag
        assert L.vrt_accum_begin_adaptive(h, 0, 16, 2, 0, 0, 2, 8, 0) == -1          # no frame
        assert L.vrt_accum_begin_adaptive(None, 16, 16, 2, 0, 0, 2, 8, 0) == -1
        assert L.vrt_accum_counts(h, None) == -5                    # still nothing begun
        assert L.vrt_accum_begin_adaptive(h, 16, 16, 2, 0, 0, 2, 1 << 24, 65535) == 0
        assert L.vrt_accum_counts(h, None) == 16 * 16
        assert L.vrt_accum_begin_ex(h, 16, 16, 2, 0, 0) == 0
        assert L.vrt_accum_counts(h, None) == -5                    # a plain accumulation
        tex, dim = product_scenes["dragon"]
        c.upload_octree(tex, dim)
        ip, iv, cp, _ = V.camera_block((63.5, 60.5, 140.5), -90.0, -10.0, 16, 16)
        c.set_camera(ip, iv, cp)
        c.accum_begin(16, 16, 0, mode=V.MODE_PRIMARY, jitter=True, adaptive=(2, 4, 0))
        assert c.accum_add((1 << 24) - 1) == (1 << 24) - 1          # rounds, looped in the lanes: each stops at its pixel's stop
        with pytest.raises(V.VrtError):
            c.accum_add(2)                                          # the 2^24 cap counts rounds
        counts, active = c.accum_counts()
        assert active == 0 and counts.max() <= 4 and counts.min() >= 2
    finally:
        c.close()


def test_frames_and_plain_accumulations_around_an_adaptive_one(ctx, V, O, product_scenes):
    m, W, H, pose = SCENES["room_outside"]
    scene, _ = _setup(ctx, V, O, product_scenes, m, W, H, pose)
    plain = {mode: _plain(ctx, W, H, mode, 3, [4], True) for mode in MODES}
    for mode in MODES:
        _adaptive(ctx, W, H, mode, 3, [2, 2], True, (2, 6, 24))
        ref_rgba, ref_id, _, _ = O.render(scene, W, H, mode)
        rgba, idd = ctx.dispatch(W, H, mode)
        _same(rgba, ref_rgba, f"mode {mode} frame after an adaptive accumulation")
        _same(idd, ref_id, f"mode {mode} frame id_dist after an adaptive accumulation")
    for mode in MODES:
        again = _plain(ctx, W, H, mode, 3, [4], True)
        for a, b, what in zip(plain[mode], again, ("rgba8", "id_dist", "shown")):
            _same(b, a, f"mode {mode} plain accumulation around an adaptive one: {what}")
