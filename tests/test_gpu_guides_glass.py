"""Guides past glass on the MI355X (vrt_set_guide_glass; rule G0-G6 of include/vrt.h) against the checker
(tests/oracle_guides_glass.c), bit for bit on all four planes: every ray source of an accumulation on both traversal routes at a
frame of whole tiles and a ragged one, any split of the samples over calls, adaptive accumulations, the setting read at the begin
and at no other time, the setting off, a world without glass, the hand-built worlds of tests/glass_worlds.py, ray batches as a list
and as an image, the device forms on a caller's stream, the four filtered and temporal accumulation routes, the accumulation's own
resolves, and the error code."""
import os

import numpy as np
import pytest

from conftest import MAPS
import emit_worlds
import glass_worlds as GL
import guide_worlds as GW
import oracle_guides as G
import oracle_guides_glass as GG
from test_gpu_shade_rays import _materials_world, _ray_mix

pytestmark = pytest.mark.gpu

W, H, FIRST, N = GW.W, GW.H, GW.FIRST, GW.N
VARIANTS = (0, 1)          # the default wide traversal and the record-array route
MODE_FULL, MODE_PRIMARY = 2, 0
RAY_KEYS = ("normal", "albedo", "depth", "hit")


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return GG.build(tmp_path_factory.mktemp("oracle_guides_glass"))


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def worlds(V, O):
    """name, and (name, size) for the ragged frame -> (texels, tex_dim, camera block, oracle scene)"""
    out = {}
    for name in GW.FRAMES:
        w = GW.world(V, name)
        tex, dim = w.flatten()
        w.close()
        for key, size in ((name, (W, H)), ((name, GW.RAGGED), GW.RAGGED)):
            cam = GW.camera(V, name, size)
            out[key] = (tex, dim, cam, O.make_scene(tex, dim, *cam))
    return out


_refs = {}


def _ref(L, worlds, name, source, first=FIRST, n=N, size=(W, H), glass=True):
    """the checker's planes of samples first .. first + n - 1, past glass or plain, computed once"""
    key = (name, source, first, n, size, glass)
    if key not in _refs:
        jitter, _ = GW.SOURCES[source]
        scene = worlds[name if size == (W, H) else (name, size)][3]
        _refs[key] = (GG if glass else G).planes(L, scene, size[0], size[1], first, n, jitter, *GW.lens_of(name, source))[0]
    return _refs[key]


def _open(ctx, worlds, name, source, mode=MODE_FULL, first=FIRST, size=(W, H), glass=True, **kw):
    tex, dim, cam, _ = worlds[name if size == (W, H) else (name, size)]
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    ctx.set_camera(*cam)
    ctx.set_lens(*GW.lens_of(name, source))
    ctx.set_guide_glass(glass)
    ctx.accum_begin(size[0], size[1], first, mode=mode, jitter=GW.SOURCES[source][0], **kw)
    return cam


@pytest.fixture(autouse=True)
def _defaults(ctx):
    yield
    ctx.set_variant(0)
    ctx.set_lens(0.0, 1.0)
    ctx.set_guide_glass(False)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("source", sorted(GW.SOURCES))
@pytest.mark.parametrize("name", sorted(GW.FRAMES))
@pytest.mark.parametrize("size", [(W, H), GW.RAGGED], ids=["40x24", "43x21"])
def test_planes_are_the_checkers_under_any_split(ctx, L, worlds, size, name, source, variant):
    """8 samples from first_sample 5: one guide call after all of them, and calls after 3 and after 8, give the checker's past-glass
    planes; they are not the plain planes"""
    ctx.set_variant(variant)
    want = _ref(L, worlds, name, source, size=size)
    what = f"{name} {size} {source} variant {variant}"
    _open(ctx, worlds, name, source, size=size)
    assert ctx.guide_glass is True
    assert ctx.accum_add(N) == N
    G.same(ctx.accum_guides(), want, f"{what}: one call")
    _open(ctx, worlds, name, source, size=size)
    assert ctx.accum_add(3) == 3
    G.same(ctx.accum_guides(), _ref(L, worlds, name, source, FIRST, 3, size), f"{what}: after 3")
    assert ctx.accum_add(N - 3) == N
    G.same(ctx.accum_guides(), want, f"{what}: after 3 and 8")
    plain = _ref(L, worlds, name, source, size=size, glass=False)
    assert not np.array_equal(plain["depth"], want["depth"]) and not np.array_equal(plain["albedo"], want["albedo"])


def test_adaptive_accumulations_take_every_round(ctx, L, worlds):
    name, source = "lamp", "jitter_lens"
    _open(ctx, worlds, name, source, adaptive=(2, 64, 65535))
    assert ctx.accum_add(3) == 3
    ctx.accum_guides()
    assert ctx.accum_add(N - 3) == N
    counts, _ = ctx.accum_counts()
    assert (counts < N).any()
    G.same(ctx.accum_guides(), _ref(L, worlds, name, source), "adaptive")


def test_the_setting_is_read_at_the_begin(ctx, L, worlds):
    """changed after the begin it has no effect until the next begin, whichever way, and it restarts nothing"""
    name, source = "lamp", "jitter"
    _open(ctx, worlds, name, source, glass=False)
    assert ctx.accum_add(3) == 3
    ctx.set_guide_glass(True)
    G.same(ctx.accum_guides(), _ref(L, worlds, name, source, FIRST, 3, glass=False), "begun off, set on: still plain")
    assert ctx.accum_add(N - 3) == N                                       # no restart: the sums go on
    G.same(ctx.accum_guides(), _ref(L, worlds, name, source, glass=False), "begun off, set on, more samples: still plain")
    ctx.accum_begin(W, H, FIRST, mode=MODE_FULL, jitter=True)              # the next begin reads it
    assert ctx.accum_add(3) == 3
    ctx.set_guide_glass(False)
    G.same(ctx.accum_guides(), _ref(L, worlds, name, source, FIRST, 3), "begun on, set off: still past glass")
    assert ctx.accum_add(N - 3) == N
    G.same(ctx.accum_guides(), _ref(L, worlds, name, source), "begun on, set off, more samples: still past glass")


@pytest.mark.parametrize("name", sorted(GW.FRAMES))
def test_the_setting_off_gives_the_plain_planes(ctx, worlds, name):
    """... those of tests/oracle_guides.c, from the library tests/oracle_guides.py builds, after the setting has been on"""
    import tempfile
    source = "jitter_lens"
    with tempfile.TemporaryDirectory() as tmp:
        L0 = G.build(tmp)
        want = G.planes(L0, worlds[name][3], W, H, FIRST, N, True, *GW.lens_of(name, source))[0]
    _open(ctx, worlds, name, source, glass=True)
    assert ctx.accum_add(1) == 1
    ctx.accum_guides()
    _open(ctx, worlds, name, source, glass=False)
    assert ctx.guide_glass is False
    assert ctx.accum_add(N) == N
    G.same(ctx.accum_guides(), want, f"{name}: off")


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_world_without_glass_gives_the_same_bytes_on_and_off(ctx, V, variant):
    """the dragon: no translucent leaf, so the dispatcher takes the plain kernels under the default traversal; the record-array route
    runs the past-glass form, whose chain ends on the first surface"""
    w = V.World()
    assert w.load_vox(os.path.join(MAPS, "dragon.vox"))
    tex, dim = w.flatten()
    w.close()
    pose = emit_worlds.DRAGON_POSE
    cam = V.camera_block(pose[:3], pose[3], pose[4], *GW.RAGGED)[:3]
    ctx.set_variant(variant)
    out = []
    for glass in (False, True):
        ctx.upload_octree(tex, dim)
        ctx.set_params(ctx.default_params())
        ctx.set_camera(*cam)
        ctx.set_lens(0.8, 60.0)
        ctx.set_guide_glass(glass)
        ctx.accum_begin(*GW.RAGGED, FIRST, mode=MODE_PRIMARY, jitter=True)
        assert ctx.accum_add(4) == 4
        out.append(ctx.accum_guides())
        o, d = np.array(pose[:3], np.float32), np.random.default_rng(2).normal(size=(1000, 3)).astype(np.float32)
        out[-1].update({"ray_" + k: v for k, v in ctx.guide_rays(o, d).items()})
    assert 0.05 < float(out[0]["coverage"].mean()) < 1.0 and out[0]["ray_hit"].sum() > 20
    for k in out[0]:
        assert np.array_equal(out[0][k].view(np.uint8), out[1][k].view(np.uint8)), k


# ---- hand-built worlds -------------------------------------------------------------------------------------------------------------
def _hand_built(ctx, V, O, L, voxels, o, d, variant):
    tex, dim = GL.build(V, voxels)
    cam = V.camera_block(GL.EYE, 0, 0, 8, 8)[:3]
    scene = O.make_scene(tex, dim, *cam)
    ctx.set_variant(variant)
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    ctx.set_guide_glass(True)
    got = ctx.guide_rays(o, d)
    G.same(got, GG.ray_planes(L, scene, o, d), "hand-built world", keys=RAY_KEYS)
    return got, GG.rays(L, scene, o, d)


@pytest.mark.parametrize("variant", VARIANTS)
def test_ten_panes_end_on_the_eighth_surface(ctx, V, O, L, variant):
    got, g = _hand_built(ctx, V, O, L, GL.ten_panes(), *GL.axis_rays(), variant)
    assert got["hit"].all() and (g.surfaces == 8).all() and (g.cell[:, 0] == GL.PANES_X[3] + 1).all()
    assert np.array_equal(got["albedo"], np.tile((np.array(GL.GLASS_BYTES, np.float64) / 255.0).astype(np.float32), (5, 1)))


@pytest.mark.parametrize("variant", VARIANTS)
def test_beyond_the_critical_angle_the_chain_ends_on_glass(ctx, V, O, L, variant):
    got, g = _hand_built(ctx, V, O, L, GL.tir_block(), np.array(GL.TIR_EYE, np.float32), np.array([GL.TIR_DIR], np.float32), variant)
    assert got["hit"][0] and g.surfaces[0] == 1 and got["albedo"][0, 3] < 1.0
    assert np.array_equal(got["normal"][0], np.array([-1, 0, 0], np.float32))


@pytest.mark.parametrize("variant", VARIANTS)
def test_pane_and_slab_worlds(ctx, V, O, L, variant):
    """a wall through a pane along +x and -x, through a thick slab at 45 degrees, and sky through a pane (a miss: all zeros)"""
    for back in (False, True):
        got, g = _hand_built(ctx, V, O, L, GL.pane_wall(back), *GL.axis_rays(back=back), variant)
        assert got["hit"].all() and (g.surfaces == 3).all()
        assert np.array_equal(got["albedo"][:, 3], np.full(5, np.float32(GL.GLASS_ALPHA / 255.0)))
    got, g = _hand_built(ctx, V, O, L, GL.oblique_slab(), np.array(GL.SLAB_EYE, np.float32), np.array([GL.SLAB_DIR], np.float32), variant)
    assert got["hit"][0] and tuple(g.cell[0]) == (GL.SLAB_WALL_X, 10, int(np.floor(GL.oblique_slab_closed_form()[0])))
    got, g = _hand_built(ctx, V, O, L, GL.pane_sky(), *GL.axis_rays(), variant)
    assert not got["hit"].any() and not got["normal"].any() and not got["albedo"].any() and not got["depth"].any()


# ---- ray batches -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def materials(V, O):
    w = _materials_world(V)
    tex, dim = w.flatten()
    w.close()
    cam = V.camera_block((12.5, 10.5, 40.5), -90.0, -10.0, W, H)[:3]
    return tex, dim, O.make_scene(tex, dim, *cam)


@pytest.mark.parametrize("variant", VARIANTS)
def test_picking_rays_from_the_lamp_rooms_eye(ctx, L, worlds, variant):
    tex, dim, _, scene = worlds["lamp"]
    ctx.set_variant(variant)
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    ctx.set_guide_glass(True)
    o, d = GW.picking_rays()
    want = GG.ray_planes(L, scene, o, d)
    G.same(ctx.guide_rays(o, d), want, f"300 picking rays, variant {variant}", keys=RAY_KEYS)
    plain = G.ray_planes(L, scene, o, d)
    through = plain["hit"] & (plain["albedo"][:, 3] < 1.0)
    assert through.sum() > 10 and want["hit"].all()
    assert (want["depth"][through] > plain["depth"][through]).all()        # the surface behind the pane is further than the pane
    ctx.set_guide_glass(False)                                             # read at the call
    G.same(ctx.guide_rays(o, d), plain, "off again", keys=RAY_KEYS)


@pytest.mark.parametrize("variant", VARIANTS)
def test_an_image_of_rays_with_every_kind_of_origin_and_direction(ctx, L, materials, variant):
    """24 x 13: origins in empty space, in glass, in a solid, on faces and outside the world, directions axis-parallel, with zero and
    tiny components, of lengths 1e-3 .. 1e3 (tests/test_gpu_shade_rays.py _ray_mix); as an image, as a list, with one shared origin"""
    tex, dim, scene = materials
    ctx.set_variant(variant)
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    ctx.set_guide_glass(True)
    n = 24 * 13
    o, d = _ray_mix(np.random.default_rng(21 + n), n, (0, 0, 0), (50, 24, 24), ((30, 2, 8), (36, 8, 14)), ((30, 2, 16), (36, 8, 22)))
    want = GG.ray_planes(L, scene, o, d)
    plain = G.ray_planes(L, scene, o, d)
    assert 30 < want["hit"].sum() < n and not np.array_equal(want["depth"], plain["depth"])
    G.same(ctx.guide_rays(o, d, width=24), want, f"24 x 13, variant {variant}", keys=RAY_KEYS)
    G.same(ctx.guide_rays(o, d), want, "as a list", keys=RAY_KEYS)
    eye = np.array([31.5, 4.5, 10.5], np.float32)                           # one origin for the batch, inside the first box
    G.same(ctx.guide_rays(eye, d, width=24), GG.ray_planes(L, scene, eye, d), "shared origin in glass", keys=RAY_KEYS)


def test_device_forms_on_a_callers_stream(ctx, V, L, worlds):
    import torch
    name, source = "lamp", "lens"
    _open(ctx, worlds, name, source)
    assert ctx.accum_add(N) == N
    bufs = {"normal": torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0"), "albedo": torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0"),
            "depth": torch.zeros((H, W), dtype=torch.float32, device="cuda:0"), "coverage": torch.zeros((H, W), dtype=torch.float32, device="cuda:0")}
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    ctx.accum_guides_device(*(bufs[k].data_ptr() for k in G.KEYS), stream=side.cuda_stream)
    torch.cuda.synchronize()
    G.same({k: bufs[k].cpu().numpy() for k in G.KEYS}, _ref(L, worlds, name, source), "accum_guides_device on a side stream")
    # ray batches: read at the call
    scene = worlds[name][3]
    o, d = GW.picking_rays()
    o3 = np.tile(o, (len(d), 1))
    d_o, d_d = torch.from_numpy(o3).to("cuda:0"), torch.from_numpy(d).to("cuda:0")
    d_n = torch.zeros((300, 3), dtype=torch.float32, device="cuda:0")
    d_a = torch.zeros((300, 4), dtype=torch.float32, device="cuda:0")
    d_z = torch.zeros(300, dtype=torch.float32, device="cuda:0")
    d_h = torch.zeros(300, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.set_guide_glass(True)
    ctx.guide_rays_device(300, d_o.data_ptr(), 3, d_d.data_ptr(), d_n.data_ptr(), d_a.data_ptr(), d_z.data_ptr(), d_h.data_ptr(),
                          stream=side.cuda_stream)
    torch.cuda.synchronize()
    got = {"normal": d_n.cpu().numpy(), "albedo": d_a.cpu().numpy(), "depth": d_z.cpu().numpy(), "hit": d_h.cpu().numpy() != 0}
    G.same(got, GG.ray_planes(L, scene, o, d), "guide_rays_device on a side stream", keys=RAY_KEYS)


# ---- the routes that bring the guide state up to date themselves -------------------------------------------------------------------
def _same_arrays(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, i)


@pytest.mark.parametrize("route", ["filtered", "filtered_var", "temporal", "temporal_mom"])
def test_accumulation_routes_use_the_state_as_begun(ctx, L, worlds, route):
    """each of the four equals the stateless call fed with the device's own past-glass planes -- which are the checker's -- and
    differs from the same route of an accumulation begun with the setting off"""
    name, source = "lamp", "corner"
    moments = route in ("filtered_var", "temporal_mom")

    def run(glass):
        cam = _open(ctx, worlds, name, source, glass=glass, hdr=True, moments=moments)
        assert ctx.accum_add(4) == 4
        ctx.set_guide_glass(not glass)                                     # after the begin: no effect
        if route == "filtered":
            got = ctx.accum_resolve_hdr_filtered()
        elif route == "filtered_var":
            got = ctx.accum_resolve_hdr_filtered_var()
        elif route == "temporal":
            got = ctx.accum_resolve_hdr_temporal()
        else:
            got = ctx.accum_resolve_hdr_temporal_mom()
        return cam, got

    _, off = run(False)
    cam, got = run(True)
    planes = ctx.accum_guides()
    G.same(planes, _ref(L, worlds, name, source, FIRST, 4), "the planes the route used")
    mean = ctx.accum_resolve_hdr()[0]
    if route == "filtered":
        want = ctx.filter_hdr(mean, planes)
    elif route == "filtered_var":
        want = ctx.filter_hdr_var(mean, planes, ctx.accum_variance())
    else:
        if route == "temporal":
            hist, integ, var = ctx.temporal_hdr(cam, mean, planes)
        else:
            hist, integ, var = ctx.temporal_hdr_mom(cam, mean, planes, ctx.accum_variance())
        want = (hist, integ) + tuple(ctx.filter_hdr_var(integ, planes, var))
    _same_arrays(got, want, route)
    assert not np.array_equal(got[-3 if route != "filtered" else 0], off[-3 if route != "filtered" else 0]), "the filtered floats differ from the plain route's"


@pytest.mark.parametrize("adaptive", [None, (2, 6, 40)])
def test_the_accumulations_own_resolves_and_counts_do_not_change(ctx, worlds, adaptive):
    name, source = "lamp", "jitter"
    kw = {"adaptive": adaptive} if adaptive else {}

    def run(glass):
        _open(ctx, worlds, name, source, glass=glass, hdr=True, **kw)
        ctx.accum_add(3)
        ctx.accum_guides()
        mid = ctx.accum_resolve() + ctx.accum_resolve_hdr()
        ctx.accum_add(N - 3)
        ctx.accum_guides()
        out = mid + ctx.accum_resolve() + ctx.accum_resolve_hdr()
        return out + ((ctx.accum_counts()[0],) if adaptive else ())

    off, on = run(False), run(True)
    assert len(off) == len(on) >= 12
    for a, b in zip(off, on):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_a_value_of_2_is_invalid(ctx, V):
    assert ctx._L.vrt_set_guide_glass(ctx._h, 2) == -1                     # VRT_E_INVALID
    assert ctx._L.vrt_set_guide_glass(ctx._h, -1) == -1
    assert ctx._L.vrt_set_guide_glass(None, 1) == -1
    with pytest.raises(ValueError):
        ctx.set_guide_glass(2)
    ctx.set_guide_glass(1)
    assert ctx.guide_glass is True
