"""Guide planes on the MI355X (vrt_accum_guides, vrt_guide_rays) against the checker (tests/oracle_guides.c), bit for bit: every
ray source of an accumulation on both traversal routes, any split of the samples over calls, the restart rule, adaptive
accumulations, the device form on a caller's stream, the error code, the accumulation's own resolves untouched, and ray batches
as a list and as an image with every kind of origin and direction vrt_shade_rays takes."""
import ctypes as C

import numpy as np
import pytest

import guide_worlds as GW
import oracle_guides as G
from test_gpu_shade_rays import _materials_world, _ray_mix

pytestmark = pytest.mark.gpu

W, H, FIRST, N = GW.W, GW.H, GW.FIRST, GW.N
VARIANTS = (0, 1)          # the default wide traversal and the record-array route
MODE_FULL, MODE_PRIMARY = 2, 0


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return G.build(tmp_path_factory.mktemp("oracle_guides"))


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


def _ref(L, worlds, name, source, first=FIRST, n=N, size=(W, H)):
    """the checker's planes of samples first .. first + n - 1, computed once"""
    key = (name, source, first, n, size)
    if key not in _refs:
        jitter, _ = GW.SOURCES[source]
        scene = worlds[name if size == (W, H) else (name, size)][3]
        _refs[key] = G.planes(L, scene, size[0], size[1], first, n, jitter, *GW.lens_of(name, source))[0]
    return _refs[key]


def _open(ctx, worlds, name, source, mode=MODE_FULL, first=FIRST, size=(W, H), **kw):
    tex, dim, cam, _ = worlds[name if size == (W, H) else (name, size)]
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    ctx.set_camera(*cam)
    ctx.set_lens(*GW.lens_of(name, source))
    ctx.accum_begin(size[0], size[1], first, mode=mode, jitter=GW.SOURCES[source][0], **kw)


@pytest.fixture(autouse=True)
def _defaults(ctx):
    yield
    ctx.set_variant(0)
    ctx.set_lens(0.0, 1.0)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("source", sorted(GW.SOURCES))
@pytest.mark.parametrize("name", sorted(GW.FRAMES))
@pytest.mark.parametrize("size", [(W, H), GW.RAGGED], ids=["40x24", "43x21"])
def test_planes_are_the_checkers_under_any_split(ctx, L, worlds, size, name, source, variant):
    """8 samples from first_sample 5: one guide call after all of them, and calls after 3 and after 8, give the checker's planes;
    at 40 x 24 (whole tiles) and at 43 x 21 (partial tiles on the right, a ragged last tile row)"""
    ctx.set_variant(variant)
    want = _ref(L, worlds, name, source, size=size)
    what = f"{name} {size} {source} variant {variant}"
    _open(ctx, worlds, name, source, size=size)
    assert ctx.accum_add(N) == N
    G.same(ctx.accum_guides(), want, f"{what}: one call")
    G.same(ctx.accum_guides(), want, f"{what}: a second call with nothing new")
    _open(ctx, worlds, name, source, size=size)
    assert ctx.accum_add(3) == 3
    G.same(ctx.accum_guides(), _ref(L, worlds, name, source, FIRST, 3, size), f"{what}: after 3")
    assert ctx.accum_add(N - 3) == N
    G.same(ctx.accum_guides(), want, f"{what}: after 3 and 8")
    assert 0.2 < float(want["coverage"].mean()) <= 1.0 and (name != "outside" or (want["coverage"] == 0).sum() > 50)


def test_a_camera_change_restarts_the_guide_state(ctx, V, L, O, worlds):
    name, source = "room", "jitter"
    tex, dim, cam, _ = worlds[name]
    _open(ctx, worlds, name, source)
    assert ctx.accum_add(3) == 3
    G.same(ctx.accum_guides(), _ref(L, worlds, name, source, FIRST, 3), "before the move")
    pose = GW.FRAMES[name][0]
    moved = V.camera_block((pose[0] + 1.25, pose[1], pose[2] - 0.5), pose[3] + 4.0, pose[4], W, H)[:3]
    ctx.set_camera(*moved)
    # the sums still hold the old camera's samples and the state is up to date: the planes resolve as before
    G.same(ctx.accum_guides(), _ref(L, worlds, name, source, FIRST, 3), "moved, nothing added")
    assert ctx.accum_add(2) == 2                                           # the add restarts
    want = G.planes(L, O.make_scene(tex, dim, *moved), W, H, FIRST, 2, True)[0]
    G.same(ctx.accum_guides(), want, "after the move")
    assert not np.array_equal(want["depth"], _ref(L, worlds, name, source, FIRST, 2)["depth"])
    # samples missing and the inputs changed since the last add: nothing to march them with
    assert ctx.accum_add(1) == 3
    ctx.set_camera(*cam)
    with pytest.raises(V.VrtError, match="vrt error -5"):
        ctx.accum_guides()
    assert ctx.accum_add(1) == 1
    G.same(ctx.accum_guides(), _ref(L, worlds, name, source, FIRST, 1), "back again")


def test_adaptive_accumulations_take_every_round(ctx, L, worlds):
    """pixels stop at 2 samples under the widest tolerance; their guides take all 8 rounds all the same"""
    name, source = "lamp", "jitter_lens"
    _open(ctx, worlds, name, source, adaptive=(2, 64, 65535))
    assert ctx.accum_add(3) == 3
    ctx.accum_guides()
    assert ctx.accum_add(N - 3) == N
    counts, _ = ctx.accum_counts()
    assert (counts < N).any()
    G.same(ctx.accum_guides(), _ref(L, worlds, name, source), "adaptive")


def test_host_and_device_forms_agree_on_a_callers_stream(ctx, L, worlds):
    import torch
    name, source = "room", "lens"
    _open(ctx, worlds, name, source)
    assert ctx.accum_add(N) == N
    bufs = {"normal": torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0"), "albedo": torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0"),
            "depth": torch.zeros((H, W), dtype=torch.float32, device="cuda:0"), "coverage": torch.zeros((H, W), dtype=torch.float32, device="cuda:0")}
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    want = _ref(L, worlds, name, source)
    for stream in (None, side.cuda_stream):
        for b in bufs.values():
            b.zero_()
        torch.cuda.synchronize()
        ctx.accum_guides_device(*(bufs[k].data_ptr() for k in G.KEYS), stream=stream)
        torch.cuda.synchronize()
        G.same({k: bufs[k].cpu().numpy() for k in G.KEYS}, want, f"device form, stream {stream}")
        G.same(ctx.accum_guides(), want, "host form")
    # any output may be NULL
    bufs["depth"].zero_()
    torch.cuda.synchronize()
    ctx.accum_guides_device(None, None, bufs["depth"].data_ptr(), None, stream=side.cuda_stream)
    torch.cuda.synchronize()
    G.same({"depth": bufs["depth"].cpu().numpy()}, want, "depth alone", keys=("depth",))


def test_no_open_accumulation_is_a_state_error(V, worlds):
    c = V.Context(0)
    try:
        tex, dim, cam, _ = worlds["room"]
        c.upload_octree(tex, dim)
        c.set_camera(*cam)
        with pytest.raises(V.VrtError, match="vrt error -5"):
            c.accum_guides()
        with pytest.raises(V.VrtError, match="vrt error -5"):
            c.accum_guides_device(None, None, None, None)
        c.accum_begin(W, H, FIRST)
        with pytest.raises(V.VrtError, match="vrt error -5"):              # begun, no sample yet
            c.accum_guides()
    finally:
        c.close()


@pytest.mark.parametrize("adaptive", [None, (2, 6, 40)])
def test_the_accumulations_own_resolves_do_not_change(ctx, worlds, adaptive):
    """vrt_accum_resolve and _resolve_hdr bytes (and the adaptive counts) with and without interleaved guide calls"""
    name, source = "lamp", "jitter"
    kw = {"adaptive": adaptive} if adaptive else {}

    def run(guides):
        _open(ctx, worlds, name, source, hdr=True, **kw)
        ctx.accum_add(3)
        if guides:
            ctx.accum_guides()
        mid = ctx.accum_resolve() + ctx.accum_resolve_hdr()
        if guides:
            ctx.accum_guides()
        ctx.accum_add(N - 3)
        if guides:
            ctx.accum_guides()
        out = mid + ctx.accum_resolve() + ctx.accum_resolve_hdr()
        return out + ((ctx.accum_counts()[0],) if adaptive else ())

    plain, with_guides = run(False), run(True)
    assert len(plain) == len(with_guides) >= 12
    for a, b in zip(plain, with_guides):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("name", sorted(GW.FRAMES))
def test_coverage_is_where_id_dist_reports_a_hit(ctx, L, worlds, name):
    """corner source, one sample of VRT_MODE_PRIMARY: the frame's voxel ID is set by an opaque first hit (comp:539: surface alpha
    >= 1), so it is non-zero exactly where the guide hit and its albedo alpha is 1; a glass first hit has coverage and ID 0
    (no voxel of these frames sits at linear index 0: tests/test_guides.py)"""
    _open(ctx, worlds, name, "corner", mode=MODE_PRIMARY, first=0)
    assert ctx.accum_add(1) == 1
    g = ctx.accum_guides()
    _, idd, _ = ctx.accum_resolve()
    G.same(g, _ref(L, worlds, name, "corner", 0, 1), f"{name} corner, one sample")
    assert set(np.unique(g["coverage"])) <= {0.0, 1.0}
    opaque = (g["coverage"] > 0) & (g["albedo"][..., 3] >= 1.0)
    assert np.array_equal(opaque, idd[..., 0] != 0)
    assert not (idd[..., 0] != 0)[g["coverage"] == 0].any()
    glass = (g["coverage"] > 0) & (g["albedo"][..., 3] < 1.0)
    assert glass.sum() > 5 and opaque.sum() > 50


# ---- ray batches -----------------------------------------------------------------------------------------------------------------
RAY_KEYS = ("normal", "albedo", "depth", "hit")


@pytest.fixture(scope="module")
def materials(V, O):
    w = _materials_world(V)
    tex, dim = w.flatten()
    w.close()
    cam = V.camera_block((12.5, 10.5, 40.5), -90.0, -10.0, W, H)[:3]
    return tex, dim, O.make_scene(tex, dim, *cam)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,width", [(300, None), (24 * 13, 24)])
def test_ray_batches_are_the_checkers(ctx, L, materials, n, width, variant):
    """a list of 300 and an image of 24 x 13: origins in empty space, in glass, in a solid, on faces and outside the world, directions
    axis-parallel, with zero and tiny components, of lengths 1e-3 .. 1e3 (tests/test_gpu_shade_rays.py _ray_mix)"""
    tex, dim, scene = materials
    ctx.set_variant(variant)
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    o, d = _ray_mix(np.random.default_rng(21 + n), n, (0, 0, 0), (50, 24, 24), ((30, 2, 8), (36, 8, 14)), ((30, 2, 16), (36, 8, 22)))
    want = G.ray_planes(L, scene, o, d)
    assert 30 < want["hit"].sum() < n and (want["albedo"][want["hit"], 3] < 1.0).any()
    G.same(ctx.guide_rays(o, d, width=width), want, f"{n} rays, width {width}, variant {variant}", keys=RAY_KEYS)
    eye = np.array([14.5, 10.5, 11.5], np.float32)                          # one origin for the batch, in the middle of the content
    shared = G.ray_planes(L, scene, eye, d)
    assert shared["hit"].sum() > 30
    G.same(ctx.guide_rays(eye, d, width=width), shared, f"{n} rays, shared origin", keys=RAY_KEYS)


def test_ray_batch_device_form_and_errors(ctx, V, L, materials):
    import torch
    tex, dim, scene = materials
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    o, d = _ray_mix(np.random.default_rng(5), 300, (0, 0, 0), (50, 24, 24), ((30, 2, 8), (36, 8, 14)), ((30, 2, 16), (36, 8, 22)))
    want = G.ray_planes(L, scene, o, d)
    d_o, d_d = torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0")
    d_n = torch.zeros((300, 3), dtype=torch.float32, device="cuda:0")
    d_a = torch.zeros((300, 4), dtype=torch.float32, device="cuda:0")
    d_z = torch.zeros(300, dtype=torch.float32, device="cuda:0")
    d_h = torch.zeros(300, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    ctx.guide_rays_device(300, d_o.data_ptr(), 3, d_d.data_ptr(), d_n.data_ptr(), d_a.data_ptr(), d_z.data_ptr(), d_h.data_ptr(),
                          stream=side.cuda_stream)
    torch.cuda.synchronize()
    got = {"normal": d_n.cpu().numpy(), "albedo": d_a.cpu().numpy(), "depth": d_z.cpu().numpy(), "hit": d_h.cpu().numpy() != 0}
    G.same(got, want, "device form", keys=RAY_KEYS)
    with pytest.raises(V.VrtError, match="vrt error -1"):                   # every output NULL
        ctx.guide_rays_device(300, d_o.data_ptr(), 3, d_d.data_ptr(), None, None, None, None)
    with pytest.raises(V.VrtError, match="vrt error -1"):
        ctx.guide_rays(o, d, width=0)


@pytest.mark.parametrize("name", sorted(GW.FRAMES))
def test_a_frames_corner_rays_give_the_accumulations_guides(ctx, L, worlds, name):
    """vrt_guide_rays on the rays the frame's pixels start from equals vrt_accum_guides at one corner sample"""
    tex, dim, cam, scene = worlds[name]
    L.o_lens_ray.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    L.o_lens_ray.restype = C.c_int
    o, d = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
    for py in range(H):
        for px in range(W):
            L.o_lens_ray(C.addressof(scene), W, H, px, py, 0, 0, 0.0, 1.0, o[py, px].ctypes.data, d[py, px].ctypes.data)
    _open(ctx, worlds, name, "corner", first=0)
    assert ctx.accum_add(1) == 1
    g = ctx.accum_guides()
    r = ctx.guide_rays(o.reshape(-1, 3), d.reshape(-1, 3), width=W)
    for k in ("normal", "albedo", "depth"):
        assert np.array_equal(r[k].reshape(g[k].shape).view(np.uint32), g[k].view(np.uint32)), k
    assert np.array_equal(r["hit"].reshape(H, W), g["coverage"] > 0)


def test_guides_hit_wherever_the_picking_query_hits(ctx, V, L, worlds):
    """vrt_cast_rays (octree_ray_cast) from the lamp room's eye: where it finds a voxel the guide has a hit. Rays it answers at a
    zero-word "ghost" leaf, which the march passes through, would be left out and are counted: this world has none."""
    tex, dim, cam, scene = worlds["lamp"]
    ctx.upload_octree(tex, dim)
    ctx.set_params(ctx.default_params())
    o, d = GW.picking_rays()
    cast = ctx.cast_rays(o, d)[0]
    g = ctx.guide_rays(o, d)
    ghost = int((cast & (G.rays(L, scene, o, d).hit == 0)).sum())
    assert ghost == 0
    assert cast.sum() > 250
    assert g["hit"][cast].all()
