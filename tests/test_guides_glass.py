"""Guides past glass (include/vrt.h vrt_set_guide_glass, G0-G6): the checker (tests/oracle_guides_glass.c) on the CPU. With no
translucent first hit it is oracle_guides.c bit for bit; hand-built worlds pin it to closed forms (tests/glass_worlds.py); on the lamp
and room frames the surface it ends on is the one the oracle's own path tracer names first behind the glass (its mode-2 voxel ID), a
chain the checker does not share; and each of four planted misreadings fails one of these comparisons."""
import numpy as np
import pytest

import glass_worlds as GL
import guide_worlds as GW
import oracle_guides as G
import oracle_guides_glass as GG

MODE_FULL = 2


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return GG.build(tmp_path_factory.mktemp("oracle_guides_glass"))


@pytest.fixture(scope="module")
def frames(V, O):
    """name -> oracle scene: the three guide_worlds frames, and the room through its glass wall (glass_worlds.ROOM_THROUGH_WALL)"""
    out = {}
    for name in GW.FRAMES:
        w = GW.world(V, name)
        tex, dim = w.flatten()
        w.close()
        out[name] = O.make_scene(tex, dim, *GW.camera(V, name))
        if name == "room":
            pose = GL.ROOM_THROUGH_WALL
            out["room_wall"] = O.make_scene(tex, dim, *V.camera_block(pose[:3], pose[3], pose[4], GW.W, GW.H)[:3])
    return out


def _scene(V, O, voxels, highlighted=(-1, -1, -1)):
    tex, dim = GL.build(V, voxels)
    cam = V.camera_block(GL.EYE, 0, 0, 8, 8)[:3]
    return O.make_scene(tex, dim, *cam, highlighted=highlighted)


# ---- off, or nothing translucent: the plain guide ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GW.FRAMES))
def test_where_no_first_hit_is_translucent_the_guide_is_the_plain_one(L, frames, name):
    """sample by sample over the corner, jitter and lens sources: every pixel whose plain guide is a miss or has alpha 255 has the
    same guide past glass, bit for bit, with S = 1 (0 on a miss); through glass the alpha stays the first surface's"""
    scene = frames[name]
    seen_glass = 0
    for source, (jitter, _) in GW.SOURCES.items():
        ap, focus = GW.lens_of(name, source)
        for k in (GW.FIRST, GW.FIRST + GW.N - 1):
            plain = G.sample(L, scene, GW.W, GW.H, k, jitter, ap, focus)
            past = GG.sample(L, scene, GW.W, GW.H, k, jitter, ap, focus)
            direct = (plain.hit == 0) | (plain.albedo[..., 3] == 255)
            for f in ("hit", "normal", "albedo", "depth", "cell"):
                a, b = getattr(plain, f), getattr(past, f)
                assert np.array_equal(a[direct].view(np.uint8), b[direct].view(np.uint8)), (name, source, k, f)
            assert np.array_equal(past.surfaces[direct], plain.hit[direct].astype(np.int32))
            through = ~direct
            assert (past.surfaces[through & (past.hit != 0)] >= 1).all()
            # A = A0: through glass the alpha stays the first surface's
            assert np.array_equal(past.albedo[..., 3][through & (past.hit != 0)], plain.albedo[..., 3][through & (past.hit != 0)])
            seen_glass += int(through.sum())
    assert seen_glass > 50


def test_the_setting_off_is_oracle_guides_on_the_three_frames(L, frames):
    """the library built from oracle_guides_glass.c holds oracle_guides.c unchanged: its planes are those of the library
    tests/oracle_guides.py builds, bit for bit, on the three guide_worlds frames"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        L0 = G.build(tmp)
        for name in GW.FRAMES:
            scene = frames[name]
            for source, (jitter, _) in GW.SOURCES.items():
                want = G.planes(L0, scene, GW.W, GW.H, GW.FIRST, 2, jitter, *GW.lens_of(name, source))[0]
                got = G.planes(L, scene, GW.W, GW.H, GW.FIRST, 2, jitter, *GW.lens_of(name, source))[0]
                G.same(got, want, f"{name} {source}")


# ---- closed forms ------------------------------------------------------------------------------------------------------------------
def _pane_wall(V, O, L, plant=None, highlighted=(-1, -1, -1), back=False):
    o, d = GL.axis_rays(back=back)
    return GG.rays(L, _scene(V, O, GL.pane_wall(back), highlighted), o, d, plant=plant), d


@pytest.mark.parametrize("back", [False, True], ids=["along+x", "along-x"])
def test_perpendicular_through_a_pane_onto_a_wall(V, O, L, back):
    """the wall's normal and RGB, the pane's alpha, three surfaces, and a depth within 1e-3 of the straight distance (11.5 on the axis:
    three pushes and two nudges of 1e-4; off the axis by up to 1.5 degrees the pane bends the path by less than 1e-4); along +x and
    along -x, where a surface's far side is the lower cell"""
    g, d = _pane_wall(V, O, L, back=back)
    assert g.hit.all() and (g.surfaces == 3).all()
    assert (g.normal == np.array([1 if back else -1, 0, 0], np.int8)).all()
    assert (g.albedo[:, :3] == np.array(GL.OPAQUE_BYTES, np.uint8)).all() and (g.albedo[:, 3] == GL.GLASS_ALPHA).all()
    assert (g.cell[:, 0] == (6 if back else 14)).all()
    dn = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1)[:, None]
    assert np.abs(g.depth - 11.5 / np.abs(dn[:, 0])).max() < 1e-3
    plain = G.rays(L, _scene(V, O, GL.pane_wall(back)), *GL.axis_rays(back=back))
    assert (plain.albedo == np.array(GL.GLASS_BYTES, np.uint8)).all() and (plain.cell[:, 0] == 10).all()


def _oblique(V, O, L, plant=None):
    g = GG.rays(L, _scene(V, O, GL.oblique_slab()), np.array(GL.SLAB_EYE, np.float32), np.array([GL.SLAB_DIR], np.float32), plant=plant)
    return g, GL.oblique_slab_closed_form()


def test_oblique_through_a_thick_slab_lands_where_snell_says(V, O, L):
    """45 degrees into four voxels of refraction 1.5: the wall cell is the one the lateral shift t sin(ti - tt) / cos tt predicts, two
    cells from the straight line's, and the depth is the bent path's length, 0.16 longer than the straight distance to that cell"""
    g, (z_bent, z_straight, bent, straight) = _oblique(V, O, L)
    assert int(np.floor(z_bent)) != int(np.floor(z_straight))
    assert min(z_bent % 1.0, 1.0 - z_bent % 1.0) > 0.05              # well inside its cell: 1e-4 pushes do not decide it
    assert g.hit[0] == 1 and g.surfaces[0] == 3
    assert tuple(g.cell[0]) == (GL.SLAB_WALL_X, 10, int(np.floor(z_bent)))
    assert tuple(g.normal[0]) == (-1, 0, 0) and tuple(g.albedo[0]) == GL.OPAQUE_BYTES + (GL.GLASS_ALPHA,)
    # the march pushes the point 1e-4 along an axis at each of the path's 36 cell crossings, and the rule nudges it twice: 38e-4 at the
    # most, and float32 rounding of a length of 25 (1e-5) on top
    assert abs(float(g.depth[0]) - bent) < 38e-4 + 1e-4
    assert bent - straight > 0.1


def test_beyond_the_critical_angle_the_chain_ends_on_glass(V, O, L):
    g = GG.rays(L, _scene(V, O, GL.tir_block()), np.array(GL.TIR_EYE, np.float32), np.array([GL.TIR_DIR], np.float32))
    assert g.hit[0] == 1 and g.surfaces[0] == 1
    assert tuple(g.cell[0]) == (8, 4, 13) and tuple(g.normal[0]) == (-1, 0, 0)
    assert tuple(g.albedo[0]) == GL.GLASS_BYTES
    dn = np.array(GL.TIR_DIR, np.float64) / np.linalg.norm(np.array(GL.TIR_DIR, np.float64))
    assert abs(float(g.depth[0]) - 5.5 / dn[0]) < 1e-3               # 5.5 / cos 60


def test_ten_panes_end_on_the_eighth_surface(V, O, L):
    g = GG.rays(L, _scene(V, O, GL.ten_panes()), *GL.axis_rays())
    assert g.hit.all() and (g.surfaces == 8).all()
    assert (g.cell[:, 0] == GL.PANES_X[3] + 1).all()                 # the far side of the fourth pane
    assert (g.albedo == np.array(GL.GLASS_BYTES, np.uint8)).all()
    assert (g.normal == np.array([-1, 0, 0], np.int8)).all()


def test_pane_then_sky_is_a_miss(V, O, L):
    g = GG.rays(L, _scene(V, O, GL.pane_sky()), *GL.axis_rays())
    assert not g.hit.any() and (g.surfaces == 2).all()
    assert not g.normal.any() and not g.albedo.any() and not g.depth.any()
    assert G.rays(L, _scene(V, O, GL.pane_sky()), *GL.axis_rays()).hit.all()   # the plain guide stops on the pane


def test_a_highlighted_voxel_behind_a_pane_is_inverted(V, O, L):
    g, _ = _pane_wall(V, O, L)
    cell = tuple(int(v) for v in g.cell[0])
    marked, _ = _pane_wall(V, O, L, highlighted=cell)
    want = tuple(255 - b for b in GL.OPAQUE_BYTES) + (GL.GLASS_ALPHA,)
    assert tuple(marked.albedo[0]) == want
    other = (marked.cell != np.array(cell)).any(-1)
    assert np.array_equal(marked.albedo[other], g.albedo[other]) and np.array_equal(marked.depth, g.depth)


# ---- the surface behind the glass is the one the oracle's path tracer names --------------------------------------------------------
@pytest.mark.parametrize("name", ["lamp", "room_wall"])
def test_final_surface_is_the_path_tracers_first_opaque_one(O, L, frames, name):
    """The oracle's mode-2 voxel ID is set by the first depth-0 ray that meets an opaque surface (rt_oracle.c:478), and behind glass
    the refracted ray is the one it marches first (rt_oracle.c:507-516: pushed last, popped first). Where the checker's chain ends on
    an opaque surface within six surfaces -- the path tracer's stack of 12 then never fills on the way -- its cell and face are that
    ID's. Pixels whose ID is 0 are skipped. Through-glass pixels (segment-0 hit translucent) left out of the comparison: at most 25 %,
    and at least 100 compared.
    Counts at 40 x 24, corner sample: lamp 895 through glass, 869 compared, 26 left out (2.9 %); the room through its glass wall
    (glass_worlds.ROOM_THROUGH_WALL) 920 through glass, 787 compared, 133 left out (14.5 %: sky beside the stone block). The
    guide_worlds pose inside the room cannot meet the condition -- of its 512 through-glass pixels 223 end in the sky behind the wall
    and 118 on the jelly cube's glass -- so the frame's pose was moved, not the cap."""
    scene = frames[name]
    idd = O.render(scene, GW.W, GW.H, MODE_FULL)[1]
    vid = idd[..., 0]
    plain = G.sample(L, scene, GW.W, GW.H, 0)
    past = GG.sample(L, scene, GW.W, GW.H, 0)
    through = (plain.hit != 0) & (plain.albedo[..., 3] < 255)
    ends_opaque = (past.hit != 0) & (past.surfaces <= 6)
    # the chain ended on an opaque surface: the surface's own alpha, which A0 hides, is 255 exactly when the chain did not stop for G4 / G5
    final = GG.sample(L, scene, GW.W, GW.H, 0, plant="alpha_of_final")
    ends_opaque &= final.albedo[..., 3] == 255
    keep = through & ends_opaque & (vid != 0)
    left_out = int(through.sum()) - int(keep.sum())
    print(f"{name}: {int(through.sum())} through glass, {int(keep.sum())} compared, {left_out} left out")
    assert keep.sum() >= 100
    assert left_out <= 0.25 * through.sum()
    assert np.array_equal(past.vid[keep], vid[keep])
    # ... and directly seen opaque pixels name their own surface, as the plain guide does
    direct = (plain.hit != 0) & (plain.albedo[..., 3] == 255) & (vid != 0)
    assert np.array_equal(past.vid[direct], vid[direct])
    # the comparison has teeth: the plain guide's cell behind glass is the pane's, not the ID's
    lin = plain.cell[..., 0] + scene.tex_dim * (plain.cell[..., 1] + scene.tex_dim * plain.cell[..., 2])
    assert (lin[keep] != vid[keep] // 6).all()


# ---- planted misreadings -----------------------------------------------------------------------------------------------------------
def test_planted_inverted_ratio_is_caught(V, O, L):
    g, (z_bent, _, _, _) = _oblique(V, O, L, plant="ratio_inverted")
    assert not (g.hit[0] == 1 and tuple(g.cell[0]) == (GL.SLAB_WALL_X, 10, int(np.floor(z_bent))))


def test_planted_straight_depth_is_caught(V, O, L):
    g, (_, _, bent, _) = _oblique(V, O, L, plant="depth_straight")
    assert abs(float(g.depth[0]) - bent) > 0.1


def test_planted_alpha_of_the_final_surface_is_caught(V, O, L):
    g, _ = _pane_wall(V, O, L, plant="alpha_of_final")
    assert (g.albedo[:, 3] == 255).all()                             # the wall's: the check above wants the pane's 0x80


def test_planted_outward_nudge_is_caught(V, O, L):
    """along -x the point nudged back out of the air lands in the glass cell it left, in medium 1.0: the same face is met again and
    again, and the chain ends on glass at the eighth surface"""
    g, _ = _pane_wall(V, O, L, plant="nudge_outwards", back=True)
    assert not (g.albedo[:, :3] == np.array(GL.OPAQUE_BYTES, np.uint8)).all(-1).any()   # never reaches the wall
