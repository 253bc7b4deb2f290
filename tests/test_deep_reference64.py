"""The checker of the path depth, the sun disc and the emitter rules (tests/oracle_paths.c, through each of its five wrappers:
oracle_path_depth, oracle_sun, oracle_emit, oracle_emit_power, oracle_emit_mis) against the independent float64 restatement
(tests/path_ref64.py with depth=, tan_radius=, emit= and mis=, written from the text of include/vrt.h alone).

Per batch and setting (D, tan_radius, rule) every decided ray must agree exactly in bytes, voxel ID and dist, and the checker's
unclamped float colour must lie within the reference's float32 bound. The reference's per-ray stats prove that a batch exercises the
branch its setting is about; each batch and setting states its measured undecided share beside its cap; the bound of a ray with an
emitter connection must stay far below what any misreading moves; and one planted misreading at a time shows that the comparison
fails when it should. tests/test_gpu_deep_reference64.py holds the device to the same traces."""
import numpy as np
import pytest

import deep_ref64 as DR
import emit_worlds as ew
import oracle_emit as oe
import oracle_emit_mis as om
import oracle_emit_power as oep
import oracle_path_depth as opd
import oracle_rays
import oracle_sun as osun
import path_ref64 as PR
import shader_ref64 as R
import sun_worlds as sw
from test_emit_power import _host_cdf
from test_emitters import _host_list
from test_path_reference64 import SAMPLES
from test_gpu_shade_rays import _ray_mix
from test_rays_reference64 import DRAGON_MIX, MATERIALS_MIX, MIN_DECIDED, MIN_DECIDED_HITS, N_MIX, Batch, RR, check_floats, scenes  # noqa: F401
from test_rays_reference64 import batch as rays_batch
from test_shader_reference64 import _slab

F = np.float32
OFF, UNIFORM, POWER, MIS = "off", "uniform", "power", "mis"
SETTINGS = ((2, 0.0, OFF), (3, 0.0, OFF), (8, 0.0, OFF), (1, 0.05, OFF), (3, 0.05, OFF), (1, 0.0, UNIFORM), (3, 0.05, UNIFORM),
            (1, 0.0, POWER), (3, 0.05, POWER), (1, 0.0, MIS), (3, 0.05, MIS), (8, 0.05, MIS))
OPEN_BATCHES = ("dragon_mix", "materials_1", "slab")
EMITTER_BATCHES = ("lamp_room", "open_emitters")
MIN_BRANCH = 200
MIX_SEED = {"dragon_mix": 51, "materials_1": 53}    # test_rays_reference64's
CEILING = {1: 0.15, 2: 0.15, 3: 0.15, 8: 0.30}
# A bound can hide a wrong sample as an undecided ray can: of the decided rays with a contributing connection, nine in ten must have
# bound / (|value| + 1e-3) below 1e-3 (every planted misreading moves a contribution by far more). Measured: medians of 3.5e-5 to
# 2.1e-4, shares of 96 to 100 %, and 93 % on the lamp room at D = 8. What dominates where the ratio is large: the chain's deviation
# across its rays (path_ref64's xerr) over the connection's length, which grows with every change of the hit axis along a chain;
# 1 / cl at connections grazing an emitter's face comes second (it was first, and far over 1e-3, while the deviation was carried as
# one number per ray and amplified at every vertex: the per-axis form brought the lamp room at D = 3 from 60 % to 98 %).
BOUND_RATIO, BOUND_SHARE = 1e-3, 0.90
# two samples per batch, all five indices across the file
BATCH_SAMPLES = {name: (SAMPLES[k % 5], SAMPLES[(k + 2) % 5]) for k, name in enumerate(OPEN_BATCHES + EMITTER_BATCHES)}


def sid(setting):
    return f"D{setting[0]}-r{setting[1]:g}-{setting[2]}"


def ref_args(setting):
    D, rad, rule = setting
    return dict(depth=D, tan_radius=rad, emit=None if rule == OFF else (UNIFORM if rule == UNIFORM else POWER), mis=rule == MIS)


CASES = [(b, s) for b in OPEN_BATCHES for s in SETTINGS if s[2] == OFF] + [(b, s) for b in EMITTER_BATCHES for s in SETTINGS if s[2] != OFF]
CASE_IDS = [f"{b}-{sid(s)}" for b, s in CASES]

# Undecided share of the in-world rays (any field of the ray undecided), measured on the reference alone (the worse of the batch's
# two samples); the cap is that share plus a quarter of itself, rounded up to the next 0.005, and never above CEILING[D].
# (batch, setting): cap                                          measured
CAPS = {
    ("dragon_mix", (2, 0.0, "off")): 0.015,         # 1.06 %
    ("dragon_mix", (3, 0.0, "off")): 0.015,         # 1.06 %
    ("dragon_mix", (8, 0.0, "off")): 0.015,         # 1.11 %
    ("dragon_mix", (1, 0.05, "off")): 0.015,        # 1.00 %
    ("dragon_mix", (3, 0.05, "off")): 0.020,        # 1.20 %
    ("materials_1", (2, 0.0, "off")): 0.045,        # 3.30 %
    ("materials_1", (3, 0.0, "off")): 0.045,        # 3.26 %
    ("materials_1", (8, 0.0, "off")): 0.045,        # 3.30 %
    ("materials_1", (1, 0.05, "off")): 0.045,       # 3.29 %
    ("materials_1", (3, 0.05, "off")): 0.045,       # 3.48 %
    ("slab", (2, 0.0, "off")): 0.005,               # 0.26 %
    ("slab", (3, 0.0, "off")): 0.005,               # 0.26 %
    ("slab", (8, 0.0, "off")): 0.010,               # 0.41 %
    ("slab", (1, 0.05, "off")): 0.010,              # 0.51 %
    ("slab", (3, 0.05, "off")): 0.005,              # 0.38 %
    ("lamp_room", (1, 0.0, "uniform")): 0.035,      # 2.61 %
    ("lamp_room", (3, 0.05, "uniform")): 0.065,     # 5.20 %
    ("lamp_room", (1, 0.0, "power")): 0.040,        # 3.19 %
    ("lamp_room", (3, 0.05, "power")): 0.085,       # 6.76 %
    ("lamp_room", (1, 0.0, "mis")): 0.045,          # 3.57 %
    ("lamp_room", (3, 0.05, "mis")): 0.090,         # 7.14 %
    ("lamp_room", (8, 0.05, "mis")): 0.290,         # 22.98 %
    ("open_emitters", (1, 0.0, "uniform")): 0.005,  # 0.37 %
    ("open_emitters", (3, 0.05, "uniform")): 0.015, # 1.09 %
    ("open_emitters", (1, 0.0, "power")): 0.005,    # 0.37 %
    ("open_emitters", (3, 0.05, "power")): 0.020,   # 1.36 %
    ("open_emitters", (1, 0.0, "mis")): 0.010,      # 0.66 %
    ("open_emitters", (3, 0.05, "mis")): 0.025,     # 1.69 %
    ("open_emitters", (8, 0.05, "mis")): 0.055,     # 4.36 %
}


class DeepBatch(Batch):
    """a Batch with the emitter list of its world (by a walk of the host's records) and the reference's traces per setting"""

    def __init__(self, *a, records=None, **kw):
        super().__init__(*a, **kw)
        self.records = records
        self.lst = self.words = self.wt = None
        if records is not None:
            self.lst, self.words = oep.walk(records, self.wmin, self.wmax)
            self.wt = np.array(oep.weights(self.lst, self.words), np.uint64)
        self._deep = {}

    def deep(self, setting, sample, flaws=()):
        key = (setting, sample & 0xFFFFFFFF)
        if flaws or key not in self._deep:
            t = PR.PathTrace.rays(self.world, self.o, self.d, self.width, sample=sample, voxel_scale=self.scale, global_light=self.gl,
                                  light_dir=self.light, flaws=flaws, **ref_args(setting))
            if flaws:
                return t
            self._deep[key] = t
        return self._deep[key]

    def deep_at(self, setting, sample, o, d, width):
        """the reference's trace of other rays in the batch's world (a batch shape), not kept"""
        return PR.PathTrace.rays(self.world, o, d, width, sample=sample, voxel_scale=self.scale, global_light=self.gl,
                                 light_dir=self.light, **ref_args(setting))

    def prefix(self, n):
        """the batch's first n rays as a batch of their own: ray i keeps its RNG pixel, so its trace is the same"""
        b = DeepBatch(self.tex, self.dim, self.o[:n], self.d[:n], self.width, scale=self.scale, wmin=self.wmin, wmax=self.wmax,
                      gl=self.gl, cam=self.cam, records=self.records)
        b.light, b._world, b.make_world = self.light, self.world, self.make_world
        return b

    def mean(self, setting, first, n):
        rad = [self.deep(setting, first + k).radiance() for k in range(n)]
        return R.hdr_mean([r[0] for r in rad], [r[1] for r in rad], [r[2] for r in rad])


@pytest.fixture(scope="module")
def CK(tmp_path_factory):
    """the checker, under the name of each of its five wrappers"""
    L = om.build(tmp_path_factory.mktemp("oracle_deep_ref64"))
    return dict.fromkeys(("depth", "sun", "emit", "power", "mis"), L)


def checker_shade(CK, b, s, setting, k, o=None, d=None):
    """the checker through the wrapper of the setting's last rule -> (rgba8, id_dist, rgb float32)"""
    D, rad, rule = setting
    o, d = (b.o if o is None else o), (b.d if d is None else d)
    if rule == OFF and rad == 0.0:
        return opd.shade(CK["depth"], s, o, d, D, b.width, k)
    if rule == OFF:
        return osun.shade(CK["sun"], s, o, d, D, rad, b.width, k)
    if rule == UNIFORM:
        return oe.shade(CK["emit"], s, o, d, D, rad, b.lst, b.width, k)
    if rule == POWER:
        return oep.shade(CK["power"], s, o, d, D, rad, b.lst, b.wt, oep.POWER, b.width, k)
    return om.shade(CK["mis"], s, o, d, D, rad, b.lst, b.wt, om.POWER, 1, b.width, k)


# ---- the batches -----------------------------------------------------------------------------------------------------------------
def _from_world(w, o, d, width, light=None, **kw):
    tex, dim = w.flatten()
    rec = np.array(w.records()[0], np.uint32).copy()
    w.close()
    b = DeepBatch(tex, dim, o, d, width, records=rec, **kw)
    if light is not None:
        b.light = np.asarray(light, F)
    return b


N_SLAB_DEEP = 7000


def slab_batch(V, light=sw.SLAB_LIGHT, n_deep=N_SLAB_DEEP):
    """1,500 rays from random origins between the floor and the slab towards the floor strip under the slab's edge, where the disc's
    penumbra (0.05 * SLAB_H = 0.4 voxels either side of the edge) lies; then n_deep rays from the air deep under the slab towards
    the floor under its middle: the world is open to the sky on three sides, about one chain in twenty-five of these lives to its
    eighth vertex (one in thirty of the strip's), and depth 8 needs 200 of them"""
    rng = np.random.default_rng(61)
    n = 1500
    target = np.stack([sw.SLAB_X0 + rng.uniform(-0.6, 0.6, n), np.full(n, float(sw.SLAB_FLOOR_TOP)), sw.SLAB_Z + rng.uniform(-6, 6, n)], 1)
    o = np.stack([sw.SLAB_X0 + rng.uniform(-5, 5, n), sw.SLAB_FLOOR_TOP + rng.uniform(2.0, 6.0, n), sw.SLAB_Z + rng.uniform(-6, 6, n)], 1)
    if n_deep:
        xm = sw.SLAB_X0 - 10.0
        t2 = np.stack([xm + rng.uniform(-3, 3, n_deep), np.full(n_deep, float(sw.SLAB_FLOOR_TOP)), sw.SLAB_Z + rng.uniform(-3, 3, n_deep)], 1)
        o2 = np.stack([xm + rng.uniform(-3, 3, n_deep), sw.SLAB_FLOOR_TOP + rng.uniform(2.0, 6.0, n_deep), sw.SLAB_Z + rng.uniform(-3, 3, n_deep)], 1)
        target, o = np.concatenate([target, t2]), np.concatenate([o, o2])
    b = _from_world(sw.slab_world(V), o, target - o, 64, light=light)
    b.make_world = lambda: sw.slab_world(V)
    return b


N_NEAR = 2000


def lamp_room_batch(V, O, RR):
    """2,000 rays from random points of the room's air towards random points of its shell, 2,000 towards the ceiling around the
    single emitters, then the 72 x 44 frame at POSE thinned to every other pixel"""
    rng = np.random.default_rng(62)
    n = 2000
    o = ew.LO + 1.2 + rng.random((3 * n, 3)) * (ew.HI - ew.LO - 1.4)
    c = np.floor(o).astype(int)
    (lx, ly, lz), _ = ew.LAMP
    solid = (c[:, 1] == ew.TABLE_Y) & (c[:, 0] >= ew.TABLE[0]) & (c[:, 0] < ew.TABLE[1]) & (c[:, 2] >= ew.TABLE[0]) & (c[:, 2] < ew.TABLE[1])
    solid |= np.all((c >= (lx, ly, lz)) & (c < (lx + 2, ly + 2, lz + 2)), 1)
    solid |= (c[:, 0] == ew.PANE_X) & (c[:, 1] >= ew.PANE_Y[0]) & (c[:, 1] < ew.PANE_Y[1]) & (c[:, 2] >= ew.PANE_Z[0]) & (c[:, 2] < ew.PANE_Z[1])
    solid |= c[:, 1] >= ew.HI - 1                                  # the layer of the single emitters
    o = o[~solid][:n]
    assert len(o) == n
    t = ew.LO + rng.random((n, 3)) * (ew.HI + 1 - ew.LO)
    face = rng.integers(0, 6, n)
    t[np.arange(n), face >> 1] = np.where(face & 1, ew.HI + 0.5, ew.LO + 0.5)
    # 2,000 more towards the ceiling around a single emitter: a bounce from there finds the emitter often enough for the floor of
    # MIS-weighted bounce hits at D = 1
    o = np.concatenate([o, o[:N_NEAR]])
    s_ = np.array([p for p, _ in ew.SINGLES], np.float64)[rng.integers(0, len(ew.SINGLES), N_NEAR)]
    t = np.concatenate([t, np.stack([s_[:, 0] + 0.5 + rng.uniform(-1.4, 1.4, N_NEAR), np.full(N_NEAR, ew.HI + 0.5),
                                     s_[:, 2] + 0.5 + rng.uniform(-1.4, 1.4, N_NEAR)], 1)])
    w = ew.lamp_room(V)
    tex, dim = w.flatten()
    cam = V.camera_block(ew.POSE[:3], ew.POSE[3], ew.POSE[4], ew.W, ew.H)[:3]
    fo, fd = oracle_rays.frame_rays(RR, O.make_scene(tex, dim, *cam), ew.W, ew.H)
    fo = np.broadcast_to(np.asarray(fo, F).reshape(-1, 3), fd.shape)
    # every other pixel of the frame in both directions: a ray through the pane carries a glass tree, every branch of it a chain,
    # and at D = 8 nearly half of these pixels hold a grazing step somewhere (0.48 undecided against 0.11 to 0.16 of the other rays)
    ys, xs = np.mgrid[0:ew.H:2, 0:ew.W:2]
    fo, fd = fo[(ys * ew.W + xs).ravel()], fd[(ys * ew.W + xs).ravel()]
    b = _from_world(w, np.concatenate([o.astype(F), fo]), np.concatenate([(t - o).astype(F), fd]), ew.W, cam=cam)
    b.n_mix = n + N_NEAR
    b.make_world = lambda: ew.lamp_room(V)
    return b


# the open emitter world's entries, lo and size: the white block [8, 16) x [4, 12) x [8, 16) is eight leaves of size 4
BIG = tuple((x, y, z, 4) for x in (8, 12) for y in (4, 8) for z in (8, 12))
SMALL, BLACK = (18, 2, 4, 2), (4, 1, 18, 1)


def open_emitter_world(V):
    """test_rays_reference64.emitter_world (a floor and a white emitter, eight leaves of size 4) with a second, dimmer emitter of size 2 and a
    black one (alpha > 0, illumination > 0, colour 0): the power rule differs from the uniform one, the black entry holds the table's
    one-tick floor, and the sun and the emitters light the same floor"""
    vox = _slab(0, 24, 0, 1, 0, 24) + _slab(8, 16, 4, 12, 8, 16, c=0xFFFFFFFF, r=3.0, i=1.0)
    vox += _slab(18, 20, 2, 4, 4, 6, c=0xc08040FF, r=3.0, i=0.5) + _slab(4, 5, 1, 2, 18, 19, c=0x000000FF, r=3.0, i=1.0)
    # four grey walls and a canopy over two thirds of them keep chains of bounces alive to depth 8; the sun enters over z >= 19
    vox += _slab(0, 1, 1, 14, 0, 24) + _slab(23, 24, 1, 14, 0, 24) + _slab(1, 23, 1, 14, 0, 1) + _slab(1, 23, 1, 14, 23, 24)
    vox += _slab(0, 24, 14, 15, 0, 19)
    w = V.World()
    for x, y, z, c, r, i in vox:
        w.insert(int(x), int(y), int(z), int(c), float(r), float(i), 0.0)
    return w


def open_emitter_batch(V):
    rng = np.random.default_rng(63)
    n = 3200
    o = np.array([1.5, 1.5, 16.5]) + rng.random((n, 3)) * np.array([21.0, 12.0, 6.0])         # in the air under the open strip
    t = np.stack([rng.uniform(0.5, 23.5, n), np.full(n, 1.0), rng.uniform(0.5, 23.5, n)], 1)
    box = rng.random(n) < 0.25
    t[box] = np.array([8.0, 4.0, 8.0]) + rng.random((int(box.sum()), 3)) * 8.0
    d = (t - o) * 10.0 ** rng.uniform(-3.0, 3.0, size=(n, 1))
    b = _from_world(open_emitter_world(V), o, d, 64)
    # the sun enters over the canopy's edge: rays into its penumbra on the floor and the walls, which the emitters light as well
    po, pd = penumbra_rays(b, rng, 20)
    b = _from_world(open_emitter_world(V), np.concatenate([b.o, po]), np.concatenate([b.d, pd]), 64)
    b.make_world = lambda: open_emitter_world(V)
    return b


# Rays into the disc's penumbrae of an open world, found on the reference alone. A random ray of a mix meets a penumbra of 0.05 at
# under 1 % of its vertices. The mix is traced at (1, 0.05, off) at three sample indices that no comparison uses; a ray whose lit
# differed from the point sun's in one of them ends in a penumbra, whatever the sample (a first hit takes no draw). Each such ray
# seeds n_around more from its origin towards points within about PENUMBRA_STEP voxels of its hit: a penumbra runs along its edge.
SEED_SAMPLES = (101, 102, 103)
N_AROUND, PENUMBRA_STEP = 72, 0.15


def penumbra_rays(b, rng, n_around=N_AROUND):
    seed = np.zeros(len(b.o), bool)
    for k in SEED_SAMPLES:
        t = b.deep((1, 0.05, OFF), k)
        f = t.frame()
        seed |= f.all_decided() & f.hit & (t.stats["sun_differs"] > 0)
    b._deep.clear()
    i = np.repeat(np.nonzero(seed)[0], n_around)
    d = b.d[i].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = np.maximum(f.dist[i].astype(np.float64), 1.0)
    d += rng.normal(0.0, PENUMBRA_STEP, d.shape) / dist[:, None]
    return b.o[i], d.astype(F)


_batches = {}


def batch(name, V, O, RR, scenes):
    if name not in _batches:
        if name in ("dragon_mix", "materials_1"):
            # the batch of test_rays_reference64 at twice its size (a chain under an open sky rarely lives to depth 8), then the
            # rays into its penumbrae
            src = rays_batch(name, V, O, RR, scenes)
            o, d = _ray_mix(np.random.default_rng(MIX_SEED[name]), 2 * N_MIX[name], *(DRAGON_MIX if name == "dragon_mix" else MATERIALS_MIX))
            b = DeepBatch(src.tex, src.dim, o, d, src.width, scale=src.scale, gl=src.gl)
            b._world, b.make_world = src.world, src.make_world
            po, pd = penumbra_rays(b, np.random.default_rng(MIX_SEED[name] + 100))
            b = DeepBatch(src.tex, src.dim, np.concatenate([b.o, po]), np.concatenate([b.d, pd]), src.width, scale=src.scale, gl=src.gl)
            b._world, b.make_world = src.world, src.make_world
        elif name == "slab":
            b = slab_batch(V)
        elif name == "lamp_room":
            b = lamp_room_batch(V, O, RR)
        else:
            assert name == "open_emitters", name
            b = open_emitter_batch(V)
        _batches[name] = b
    return _batches[name]


DISC, TERMINAL, CONNECTION, MIS_BOUNCE = ("lit differs from the point sun's", "a terminal vertex at depth D", "a contributing connection",
                                          "an MIS-weighted bounce hit")


def branch_rays(t, setting, dec, name):
    """branch -> the decided rays of batch `name` that reached a branch the setting is about. The disc's branch is asked of every
    batch with a radius but the lamp room: it is closed to the sun, so no vertex in it is lit by either sun"""
    D, rad, rule = setting
    st = t.stats
    out = {}
    if D > 1:
        out[TERMINAL] = dec & (st["terminal"] > 0)
    if rad > 0 and name != "lamp_room":
        out[DISC] = dec & (st["sun_differs"] > 0)
    if rule != OFF:
        out[CONNECTION] = dec & (st["conn_contributing"] > 0)
    if rule == MIS:
        out[MIS_BOUNCE] = dec & (st["mis_bounce_hits"] > 0)
    return out


def undecided_share(f):
    return f.in_world_undecided_share()


# ---- decided rays are exact, floats within the bound --------------------------------------------------------------------------
@pytest.mark.parametrize("name,setting", CASES, ids=CASE_IDS)
def test_checkers_match_the_reference(V, O, RR, CK, scenes, name, setting):
    b = batch(name, V, O, RR, scenes)
    s = b.scene(O, V)
    seen = set()
    for k in BATCH_SAMPLES[name]:
        what = f"{name} {sid(setting)} sample {k}"
        rgba, idd, rgb = checker_shade(CK, b, s, setting, k)
        t = b.deep(setting, k)
        f = t.frame()
        r = R.compare(f, rgba, idd)
        dec = f.all_decided()
        share = undecided_share(f)
        print(f"{what}: in-world {int((~f.outside).sum())} decided {int(dec.sum())} decided hits {int((dec & f.hit).sum())} "
              f"undecided share {share:.4f}")
        assert r["bad"] == 0, (what, r)
        assert dec.sum() >= MIN_DECIDED and (dec & f.hit).sum() >= MIN_DECIDED_HITS, (what, int(dec.sum()), int((dec & f.hit).sum()))
        for branch, rays in branch_rays(t, setting, dec, name).items():
            print(f"{what}: {branch}: {int(rays.sum())}")
            assert rays.sum() >= MIN_BRANCH, (what, branch, int(rays.sum()))
        cap = CAPS[(name, setting)]
        assert cap <= CEILING[setting[0]] and share <= cap, (what, share, cap)
        want, bound, decf = t.radiance()
        check_floats(rgb, want, bound, decf, what)
        if setting[2] != OFF:
            conn = decf & (t.stats["conn_contributing"] > 0)
            ratio = (bound[conn] / (np.abs(want[conn]) + 1e-3)).max(1)
            print(f"{what}: bound / (|value| + 1e-3) over {int(conn.sum())} rays with a connection: median {np.median(ratio):.2e} "
                  f"share below {BOUND_RATIO:g}: {(ratio < BOUND_RATIO).mean():.4f}")
            assert (ratio < BOUND_RATIO).mean() >= BOUND_SHARE, (what, float((ratio < BOUND_RATIO).mean()))
        seen.add(rgba.tobytes())
    assert len(seen) == 2


# ---- the defaults move no bit ----------------------------------------------------------------------------------------------------
def test_default_arguments_change_no_bit(V, O, RR, scenes):
    """depth=1, tan_radius=0, emit=None, mis=False passed explicitly, and sampling or MIS switched on where nothing reads them, give
    the trace of a call without them, bit for bit. Both sides are this module as it stands: that no bit moved against the module
    as it was is held by the earlier tests of the three reference modules, which are unchanged and compare it with the checkers."""
    b = rays_batch("materials_1", V, O, RR, scenes)
    k = SAMPLES[1]
    old = b.trace(2, k)
    new = PR.PathTrace.rays(b.world, b.o, b.d, b.width, sample=k, voxel_scale=b.scale, global_light=b.gl, light_dir=b.light, depth=1,
                            tan_radius=0.0, emit=None, mis=False)
    f, g = old.frame(), new.frame()
    for a in ("rgba", "id", "dist", "dec_id", "dec_dist", "dec_rgb", "hit", "outside"):
        assert np.array_equal(getattr(f, a), getattr(g, a)), a
    for x, y in zip(old.radiance(), new.radiance()):
        assert x.tobytes() == y.tobytes()
    # sampling on over a world without emitters, and MIS without the power rule, are read nowhere
    d = rays_batch("dragon_mix", V, O, RR, scenes)
    old = d.trace(2, k)
    for kw in (dict(emit=POWER, mis=True), dict(emit=UNIFORM, mis=True)):
        new = PR.PathTrace.rays(d.world, d.o, d.d, d.width, sample=k, voxel_scale=d.scale, global_light=d.gl, light_dir=d.light, **kw)
        for x, y in zip(old.radiance(), new.radiance()):
            assert x.tobytes() == y.tobytes()


# ---- the emitter list and the thresholds ---------------------------------------------------------------------------------------
def _odd_bounds_stream():
    """a hand-written stream under the bounds [0, 4) x [0, 2) x [0, 2), no power of two: the root's child 0 is a leaf whose box
    [0, 2) x [0, 1) x [0, 1) is no cube (an emitter: listed as its two unit cells), child 7 a grey leaf, child 4 an internal node
    whose one live child [2, 3) x [0, 1) x [0, 1) is a second emitter -> (texels, tex_dim, world_min, world_max)"""
    tx = sw._tx
    leaf = 0x800000
    stream = tx(1, 0x91) + tx(4 | leaf, 0) + tx(8, 0) + tx(6 | leaf, 0) + [255, 224, 160, 255, 255, 200, 0, 255] \
        + [160, 160, 160, 255, 255, 0, 0, 255] + tx(9, 0x08) + tx(10 | leaf, 0) + [16, 32, 48, 255, 255, 64, 0, 255]
    return np.array(stream, np.uint8), 3, (0, 0, 0), (4, 2, 2)


def _black_world(V):
    w = V.World()
    for x, y, z, c, r, i in _slab(0, 8, 0, 1, 0, 8) + _slab(2, 4, 2, 4, 2, 4, c=0x000000ff, i=1.0) + _slab(6, 7, 3, 4, 1, 2, c=0x000000ff, i=0.5) \
            + _slab(1, 2, 5, 6, 6, 7, c=0x000000ff, i=1.0):
        w.insert(x, y, z, c, float(r), float(i), 0.0)
    return w, (-1023,) * 3, (1024,) * 3


@pytest.mark.parametrize("name", ["lamp_room", "open_emitters", "odd_bounds", "all_black"])
def test_emitter_list_and_thresholds_are_the_hosts(V, name):
    if name == "lamp_room":
        w, wmin, wmax = ew.lamp_room(V), (-1023,) * 3, (1024,) * 3
    elif name == "open_emitters":
        w, wmin, wmax = open_emitter_world(V), (-1023,) * 3, (1024,) * 3
    elif name == "all_black":
        w, wmin, wmax = _black_world(V)
    if name == "odd_bounds":
        tex, dim, wmin, wmax = _odd_bounds_stream()
        rec = V.build_layout(tex)[0]
    else:
        tex, dim = w.flatten()
        rec = np.array(w.records()[0], np.uint32).copy()
        w.close()
    E = DR.Emitters(R.World(tex, dim, wmin, wmax))
    n, lst = _host_list(V, rec, wmin, wmax)
    wt, cdf = _host_cdf(V, rec, wmin, wmax)
    assert n == E.N > 0 and np.array_equal(lst, E.entries()), (name, n, E.N)
    assert [int(x) for x in wt] == E.W and [int(x) for x in cdf] == E.T, name
    assert E.T[-1] == 1 << 24 and all(b > a for a, b in zip([0] + E.T, E.T))
    if name == "lamp_room":
        assert sorted(E.size.tolist()) == [1, 1, 1, 2]
    if name == "open_emitters":
        assert E.entries().tolist() == sorted([list(e) for e in BIG + (SMALL, BLACK)]) and min(E.W) == 0 < E.total
        j = E.W.index(0)
        assert E.T[j] - (E.T[j - 1] if j else 0) == 1, "the black entry holds exactly the one-tick floor"
    if name == "odd_bounds":
        assert E.entries().tolist() == [[0, 0, 0, 1], [1, 0, 0, 1], [2, 0, 0, 1]] and E.node[0] == E.node[1] != E.node[2], \
            "a merged leaf that is no cube, listed as its unit cells"
        assert E.W == [200 * (255 + 224 + 160)] * 2 + [64 * (16 + 32 + 48)]
    if name == "all_black":
        assert E.total == 0 and E.inv_power == 0.0 and E.T == [(j + 1) * (1 << 24) // E.N for j in range(E.N)]


# ---- the comparison can fail: one planted misreading at a time ------------------------------------------------------------------
# flaw: (batch, setting)
MUTATIONS = {
    "inner_ambient": ("dragon_mix", (3, 0.0, OFF)), "inner_keeps_dim": ("dragon_mix", (3, 0.0, OFF)),
    "depth_off_by_one": ("dragon_mix", (3, 0.0, OFF)), "sun_draws_after_bounce": ("dragon_mix", (3, 0.05, OFF)),
    "sun_unit_length": ("slab_long_light", (1, 0.05, OFF)), "sun_glass_ndotl": ("materials_1", (1, 0.05, OFF)),
    "emit_origin_2e3": ("lamp_room", (1, 0.0, UNIFORM)), "emit_draw_order": ("lamp_room", (1, 0.0, UNIFORM)),
    "emit_keeps_bounce_emission": ("lamp_room", (3, 0.05, UNIFORM)), "emit_any_emitter": ("lamp_room", (1, 0.0, UNIFORM)),
    "power_six_faces": ("lamp_room", (1, 0.0, POWER)), "power_no_p": ("lamp_room", (1, 0.0, POWER)),
    "mis_m_of_cube": ("lamp_room", (1, 0.0, MIS)), "mis_wb_cosine_at_hit": ("lamp_room", (3, 0.05, MIS)),
}
MIN_CAUGHT = 20


@pytest.mark.parametrize("flaw", PR.DEEP_FLAWS)
def test_each_planted_deep_flaw_is_detected(V, O, RR, CK, scenes, flaw):
    """on a named batch and setting the flawed reference disagrees with the checker on at least 20 decided rays (bytes, ID, dist or
    a float beyond its bound); the unflawed one on none"""
    assert set(MUTATIONS) == set(PR.DEEP_FLAWS)
    name, setting = MUTATIONS[flaw]
    if name == "slab_long_light":
        if name not in _batches:
            _batches[name] = slab_batch(V, light=(0.0, 1.5, 0.0), n_deep=0)      # vrt_params allows a lightDir of any length
        b = _batches[name]
        k = SAMPLES[0]
    else:
        b = batch(name, V, O, RR, scenes)
        k = BATCH_SAMPLES[name][0]
    rgba, idd, rgb = checker_shade(CK, b, b.scene(O, V), setting, k)

    def disagreements(t):
        f = t.frame()
        want, bound, dec = t.radiance()
        wrong = dec & (np.abs(R.hdr_value(rgb.astype(np.float64)) - want) > bound).any(1)
        return max(R.compare(f, rgba, idd)["bad"], int(wrong.sum()))

    assert disagreements(b.deep(setting, k)) == 0, flaw
    caught = disagreements(b.deep(setting, k, flaws=(flaw,)))
    print(f"{flaw}: {caught} decided rays disagree on {name} {sid(setting)}")
    assert caught >= MIN_CAUGHT, (flaw, caught)
