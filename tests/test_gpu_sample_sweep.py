"""Seeded random worlds against every sample route on the MI355X: the 36 cases of sample_sweep_worlds.py -- six families of six
worlds, each at the setting its schedule assigns (path depth, sun radius, emitter rule, ray source, variant) -- bit for bit against
the checkers. Per case: the accumulation in VRT_MODE_FULL from the scheduled source, plain (3 + 5 against 8 in one add), adaptive with
its counts, HDR with both tone maps (test_gpu_emitters._forms) and HDR with moments; the id_dist of every resolve; the two primary
modes from the same source; the guide planes of the plain accumulation, plain and past glass; and the world's batch of 257 arbitrary
rays through shade_rays in all three modes, shade_rays_hdr with caller sums and guide_rays with glass off and on, in the host forms
and, where index % 3 == 0, the device forms on a caller's stream. run_case() is shared with fuzz/fuzz_samples.py, which replays a
case from the name every failure message carries: `fuzz_samples.py --case FAMILY INDEX`."""
import numpy as np
import pytest

import oracle_emit as oe
import oracle_emit_mis as om
import oracle_guides as G
import oracle_guides_glass as GG
import oracle_hdr
import oracle_lens
import oracle_moments as OM
import oracle_rays
import oracle_sun as osun
import sample_sweep_worlds as sw
import test_gpu_emit_mis as tem
import test_gpu_emitters as tge

pytestmark = pytest.mark.gpu
F = np.float32
ON = {"off": tem.OFF, "uniform": tem.UNIFORM, "power": tem.POWER, "power+mis": tem.MIS}   # a rule as test_gpu_emit_mis.Refs' `on`
RAY_KEYS = ("normal", "albedo", "depth", "hit")
SHARED_WIDTH = 13                      # the shared-origin sub-batch as an image: 13 x 5
assert sw.N_SHARED % SHARED_WIDTH == 0


def build_libs(tmp):
    """every checker the sweep compares against, compiled once -> a dict"""
    return {"paths": (oe.build(tmp), osun.build(tmp), oracle_rays.build(tmp), oracle_lens.build(tmp), oracle_hdr.build(tmp), om.build(tmp)),
            "guides": GG.build(tmp), "moments": OM.build(tmp)}


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return build_libs(tmp_path_factory.mktemp("oracle_sample_sweep"))


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def refs_of(libs, O, V, case, pose=None):
    """test_gpu_emit_mis.Refs of the case's world, pose, frame and lens, with the case's uniforms in the checker's scene"""
    r = tem.Refs(libs["paths"], O, V, case.world, pose=pose or case.pose, lens=case.lens, W=case.W, H=case.H,
                 bounds=case.bounds or ())
    r.scene = case.scene(O, r.cam)
    assert np.array_equal(r.list, case.list)
    return r


def upload(c, case):
    c.upload_octree(case.tex, case.dim)


def settings(c, case, r):
    """the case's camera, uniforms and scheduled setting into a context that holds its tree"""
    s = case.setting
    c.set_camera(*r.cam)
    c.set_params(case.fill_params(c.default_params()))
    c.set_variant(s["variant"])
    c.set_lens(0.0, 1.0)
    c.set_path_depth(s["D"])
    c.set_sun_disc(s["radius"])
    c.set_emitter_sampling(s["rule"] != "off")
    c.set_emitter_importance(1 if s["rule"].startswith("power") else 0)
    c.set_emitter_mis(1 if s["rule"] == "power+mis" else 0)
    c.set_guide_glass(False)


def load(c, case, r):
    upload(c, case)
    settings(c, case, r)


def reset(c):
    """every context setting a case touches, back to its default"""
    tem._reset(c)
    c.set_guide_glass(False)
    c.set_params(c.default_params())


def _mean(samples):
    n = len(samples)
    out = ((sum(s.astype(np.uint64) for s in samples) + n // 2) // n).astype(np.uint8)
    out[..., 3] = 255
    return out


def _hdr_sums(HH, rgbs):
    sums = np.zeros(rgbs[0].shape, np.float64)
    for rgb in rgbs:
        rgb = np.ascontiguousarray(rgb, F)
        HH.o_hdr_add(sums.ctypes.data, rgb.ctypes.data, None, rgb.size)
    mean = np.zeros(rgbs[0].shape, F)
    counts = np.full(len(mean), len(rgbs), np.uint32)
    HH.o_hdr_mean(sums.ctypes.data, counts.ctypes.data, len(mean), mean.ctypes.data)
    return sums, mean


def run_case(c, V, O, libs, case, report=lambda route, check: check(), resident=False):
    """every route of the sweep on one case; report(route, check) runs one route's comparison (the fuzzer's catches the assertion);
    resident: the context already holds the case's tree (test_gpu_edit_sessions.py runs these bodies on a tree that patches left
    behind), only the settings are made"""
    import torch
    s, W, H, name = case.setting, case.W, case.H, case.name()
    source, D, radius, on = s["source"], s["D"], s["radius"], ON[s["rule"]]
    jitter, lens = tge.ALL_SOURCES[source]
    ap, focus = case.lens if lens else (0.0, 1.0)
    r = refs_of(libs, O, V, case)
    LL, HH, LG, ML = r.LL, r.HH, libs["guides"], libs["moments"]
    same = lambda got, ref, what: tge._same(got, ref, f"{name}: {what}", W)   # noqa: E731
    device = case.index % 3 == 0
    side = torch.cuda.Stream(device="cuda:0") if device else None
    (settings if resident else load)(c, case, r)
    assert np.array_equal(c.emitters(), case.list), f"{name}: the emitter list"

    report("accum forms", lambda: tge._forms(c, r, source, D, radius, on, W, H, what=name))

    def moments():
        tge._begin(c, r, source, W=W, H=H, hdr=True, moments=True)
        assert c.accum_add(1) == 1 and c.accum_add(2) == 3
        acc = OM.Accum(ML, H, W)
        for k in range(3):
            acc.add(r.sample(source, D, radius, k, on)[2].reshape(H, W, 3))
        same(tge._bits(c.accum_variance()), tge._bits(acc.variance()), "moments: variance plane")
        same(tge._bits(c.accum_resolve_hdr("clamp", 1.0)[0]), tge._bits(acc.mean()), "moments: float mean")
        same(c.accum_resolve()[1], r.frame_id(), "moments: id_dist")
    report("accum moments", moments)

    def primary():
        for mode in (0, 1):
            c.set_lens(ap, focus)
            c.accum_begin(W, H, 0, mode=mode, jitter=jitter)
            assert c.accum_add(3) == 3
            rgba, idd, _ = c.accum_resolve()
            same(rgba, _mean([oracle_lens.render(LL, r.scene, W, H, mode, k, ap, focus, jitter=jitter)[0] for k in range(3)]),
                 f"primary mode {mode} rgba8")
            same(idd, O.render(r.scene, W, H, mode)[1], f"primary mode {mode} id_dist")
    report("accum primary modes", primary)

    def guides():
        for glass in (False, True):
            c.set_guide_glass(glass)
            tge._begin(c, r, source, W=W, H=H)
            assert c.accum_add(3) == 3 and c.accum_add(5) == 8
            want = (GG if glass else G).planes(LG, r.scene, W, H, 0, 8, jitter, ap, focus)[0]
            G.same(c.accum_guides(), want, f"{name}: accum_guides glass {glass}")
            if device:
                bufs = {k: torch.zeros(want[k].shape, dtype=torch.float32, device="cuda:0") for k in G.KEYS}
                torch.cuda.synchronize()
                c.accum_guides_device(*(bufs[k].data_ptr() for k in G.KEYS), stream=side.cuda_stream)
                torch.cuda.synchronize()
                G.same({k: bufs[k].cpu().numpy() for k in G.KEYS}, want, f"{name}: accum_guides_device glass {glass}")
        c.set_guide_glass(False)
    report("accum guides", guides)

    o_all, d_all = case.rays
    batches = (("list", o_all, d_all, None), ("shared", case.shared_origin, d_all[:sw.N_SHARED], SHARED_WIDTH))

    def rays():
        for tag, o, d, width in batches:
            n = len(d)
            o3 = o if o.ndim == 2 else np.tile(o, (n, 1))
            for mode in (0, 1):
                want = oracle_rays.shade(r.R, r.scene, o, d, mode, width=width, sample=0)
                got = c.shade_rays(o, d, mode, width=width)
                same(got[0], want[0], f"shade_rays {tag} mode {mode} rgba8")
                same(got[1], want[1], f"shade_rays {tag} mode {mode} id_dist")
            smp = [r.shade(o, d, D, radius, k, on, n if width is None else width) for k in (5, 6, 7)]
            want = _mean([x[0] for x in smp])
            got = c.shade_rays(o, d, 2, width=width, first_sample=5, n_samples=3)
            same(got[0], want, f"shade_rays {tag} mode 2 samples 5..7 rgba8")
            same(got[1], smp[0][1], f"shade_rays {tag} mode 2 id_dist")
            sums, mean = _hdr_sums(HH, [x[2] for x in smp])
            rgb, rgba, idd = c.shade_rays_hdr(o, d, 2, width=width, first_sample=5, n_samples=3, tonemap="reinhard", exposure=1.7)
            same(tge._bits(rgb), tge._bits(mean), f"shade_rays_hdr {tag} float mean")
            same(rgba, oracle_hdr.tonemap(HH, mean[None], "reinhard", 1.7)[0], f"shade_rays_hdr {tag} reinhard bytes")
            same(idd, smp[0][1], f"shade_rays_hdr {tag} id_dist")
            # caller sums, 1 + 2: the only form that takes them is the device one
            t_o, t_d = torch.from_numpy(np.ascontiguousarray(o3)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(d)).to("cuda:0")
            t_sums = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
            t_rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda:0")
            t_rgba = torch.zeros((n, 4), dtype=torch.uint8, device="cuda:0")
            t_id = torch.zeros((n, 2), dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            stream = side.cuda_stream if device else None
            prior = 0
            for ns in (1, 2):
                c.shade_rays_hdr_device(n, t_o.data_ptr(), 3, t_d.data_ptr(), t_rgb.data_ptr(), t_rgba.data_ptr(), t_id.data_ptr(),
                                        t_sums.data_ptr(), n_prior=prior, mode=2, width=width, first_sample=5 + prior, n_samples=ns,
                                        tonemap="reinhard", exposure=1.7, stream=stream)
                prior += ns
            c.synchronize()
            torch.cuda.synchronize()
            same(t_sums.cpu().numpy().view(np.uint64), sums.view(np.uint64), f"shade_rays_hdr_device {tag} 1 + 2 float64 sums")
            same(tge._bits(t_rgb.cpu().numpy()), tge._bits(mean), f"shade_rays_hdr_device {tag} 1 + 2 float mean")
            same(t_rgba.cpu().numpy(), oracle_hdr.tonemap(HH, mean[None], "reinhard", 1.7)[0], f"shade_rays_hdr_device {tag} bytes")
            same(t_id.cpu().numpy(), smp[0][1], f"shade_rays_hdr_device {tag} id_dist")
            if device:
                c.shade_rays_device(n, t_o.data_ptr(), 3, t_d.data_ptr(), t_rgba.data_ptr(), t_id.data_ptr(), 2, width=width, first_sample=5,
                                    n_samples=3, stream=stream)
                torch.cuda.synchronize()
                same(t_rgba.cpu().numpy(), want, f"shade_rays_device {tag} mode 2 rgba8")
                same(t_id.cpu().numpy(), smp[0][1], f"shade_rays_device {tag} mode 2 id_dist")
    report("ray batches", rays)

    def guide_rays():
        for tag, o, d, width in batches:
            n = len(d)
            for glass in (False, True):
                c.set_guide_glass(glass)
                want = (GG if glass else G).ray_planes(LG, r.scene, o, d)
                G.same(c.guide_rays(o, d, width=width), want, f"{name}: guide_rays {tag} glass {glass}", keys=RAY_KEYS)
                if device:
                    o3 = o if o.ndim == 2 else np.tile(o, (n, 1))
                    t_o, t_d = torch.from_numpy(np.ascontiguousarray(o3)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(d)).to("cuda:0")
                    t_n = torch.zeros((n, 3), dtype=torch.float32, device="cuda:0")
                    t_a = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
                    t_z = torch.zeros(n, dtype=torch.float32, device="cuda:0")
                    t_h = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    c.guide_rays_device(n, t_o.data_ptr(), 3, t_d.data_ptr(), t_n.data_ptr(), t_a.data_ptr(), t_z.data_ptr(), t_h.data_ptr(),
                                        width=width, stream=side.cuda_stream)
                    torch.cuda.synchronize()
                    got = {"normal": t_n.cpu().numpy(), "albedo": t_a.cpu().numpy(), "depth": t_z.cpu().numpy(), "hit": t_h.cpu().numpy() != 0}
                    G.same(got, want, f"{name}: guide_rays_device {tag} glass {glass}", keys=RAY_KEYS)
        c.set_guide_glass(False)
    report("guide rays", guide_rays)

    if case.outside_pose is not None:
        def outside():
            """the eye outside the world bounds, looking in: sky on every pixel by the shader's rule, on every route all the same"""
            r2 = refs_of(libs, O, V, case, pose=case.outside_pose)
            c.set_camera(*r2.cam)
            assert not np.any(r2.frame_id()[..., 0])
            tge._begin(c, r2, source, W=W, H=H)
            assert c.accum_add(3) == 3
            got = c.accum_resolve()
            same(got[0], r2.mean(source, D, radius, 0, 3, on), "eye outside the world: rgba8 after 3")
            same(got[1], r2.frame_id(), "eye outside the world: id_dist")
            for glass in (False, True):
                c.set_guide_glass(glass)
                tge._begin(c, r2, source, W=W, H=H)
                assert c.accum_add(3) == 3
                G.same(c.accum_guides(), (GG if glass else G).planes(LG, r2.scene, W, H, 0, 3, jitter, ap, focus)[0],
                       f"{name}: eye outside the world: accum_guides glass {glass}")
            c.set_guide_glass(False)
        report("eye outside the world", outside)


@pytest.mark.parametrize("index", range(sw.N_INDEX))
@pytest.mark.parametrize("family", sw.FAMILIES)
def test_sweep_case(ctx, V, O, libs, family, index):
    case = sw.case(V, O, family, index)
    try:
        run_case(ctx, V, O, libs, case)
    finally:
        case.close()
        reset(ctx)
