"""Seeded edit sessions on the MI355X: the 12 sessions of edit_sessions.py, one Context each from the first upload to the last
checkpoint, never re-created. The first stream goes up once (upload_octree where the index is even, upload_records where it is odd);
every edit after it reaches the device as a patch, a box patch, a batch or a compaction (the full upload only where a patch is
refused). At each of the three checkpoints the PATCHED context is held bit for bit to the checkers of test_gpu_sample_sweep.build_libs on
the edited world's own flatten(), at the case's scheduled depth, sun radius, emitter rule, ray source and variant:

  * the ray batches' device forms on a caller's stream, enqueued directly after the last patch with no host wait of the test's own
    (index even);
  * the accumulation that was alive across the group -- begun before it from the scheduled source with HDR and moments, three samples
    in, guides up to date: the next accum_add(2) returns 2 (the edit restarted the sums), and its resolve, HDR resolve, variance and
    guide planes are those of samples 0 and 1 on the EDITED world (an accumulation takes the guide rule its begin reads: past glass
    and plain in turn over the groups; it is not adaptive, so it has no accum_counts: those are compared on the adaptive run below);
  * emitters() and emitter_cdf() against the walk; frames in modes 0, 1, 2 with the miss tiles on (after four repeats, so that the mask
    of the new tree exists) and off, at the scheduled variant and the other of {0, 1}; cast_rays on the 65 shared-origin rays and
    find_voxels on the edited voxels against the oracle's own functions on a pointer tree edited in step;
  * a plain accumulation of 3 samples, an adaptive one (min 2, max 4) with its counts, the primary modes with 2 samples;
  * shade_rays in modes 0, 1, 2 (samples 5 .. 6), shade_rays_hdr and guide_rays with glass off and on, on the redrawn batch of 257 rays
    and the shared-origin batch.

After the last checkpoint: test_gpu_sample_sweep.run_case's own route bodies on the resident, patched tree; then compact(), and the live accumulation's comparison once more. The long session (`mixed` 1) also asserts that
scene_info()["n_records"] fell between two consecutive edits of its long run: vrt_patch_plan compacted by itself while the accumulation
was alive. run_session() is shared with fuzz/fuzz_edits.py; every failure message carries `edit session FAMILY INDEX checkpoint K: route`."""
import time

import numpy as np
import pytest

import edit_sessions as es
import oracle_adaptive
import oracle_emit_power as oep
import oracle_guides as G
import oracle_guides_glass as GG
import oracle_hdr
import oracle_lens
import oracle_moments as OM
import oracle_rays
import sample_sweep_worlds as sw
import test_gpu_emitters as tge
import test_gpu_queries as tq
import test_gpu_sample_sweep as tgs

pytestmark = pytest.mark.gpu
F = np.float32
KEYS = [(f, i) for f in es.FAMILIES for i in es.INDICES]
ADAPTIVE = (2, 4, 8)                   # min, max, tolerance
MISS_REPEATS = 4


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return tgs.build_libs(tmp_path_factory.mktemp("oracle_edit_sessions"))


def bounds_of(case):
    return case.bounds or ((-1023,) * 3, (1024,) * 3)


def run_session(c, V, O, libs, family, index, seed=es.SEED, plan=None, report=lambda route, check: check(), times=None):
    """one whole session on context c; report(route, check) runs one route's comparison (the fuzzer's catches the assertion)"""
    import torch
    device = index % 2 == 0
    side = torch.cuda.Stream(device="cuda:0") if device else None
    LG, ML = libs["guides"], libs["moments"]
    st = {}

    def begin_live(r, cp, glass):
        """the accumulation that lives across the next group: HDR with moments, three samples, guides up to date. An accumulation
        takes the guide rule its begin reads, so one live accumulation carries one: past glass and plain in turn"""
        st["live_glass"] = glass
        c.set_guide_glass(glass)
        tge._begin(c, r, cp.setting["source"], W=cp.W, H=cp.H, hdr=True, moments=True)
        c.set_guide_glass(False)
        assert c.accum_add(3) == 3, f"{cp.name()}: the live accumulation's first add"
        c.accum_guides()

    def live(r, cp, why):
        """the accumulation begun before the edit, after it: restarted, and samples 0 and 1 of the edited world"""
        s, W, H, name = cp.setting, cp.W, cp.H, cp.name()
        source, D, radius, on = s["source"], s["D"], s["radius"], tgs.ON[s["rule"]]
        jitter, lens = tge.ALL_SOURCES[source]
        ap, focus = cp.lens if lens else (0.0, 1.0)
        same = lambda got, ref, what: tge._same(got, ref, f"{name}: live accumulation {why}: {what}", W)   # noqa: E731
        assert c.accum_add(2) == 2, f"{name}: live accumulation {why}: the edit did not restart the sums"
        acc = OM.Accum(ML, H, W)
        for k in range(2):
            acc.add(r.sample(source, D, radius, k, on)[2].reshape(H, W, 3))
        got = c.accum_resolve()
        same(got[0], r.mean(source, D, radius, 0, 2, on), "rgba8")
        same(got[1], r.frame_id(), "id_dist")
        rgb, rgba, _ = c.accum_resolve_hdr("reinhard", 1.7)
        same(tge._bits(rgb), tge._bits(acc.mean()), "float mean")
        same(rgba, oracle_hdr.tonemap(r.HH, acc.mean(), "reinhard", 1.7), "reinhard bytes")
        same(tge._bits(c.accum_variance()), tge._bits(acc.variance()), "variance plane")
        glass = st["live_glass"]
        want = (GG if glass else G).planes(LG, r.scene, W, H, 0, 2, jitter, ap, focus)[0]
        G.same(c.accum_guides(), want, f"{name}: live accumulation {why}: accum_guides glass {glass}")

    def target(S):
        case = S.case
        st["mirror"] = es.Mirror(O, S)
        st["eye"] = S.eye.astype(F)
        r = tgs.refs_of(libs, O, V, case)
        c.set_params(case.fill_params(c.default_params()))
        if device:
            c.upload_octree(case.tex, case.dim)
        else:
            c.upload_records(case.records, case.dim)
        tgs.settings(c, case, r)
        c.set_option(V.OPT_MISS_TILES, 1)
        st["refs"], st["cp"] = r, case
        return c

    def before_group(S, k, t):
        report("live accumulation begun", lambda: begin_live(st["refs"], st["cp"], (k + index) % 2 == 0))
        st["t0"] = time.perf_counter()

    def device_forms(cp):
        """enqueued on the caller's stream straight after the last patch: the only waits before them are the library's own"""
        out = []
        for tag, o, d, width in batches_of(cp):
            n = len(d)
            o3 = o if o.ndim == 2 else np.tile(o, (n, 1))
            t_o, t_d = torch.from_numpy(np.ascontiguousarray(o3)).to("cuda:0", non_blocking=True), torch.from_numpy(np.ascontiguousarray(d)).to("cuda:0", non_blocking=True)
            t_rgba = torch.zeros((n, 4), dtype=torch.uint8, device="cuda:0")
            t_id = torch.zeros((n, 2), dtype=torch.int32, device="cuda:0")
            g = [torch.zeros(shape, dtype=dt, device="cuda:0") for shape, dt in (((n, 3), torch.float32), ((n, 4), torch.float32), ((n,), torch.float32),
                                                                                  ((n,), torch.uint8))]
            side.wait_stream(torch.cuda.current_stream(device="cuda:0"))         # a wait on the device, none on the host
            c.shade_rays_device(n, t_o.data_ptr(), 3, t_d.data_ptr(), t_rgba.data_ptr(), t_id.data_ptr(), 2, width=width, first_sample=5, n_samples=2,
                                stream=side.cuda_stream)
            c.guide_rays_device(n, t_o.data_ptr(), 3, t_d.data_ptr(), *(x.data_ptr() for x in g), width=width, stream=side.cuda_stream)
            out.append((tag, t_o, t_d, t_rgba, t_id, g))
        return out

    def batches_of(cp):
        o_all, d_all = cp.rays
        return (("list", o_all, d_all, None), ("shared", cp.shared_origin, d_all[:sw.N_SHARED], tgs.SHARED_WIDTH))

    def at_checkpoint(S, cp, counts, t):
        s, W, H, name = cp.setting, cp.W, cp.H, cp.name()
        source, D, radius, on = s["source"], s["D"], s["radius"], tgs.ON[s["rule"]]
        jitter, lens = tge.ALL_SOURCES[source]
        ap, focus = cp.lens if lens else (0.0, 1.0)
        same = lambda got, ref, what: tge._same(got, ref, f"{name}: {what}", W)   # noqa: E731
        queued = device_forms(cp) if device else None
        st["patch_seconds"] = st.get("patch_seconds", 0.0) + time.perf_counter() - st["t0"]
        st["counts"] = st.get("counts", []) + [counts]
        r = tgs.refs_of(libs, O, V, cp)
        st["refs"], st["cp"] = r, cp
        HH = r.HH

        if device:
            def on_stream():
                torch.cuda.synchronize()
                for (tag, o, d, width), (_, _, _, t_rgba, t_id, g) in zip(batches_of(cp), queued):
                    smp = [r.shade(o, d, D, radius, k, on, len(d) if width is None else width) for k in (5, 6)]
                    same(t_rgba.cpu().numpy(), tgs._mean([x[0] for x in smp]), f"shade_rays_device after the last patch {tag} rgba8")
                    same(t_id.cpu().numpy(), smp[0][1], f"shade_rays_device after the last patch {tag} id_dist")
                    got = {"normal": g[0].cpu().numpy(), "albedo": g[1].cpu().numpy(), "depth": g[2].cpu().numpy(), "hit": g[3].cpu().numpy() != 0}
                    G.same(got, G.ray_planes(LG, r.scene, o, d), f"{name}: guide_rays_device after the last patch {tag}", keys=tgs.RAY_KEYS)
            report("device forms after the last patch", on_stream)

        report("live accumulation", lambda: live(r, cp, "across the group"))

        def emitters():
            assert np.array_equal(c.emitters(), cp.list), f"{name}: emitters()"
            want = np.array(oep.thresholds([int(w) for w in cp.weights]), np.uint32).reshape(-1)
            assert np.array_equal(c.emitter_cdf(), want), f"{name}: emitter_cdf()"
        report("emitter list and table", emitters)

        def frames():
            want = {mode: O.render(r.scene, W, H, mode)[:2] for mode in (0, 1, 2)}
            for variant in (s["variant"], 1 - s["variant"]):
                c.set_variant(variant)
                for tiles in (1, 0):
                    c.set_option(V.OPT_MISS_TILES, tiles)
                    for mode in (0, 1, 2):
                        for _ in range(MISS_REPEATS if tiles else 1):
                            got = c.dispatch(W, H, mode)
                        same(got[0], want[mode][0], f"dispatch variant {variant} miss tiles {tiles} mode {mode} rgba8")
                        same(got[1], want[mode][1], f"dispatch variant {variant} miss tiles {tiles} mode {mode} id_dist")
            c.set_option(V.OPT_MISS_TILES, 1)
            c.set_variant(s["variant"])
        report("frames", frames)

        def queries():
            tree, box = st["mirror"].tree, tuple(tuple(float(v) for v in b) for b in bounds_of(cp))
            assert np.array_equal(O.flatten(tree)[0], cp.tex), f"{name}: the mirrored pointer tree is not the edited world"
            dirs = cp.rays[1][:sw.N_SHARED]
            pts = np.array(cp.edited, np.int32).reshape(-1, 3)
            hit, coord, place, leaf, steps = c.cast_rays(st["eye"], dirs, box)
            present, words = c.find_voxels(pts)
            with tq.zero_leaves_emptied(tree):
                tq.compare_rays(O, tree, st["eye"], dirs, box, f"{name}: cast_rays", True, hit, coord, place, leaf)
                tq.compare_points(O, O.lib(), cp.world, tree, pts, present, words, f"{name}: find_voxels")
            assert steps.min() >= 1 and steps.max() <= 512, f"{name}: cast_rays steps"
        report("queries", queries)

        def plain():
            for glass in (False, True):                  # an accumulation takes the guide rule its begin reads
                c.set_guide_glass(glass)
                tge._begin(c, r, source, W=W, H=H)
                assert c.accum_add(3) == 3
                got = c.accum_resolve()
                same(got[0], r.mean(source, D, radius, 0, 3, on), "plain accumulation rgba8 after 3")
                same(got[1], r.frame_id(), "plain accumulation id_dist")
                G.same(c.accum_guides(), (GG if glass else G).planes(LG, r.scene, W, H, 0, 3, jitter, ap, focus)[0],
                       f"{name}: plain accumulation accum_guides glass {glass}")
            c.set_guide_glass(False)
        report("plain accumulation", plain)

        def adaptive():
            tge._begin(c, r, source, W=W, H=H, adaptive=ADAPTIVE)
            assert c.accum_add(2) == 2 and c.accum_add(2) == 4
            got = c.accum_resolve()
            cnt, active = c.accum_counts()
            ref = oracle_adaptive.accumulate(lambda k: r.sample(source, D, radius, k, on)[0].reshape(H, W, 4), H, W, 0, 4, ADAPTIVE, np.int64)
            assert np.array_equal(cnt, ref.counts()), f"{name}: adaptive counts"
            assert active == int(ref.active(ADAPTIVE).sum()), f"{name}: adaptive active pixels"
            same(got[0], ref.resolve(), "adaptive rgba8")
            same(got[1], r.frame_id(), "adaptive id_dist")
        report("adaptive accumulation", adaptive)

        def primary():
            for mode in (0, 1):
                c.set_lens(ap, focus)
                c.accum_begin(W, H, 0, mode=mode, jitter=jitter)
                assert c.accum_add(2) == 2
                rgba, idd, _ = c.accum_resolve()
                same(rgba, tgs._mean([oracle_lens.render(r.LL, r.scene, W, H, mode, k, ap, focus, jitter=jitter)[0] for k in range(2)]),
                     f"primary mode {mode} rgba8")
                same(idd, O.render(r.scene, W, H, mode)[1], f"primary mode {mode} id_dist")
        report("accum primary modes", primary)

        def rays():
            for tag, o, d, width in batches_of(cp):
                n = len(d)
                for mode in (0, 1):
                    want = oracle_rays.shade(r.R, r.scene, o, d, mode, width=width, sample=0)
                    got = c.shade_rays(o, d, mode, width=width)
                    same(got[0], want[0], f"shade_rays {tag} mode {mode} rgba8")
                    same(got[1], want[1], f"shade_rays {tag} mode {mode} id_dist")
                smp = [r.shade(o, d, D, radius, k, on, n if width is None else width) for k in (5, 6)]
                got = c.shade_rays(o, d, 2, width=width, first_sample=5, n_samples=2)
                same(got[0], tgs._mean([x[0] for x in smp]), f"shade_rays {tag} mode 2 samples 5..6 rgba8")
                same(got[1], smp[0][1], f"shade_rays {tag} mode 2 id_dist")
                _, mean = tgs._hdr_sums(HH, [x[2] for x in smp])
                rgb, rgba, idd = c.shade_rays_hdr(o, d, 2, width=width, first_sample=5, n_samples=2, tonemap="reinhard", exposure=1.7)
                same(tge._bits(rgb), tge._bits(mean), f"shade_rays_hdr {tag} float mean")
                same(rgba, oracle_hdr.tonemap(HH, mean[None], "reinhard", 1.7)[0], f"shade_rays_hdr {tag} reinhard bytes")
                same(idd, smp[0][1], f"shade_rays_hdr {tag} id_dist")
                for glass in (False, True):
                    c.set_guide_glass(glass)
                    G.same(c.guide_rays(o, d, width=width), (GG if glass else G).ray_planes(LG, r.scene, o, d),
                           f"{name}: guide_rays {tag} glass {glass}", keys=tgs.RAY_KEYS)
                c.set_guide_glass(False)
        report("ray batches", rays)

    S = None
    try:
        S, groups = es.run(V, O, family, index, target=target, at_checkpoint=at_checkpoint, before_group=before_group, seed=seed, plan=plan,
                           mirror=lambda *a: st["mirror"](*a))
        cp, r = groups[-1][2], st["refs"]

        # the sweep's own route bodies, at their own sample counts, on the tree as the patches left it
        tgs.run_case(c, V, O, libs, cp, report=lambda route, check: report(f"sweep routes on the patched tree: {route}", check), resident=True)

        def after_compaction():
            begin_live(r, cp, (len(groups) + index) % 2 == 0)
            c.compact()
            live(r, cp, "across compact()")
        report("after the last checkpoint", after_compaction)
        if (family, index % len(es.INDICES)) == es.LONG and plan is None:
            rec, own = st["counts"][-1]["records"], st["counts"][-1]["own"]
            # after a patch that was applied: not after a full upload or an explicit compact(), which lower the count too
            falls = [j for j in range(1, len(rec)) if rec[j] < rec[j - 1] and own[j]]
            assert falls, f"edit session {family} {index}: n_records never fell during the long run: vrt_patch_plan did not compact by itself"
        if times is not None:
            times["patch_seconds"] = st["patch_seconds"]
            times["edits"] = sum(x["edits"] for x in st["counts"])
            times["fallbacks"] = sum(x["fallbacks"] for x in st["counts"])
    finally:
        if "mirror" in st:
            st["mirror"].close()
        if S is not None:
            S.close()
        tgs.reset(c)
        c.set_option(V.OPT_MISS_TILES, 1)


@pytest.mark.parametrize("family,index", KEYS)
def test_edit_session(V, O, libs, family, index):
    c = V.Context(0)                                     # one context per session: it lives from the first upload to the last checkpoint
    t0, times = time.perf_counter(), {}
    try:
        run_session(c, V, O, libs, family, index, times=times)
    finally:
        c.close()
    print(f"edit session {family} {index}: {time.perf_counter() - t0:.1f} s in all, checkers included; {times.get('edits')} patch operations "
          f"({times.get('fallbacks')} full uploads) in {times.get('patch_seconds', 0.0):.2f} s, world edits and planning included")


def test_a_batch_goes_on_after_a_patch_that_voids_the_wide_layout(V, O):
    """PatchBatch::wide_invalid on the device, by hand-written streams in the world [0, 8)^3 (edit_sessions.VOID_STEPS; the host half
    is test_edit_sessions.py's test of the same name): a context that renders through the wide layout takes one batch whose first
    patch voids that layout and whose next two go to the records alone; after patch_end the frames of every mode, on the wide
    variants' fall-back and the record-array variant, are the oracle's on the last step's own stream, the tracked texel count is
    that stream's, and an accumulation that was alive across the batch starts again."""
    import ctypes as C
    W, H = 64, 48
    start, final = es.hand_stream(es.VOID_START), es.hand_stream(es.VOID_STEPS[-1][2])
    ip, iv, cp, _ = V.camera_block((1.3, 2.1, 0.7), 52.0, 18.0, W, H)

    def oracle(tex, mode):
        s = O.make_scene(tex, es.VOID_DIM, ip, iv, cp)
        s.bounds_min[:], s.bounds_max[:] = es.VOID_BOUNDS
        return O.render(s, W, H, mode)[:2]

    c = V.Context(0)
    try:
        p = c.default_params()
        p.world_min[:], p.world_max[:] = es.VOID_BOUNDS
        c.set_params(p)
        c.upload_octree(start, es.VOID_DIM)
        c.set_camera(ip, iv, cp)
        for mode in (0, 1, 2):                           # the wide layout is built and in use
            got, want = c.dispatch(W, H, mode), oracle(start, mode)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"before the batch, mode {mode}"
        c.accum_begin(W, H, 0, mode=2)
        assert c.accum_add(3) == 3
        c.patch_begin()
        for voxel, path, tree in es.VOID_STEPS:
            plan = V.Patch()
            assert c._L.vrt_patch_plan(c._h, *voxel, 15, C.byref(plan)) == 0, voxel
            assert list(plan.path[:plan.depth]) == path, (voxel, list(plan.path[:plan.depth]))
            rec = V.subtree_records(es.hand_stream(tree), path)
            c._chk(c._L.vrt_patch_apply(c._h, C.byref(plan), rec.ctypes.data, len(rec)))
        c.patch_end()
        info = c.scene_info()
        assert (info["n_texels"], info["tex_dim"]) == (len(final) // 4, es.VOID_DIM), info
        assert c.accum_add(2) == 2, "the batch did not restart the sums"
        for variant in (0, 1):
            c.set_variant(variant)
            for mode in (0, 1, 2):
                got, want = c.dispatch(W, H, mode), oracle(final, mode)
                tge._same(got[0], want[0], f"after the batch: variant {variant} mode {mode} rgba8", W)
                tge._same(got[1], want[1], f"after the batch: variant {variant} mode {mode} id_dist", W)
    finally:
        c.close()
