"""The per-launch profiler (vrt_set_profiling / vrt_set_profiling_stride / vrt_profile_read) and vrt_dispatch_timed on the MI355X:
which launches take a slot and how many, that each entry is the time of its own launch, that the event pair on the dispatch packet
spans the whole launch, and that a profiled launch (hipExtLaunchKernelGGL) writes the bytes of an unprofiled one (hipLaunchKernelGGL).

The reference is independent of the library: the test's own torch.cuda.Event(enable_timing=True) pairs on a stream of its own, which
it hands to the device-pointer entry points -- marker packets around the call, where the profiler reads the kernel's own packet.

    B        the cost of an empty bracket: the median over 200 such pairs around one single-wave torch operation, each queued
             behind about 1 ms of work so that the host's enqueue latency is not inside the pair. Measured at the start of the module.
    nesting  the packet's begin and end lie between the two markers of an in-order stream: prof <= bracket + B (one B of marker
             granularity)
    span     nothing the launch runs is left out: bracket - prof <= 3 B for launches of at least 10 B (the bracket adds the two
             markers B measures; the factor 3 is other tenants' jitter)

Every timing is the median of 9 repetitions after 3 untimed ones; every bracketed launch is queued behind a blocker like B's pairs, with
feedback scheduling and miss tiles off (the trace kernels are then all enqueue() puts on the stream). The host-pointer entry points
run on the context's own stream, which a caller cannot bracket: they are counted and compared byte for byte only.

With VRT_PROFILER_CHECK_OUT set, everything measured goes to that file (profiles/profiler_check.txt is one such run)."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_INVALID = -1   # include/vrt.h VRT_E_INVALID
REPS, WARM = 9, 3
_LOG = []


def _log(line):
    _LOG.append(line)
    print(line)


class Reference:
    """the independent instrument: a stream, a blocker of about 1 ms, timing event pairs"""

    def __init__(self):
        import torch
        self.torch = torch
        self.s = torch.cuda.Stream()
        self.big = torch.zeros(128 << 20, dtype=torch.float32, device="cuda")   # 512 MiB read and written per blocker operation
        self.small = torch.zeros(64, dtype=torch.float32, device="cuda")        # one wave
        torch.cuda.synchronize()
        t = []
        for _ in range(8):
            e0, e1 = self.pair()
            e0.record(self.s)
            with torch.cuda.stream(self.s):
                self.big.add_(1.0)
            e1.record(self.s)
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        self.block_op_ms = float(np.median(t[3:]))
        self.n_block = int(min(32, max(1, math.ceil(1.0 / self.block_op_ms))))
        ev = [self.bracket(self._one_wave) for _ in range(200)]
        self.s.synchronize()
        b = np.array([a.elapsed_time(z) for a, z in ev])
        self.B = float(np.median(b))
        _log(f"blocker: {self.n_block} x {self.block_op_ms:.4f} ms; B = {self.B:.6f} ms (median of 200 pairs around one single-wave "
             f"operation; min {b.min():.6f}, 90th percentile {np.percentile(b, 90):.6f})")

    def pair(self):
        return self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)

    def _one_wave(self, _stream):
        with self.torch.cuda.stream(self.s):
            self.small.add_(1.0)

    def bracket(self, fn):
        """fn(stream handle) between two markers, behind the blocker -> the event pair (read it after a synchronize)"""
        e0, e1 = self.pair()
        with self.torch.cuda.stream(self.s):
            for _ in range(self.n_block):
                self.big.add_(1.0)
        e0.record(self.s)
        fn(self.s.cuda_stream)
        e1.record(self.s)
        return e0, e1

    def brackets(self, fn, reps=REPS):
        ev = [self.bracket(fn) for _ in range(reps)]
        self.s.synchronize()
        return np.array([a.elapsed_time(z) for a, z in ev], np.float64)


@pytest.fixture(scope="module")
def T():
    _log("profiler check, commit " + os.environ.get("VRT_PROFILER_CHECK_COMMIT", "(not given)") + "; times in ms, medians of "
         f"{REPS} after {WARM} untimed")
    t = Reference()
    yield t
    out = os.environ.get("VRT_PROFILER_CHECK_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(_LOG) + "\n")


def _tx(value, alpha):
    return [value & 255, (value >> 8) & 255, (value >> 16) & 255, alpha]


@pytest.fixture(scope="module")
def scenes(V, product_scenes, golden):
    """the smallest scenes of test_gpu_parity.py at their frame sizes there, a model scene at 64 x 48, and the room (H of the contrasts)"""
    from conftest import random_voxels
    leaf = [200, 40, 90, 255, 255, 0, 0, 255]
    regular = _tx(1, 0x81) + _tx(3 | 0x800000, 0) + _tx(5, 0) + leaf + _tx(6, 0x01) + _tx(7 | 0x800000, 0) + leaf
    unit = (_tx(1, 0x80) + _tx(2, 0) + _tx(3, 0x01) + _tx(4, 0) + _tx(5, 0x01) + _tx(6, 0) + _tx(7, 0x80) + _tx(8 | 0x800000, 0) + leaf)
    w = V.World(world_min=(-64,) * 3, world_max=(192,) * 3)
    w.insert_many(*random_voxels(np.random.default_rng(4), 5000, -60, 70))
    tex192, dim192 = w.flatten()
    w.close()
    small = dict(wmin=(0, 0, 0), wmax=(8, 8, 8), pos=(1.3, 2.1, 0.7), yaw=52.0, pitch=18.0, W=64, H=48, dim=3)
    room = golden["frames"]["frames"]["room_inside_720p_full/mode2"]["pose"]
    return {
        "regular": dict(small, tex=np.array(regular, np.uint8)),
        "unit-internal": dict(small, tex=np.array(unit, np.uint8)),                      # the explicit-AABB kernels (trav 1)
        "world192": dict(tex=tex192, dim=dim192, wmin=(-64,) * 3, wmax=(192,) * 3, pos=(100.5, 90.5, 120.5), yaw=-130.0, pitch=-30.0,
                         W=128, H=80),                                                    # no wide layout: the record-array kernels (trav 2)
        "dragon": dict(tex=product_scenes["dragon"][0], dim=product_scenes["dragon"][1], wmin=None, wmax=None, pos=(63.5, 60.5, 140.5),
                       yaw=-90.0, pitch=-10.0, W=64, H=48),
        "room": dict(tex=product_scenes["room"][0], dim=product_scenes["room"][1], wmin=None, wmax=None, pos=tuple(room[:3]), yaw=room[3],
                     pitch=room[4], W=256, H=144),
    }


def _plain(c, V):
    """only the trace kernels on the stream: no order or mask kernels, no memsets"""
    c.set_tile_scheduling(0)
    c.set_option(V.OPT_MISS_TILES, 0)
    c.set_option(V.OPT_FULL_OPAQUE, 6)
    c.set_variant(0)
    c.set_profiling(0)


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    _plain(c, V)
    yield c
    c.close()


def _camera(c, V, sc, W=None, H=None, dyaw=0.0):
    ip, iv, cp, _ = V.camera_block(sc["pos"], sc["yaw"] + dyaw, sc["pitch"], W or sc["W"], H or sc["H"])
    if dyaw == 0.0:
        c.set_camera(ip, iv, cp)
    return ip, iv, cp


def _load(c, V, sc, W=None, H=None):
    _plain(c, V)
    c.upload_octree(sc["tex"], sc["dim"])
    p = c.default_params()
    if sc["wmin"] is not None:
        p.world_min[:] = sc["wmin"]
        p.world_max[:] = sc["wmax"]
    c.set_params(p)
    return _camera(c, V, sc, W, H)


class Bufs:
    """device images of up to four views, zeroed before a run and read whole after it"""

    def __init__(self, T, W, H, n=4):
        t = T.torch
        self.t = t
        self.rgba = [t.zeros(W * H, dtype=t.int32, device="cuda") for _ in range(n)]
        self.idd = [t.zeros(W * H * 2, dtype=t.int32, device="cuda") for _ in range(n)]

    def zero(self):
        self.t.cuda.synchronize()   # the fills run on torch's stream: after what the test's stream still runs, and done before the next launch
        for x in self.rgba + self.idd:
            x.zero_()
        self.t.cuda.synchronize()

    def fetch(self):
        self.t.cuda.synchronize()
        return [x.cpu().numpy() for x in self.rgba + self.idd]

    def views(self, c, V, sc, W, H, n=4):
        cams = [_camera(c, V, sc, W, H, dyaw) for dyaw in (0.0, 7.0, -9.0, 15.0)[:n]]
        return V.make_views([(ip, iv, cp, r.data_ptr(), i.data_ptr()) for (ip, iv, cp), r, i in zip(cams, self.rgba, self.idd)])


def _same(got, ref, what):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(r).view(np.uint8)), f"{what}: output {k} differs between a profiled and an unprofiled launch"


def _entries(c, n, what):
    ms = c.profile_read()
    assert len(ms) == n, f"{what}: {len(ms)} entries, expected {n}"
    assert np.all(np.isfinite(ms)) and np.all(ms > 0), f"{what}: {ms}"
    assert len(c.profile_read()) == 0, f"{what}: a second read returns entries again"
    return ms.astype(np.float64)


def _timed(c, T, fn, slots=1):
    """REPS bracketed, profiled calls of fn (after the untimed ones the caller made) -> (brackets, the profiler's time per call)"""
    c.set_profiling(REPS * slots)
    br = T.brackets(fn)
    pr = _entries(c, REPS * slots, "bracketed launches").reshape(REPS, slots)
    c.set_profiling(0)
    return br, pr


def _check_route(c, T, what, slots, fn, fetch, zero):
    """fn(stream) is one call of an entry point that takes `slots` slots: counts, bytes, and the nesting against the brackets"""
    s = T.s.cuda_stream
    c.set_profiling(0)
    zero()
    fn(s)
    ref = fetch()
    c.set_profiling(2 * slots + 1)
    for _ in range(2):
        zero()
        fn(s)
    got = fetch()
    _entries(c, 2 * slots, what)
    _same(got, ref, what)
    br, pr = _timed(c, T, fn, slots)   # the three calls above were the untimed ones
    d = br - pr.sum(axis=1)
    _log(f"{what}: bracket {np.median(br):.6f} profiler {np.median(pr.sum(axis=1)):.6f} difference {np.median(d):.6f}")
    assert np.median(d) >= -T.B, f"{what}: the profiler's time {np.median(pr.sum(axis=1)):.6f} exceeds the bracket {np.median(br):.6f} + B {T.B:.6f}"


def _frame_routes(c, V, sc, b, W, H, mode):
    r0, i0 = b.rgba[0].data_ptr(), b.idd[0].data_ptr()
    v1, v4 = b.views(c, V, sc, W, H, 1), b.views(c, V, sc, W, H, 4)
    return [("vrt_dispatch_rows", 1, lambda s: c.dispatch_rows(W, H, 0, H, mode, r0, i0, s)),
            ("vrt_dispatch_rows 3..H-5", 1, lambda s: c.dispatch_rows(W, H, 3, H - 5, mode, r0, i0, s)),
            ("vrt_dispatch_shard 1/2 x 8", 1, lambda s: c.dispatch_shard(W, H, 8, 1, 2, mode, r0, i0, s)),
            ("vrt_dispatch_tiles 1/3 x 5", 1, lambda s: c.dispatch_tiles(W, H, 5, 1, 3, mode, r0, i0, s)),
            ("vrt_dispatch_views 1", 1, lambda s: c.dispatch_views(W, H, H, 0, 1, mode, v1, s)),
            ("vrt_dispatch_views 4", 1, lambda s: c.dispatch_views(W, H, H, 0, 1, mode, v4, s)),   # four views: one launch, one slot
            ("vrt_dispatch_timed x 3", 3, lambda s: c.dispatch_timed(W, H, 0, H, mode, r0, i0, 3, s))]


@pytest.mark.parametrize("name", ["regular", "unit-internal", "world192", "dragon"])
def test_frame_launches_take_one_slot_each_and_keep_their_pixels(V, T, ctx, scenes, name):
    """Every device-pointer entry point in every mode (variant 0), and vrt_dispatch_rows on every variant the library accepts: one
    slot per launch (n for vrt_dispatch_timed(iters=n)), the same bytes profiled or not, the profiler's time within the bracket. The
    unit-internal stream takes trav 1 and the [-64, 192)^3 world trav 2 on every variant: mode 2 there is the record-array fallback
    of trace_full, which dropped its events. Then the host-pointer forms: vrt_dispatch and vrt_dispatch_frame (the display pass
    takes no slot)."""
    c, sc = ctx, scenes[name]
    W, H = sc["W"], sc["H"]
    _load(c, V, sc)
    b = Bufs(T, W, H)
    for v in V.available_variants():
        for mode in (0, 1, 2):
            c.set_variant(v)
            routes = _frame_routes(c, V, sc, b, W, H, mode)
            for what, slots, fn in routes if v == 0 else routes[:1]:
                _check_route(c, T, f"{name} {W}x{H} variant {v} mode {mode} {what}", slots, fn, b.fetch, b.zero)
    c.set_variant(0)
    for mode in (0, 1, 2):
        for what, run in (("vrt_dispatch", lambda: c.dispatch(W, H, mode)), ("vrt_dispatch_frame", lambda: c.dispatch_frame(W, H, mode))):
            c.set_profiling(0)
            ref = run()
            c.set_profiling(3)
            got = [run() for _ in range(2)][-1]
            _entries(c, 2, f"{name} mode {mode} {what}")
            _same(got, ref, f"{name} mode {mode} {what}")
    c.set_profiling(0)


def test_async_dispatch_is_one_slot_and_the_read_waits_by_itself(V, T, ctx, scenes):
    """vrt_dispatch_async into page-locked buffers, read without vrt_dispatch_wait: vrt_profile_read waits for the launches"""
    c, sc = ctx, scenes["dragon"]
    W, H = sc["W"], sc["H"]
    _load(c, V, sc)
    ref = c.dispatch(W, H, 1)
    pins = [(c.host_alloc((H, W, 4), np.uint8), c.host_alloc((H, W, 2), np.int32)) for _ in range(2)]
    try:
        c.set_profiling(4)
        tickets = [c.dispatch_async(W, H, 1, r, i) for r, i in pins]
        _entries(c, 2, "vrt_dispatch_async, no wait")
        for t in tickets:
            c.dispatch_wait(t)
        for r, i in pins:
            _same((r, i), ref, "vrt_dispatch_async")
    finally:
        c.set_profiling(0)
        for r, i in pins:
            c.host_free(r)
            c.host_free(i)


def _rays(sc, n, seed=11):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = (np.asarray(sc["pos"], np.float32) + rng.uniform(-0.25, 0.25, size=(n, 3))).astype(np.float32)
    return o, d


class RayBufs:
    def __init__(self, T, o, d):
        t = T.torch
        self.t = t
        n = d.shape[0]
        self.n = n
        self.o, self.d = t.from_numpy(o).cuda(), t.from_numpy(d).cuda()
        self.rgba, self.idd = t.zeros(n, dtype=t.int32, device="cuda"), t.zeros(n * 2, dtype=t.int32, device="cuda")
        self.rgb, self.sums = t.zeros(n * 3, dtype=t.float32, device="cuda"), t.zeros(n * 3, dtype=t.float64, device="cuda")

    def zero(self):
        self.t.cuda.synchronize()   # as Bufs.zero(): a fill that overtook the launch before it would leave that launch's sums in place
        for x in (self.rgba, self.idd, self.rgb, self.sums):
            x.zero_()
        self.t.cuda.synchronize()

    def fetch(self):
        self.t.cuda.synchronize()
        return [x.cpu().numpy() for x in (self.rgba, self.idd, self.rgb, self.sums)]

    def plain(self, c, mode, n_samples, width=37):
        return lambda s: c.shade_rays_device(self.n, self.o.data_ptr(), 3, self.d.data_ptr(), self.rgba.data_ptr(), self.idd.data_ptr(), mode=mode,
                                             width=width, first_sample=3, n_samples=n_samples, stream=s)

    def hdr(self, c, mode, n_samples, width=37):
        return lambda s: c.shade_rays_hdr_device(self.n, self.o.data_ptr(), 3, self.d.data_ptr(), self.rgb.data_ptr(), self.rgba.data_ptr(),
                                                 self.idd.data_ptr(), self.sums.data_ptr(), 0, mode=mode, width=width, first_sample=3,
                                                 n_samples=n_samples, tonemap="reinhard", exposure=0.5, stream=s)


@pytest.mark.parametrize("name", ["unit-internal", "world192", "dragon"])
def test_ray_batches_take_one_slot_each_and_keep_their_outputs(V, T, ctx, scenes, name):
    """The four forms of vrt_shade_rays on the traversals 1, 2 and 4, every mode: one launch and one slot per call -- the host forms
    stage the batch through the context's buffers and shade it in one launch (vrt_rays.cpp shade()), whatever its size: 777 rays are
    13 waves --, the same colours, (id, dist), HDR floats and sums profiled or not, the device forms within their brackets."""
    c, sc = ctx, scenes[name]
    _load(c, V, sc)
    o, d = _rays(sc, 777)
    rb = RayBufs(T, o, d)
    for mode in (0, 1, 2):
        for what, fn in (("vrt_shade_rays_device", rb.plain(c, mode, 2)), ("vrt_shade_rays_hdr_device", rb.hdr(c, mode, 2))):
            _check_route(c, T, f"{name} mode {mode} {what} 777 rays x 2 samples", 1, fn, rb.fetch, rb.zero)
        for what, run in (("vrt_shade_rays", lambda: c.shade_rays(o, d, mode, 37, 3, 2)),
                          ("vrt_shade_rays_hdr", lambda: c.shade_rays_hdr(o, d, mode, 37, 3, 2, "reinhard", 0.5))):
            c.set_profiling(0)
            ref = run()
            c.set_profiling(3)
            got = [run() for _ in range(2)][-1]
            _entries(c, 2, f"{name} mode {mode} {what}")
            _same(got, ref, f"{name} mode {mode} {what}")
    c.set_profiling(0)


def test_every_form_of_the_opaque_full_path_tracer_is_one_slot(V, T, ctx, scenes):
    """VRT_OPT_FULL_OPAQUE 0, 1, 5, 6, 7 on an opaque scene seen from empty space: the general kernel, two kernels with a seed buffer
    between them, one kernel at three occupancies -- each one slot, the two-pass form too (one pair spanning both kernels)"""
    c, sc = ctx, scenes["dragon"]
    W, H = sc["W"], sc["H"]
    _load(c, V, sc)
    assert V.tree_is_opaque(sc["tex"])   # what the dispatcher asks before it takes these forms (eye in empty space: the parity suite's pose)
    b = Bufs(T, W, H, 1)
    r0, i0 = b.rgba[0].data_ptr(), b.idd[0].data_ptr()
    ref = None
    for form in (0, 1, 5, 6, 7):
        c.set_option(V.OPT_FULL_OPAQUE, form)
        _check_route(c, T, f"dragon {W}x{H} mode 2 FULL_OPAQUE {form}", 1, lambda s: c.dispatch_rows(W, H, 0, H, 2, r0, i0, s), b.fetch, b.zero)
        out = b.fetch()
        ref = ref or out
        _same(out, ref, f"FULL_OPAQUE {form} against 0")
    c.set_option(V.OPT_FULL_OPAQUE, 6)


def _scheduled_frames(V, sc, W, H, mode, period, profiled, n=7):
    """n launches of one shape under the feedback scheduler on a fresh context -> (hashes per frame, profile entries, workgroups in
    the order, largest split count)"""
    c = V.Context(0)
    try:
        c.upload_octree(sc["tex"], sc["dim"])
        _camera(c, V, sc, W, H)
        c.set_option(V.OPT_MISS_TILES, 0)
        c.set_tile_scheduling(period)
        if profiled:
            c.set_profiling(n)
        hashes, split = [], 0
        for _ in range(n):
            rgba, idd = c.dispatch(W, H, mode)
            hashes.append((V.fnv1a64(rgba), V.fnv1a64(idd)))
            split = max(split, c.sched_split_count())
        ms = _entries(c, n, f"scheduled {W}x{H} mode {mode} period {period}") if profiled else None
        return hashes, ms, c.sched_order().size, split
    finally:
        c.close()


def test_scheduled_launches_take_one_slot_each(V, scenes, golden):
    """Measuring, ordered and heavy-split launches (shapes and launch counts of test_feedback_tile_scheduling_never_changes_pixels and
    test_heaviest_tiles_as_part_tile_waves_never_change_pixels, which show the routes taken the same way: an order of all workgroups
    exists, a split count was read back): seven launches, seven entries -- the order kernel and the split's memset are outside the
    pair and take no slot --, and the frames of a profiled run equal an unprofiled one's."""
    W, H = 1016, 520
    n_wg = (((W + 7) // 8) * ((H + 7) // 8) + 3) // 4
    plain = _scheduled_frames(V, scenes["dragon"], W, H, 0, 2, False)
    prof = _scheduled_frames(V, scenes["dragon"], W, H, 0, 2, True)
    assert plain[2] == n_wg and prof[2] == n_wg
    assert prof[0] == plain[0] and len(set(prof[0])) == 1
    g = golden["frames"]["frames"]["room_inside_720p_full/mode2"]
    W, H = g["width"], g["height"]
    plain = _scheduled_frames(V, scenes["room"], W, H, 2, 3, False)
    prof = _scheduled_frames(V, scenes["room"], W, H, 2, 3, True)
    assert plain[3] > 0 and prof[3] > 0          # the split engaged
    assert prof[0] == plain[0] and len(set(prof[0])) == 1
    assert "%016x" % prof[0][0][0] == g["rgba_fnv1a64"] and "%016x" % prof[0][0][1] == g["id_dist_fnv1a64"]


def test_calls_that_take_no_slot(V, T, ctx, scenes):
    """vrt_accum_add (three modes, plain, HDR, jittered), the display passes, the world queries: after each of them a frame launch
    lands in slot 0, and under a stride of 2 they do not move which launch is timed (launch, call, launch: the first alone)."""
    c, sc = ctx, scenes["dragon"]
    W, H = sc["W"], sc["H"]
    _load(c, V, sc)
    t = T.torch
    b = Bufs(T, W, H, 1)
    r0, i0 = b.rgba[0].data_ptr(), b.idd[0].data_ptr()
    rgba, idd = c.dispatch(W, H, 1)
    d_rgb = t.rand(W * H * 3, dtype=t.float32, device="cuda")
    d_out, d_out_rgb = t.zeros(W * H, dtype=t.int32, device="cuda"), t.zeros(W * H * 3, dtype=t.float32, device="cuda")
    t.cuda.synchronize()
    o, d = _rays(sc, 100)

    def accum(mode, hdr, jitter):
        def run():
            c.accum_begin(W, H, 0, mode, jitter=jitter, hdr=hdr)
            c.accum_add(2)
            c.accum_add(1)
            (c.accum_resolve_hdr if hdr else c.accum_resolve)()
        return run

    calls = [(f"vrt_accum_add mode {m} hdr {h} jitter {j}", accum(m, h, j)) for m in (0, 1, 2) for h in (False, True) for j in (False, True)]
    calls += [("vrt_denoise", lambda: c.denoise_device(W, H, r0, i0, d_out.data_ptr())),
              ("vrt_denoise_host", lambda: c.denoise(rgba, idd)),
              ("vrt_denoise_hdr", lambda: c.denoise_hdr_device(W, H, d_rgb.data_ptr(), i0, d_out_rgb.data_ptr(), d_out.data_ptr())),
              ("vrt_cast_rays", lambda: c.cast_rays(o, d)),
              ("vrt_find_voxels", lambda: c.find_voxels(np.arange(300, dtype=np.int32).reshape(-1, 3)))]
    launch = lambda: c.dispatch_rows(W, H, 0, H, 1, r0, i0)
    for what, call in calls:
        c.set_profiling(4)
        call()
        launch()
        _entries(c, 1, f"{what}, then one frame launch")
        c.set_profiling(4, every=2)
        launch()
        call()
        launch()
        _entries(c, 1, f"launch, {what}, launch under a stride of 2")
    c.set_profiling(0)


def test_miss_mask_build_takes_no_slot(V, scenes):
    """VRT_OPT_MISS_TILES: the second sighting of a view builds its mask (a memset and a kernel before the trace kernel); the frame
    still takes exactly one slot. The view gets a mask: the host restatement of the dispatcher's decision says so."""
    sc = scenes["dragon"]
    W, H = sc["W"], sc["H"]
    c = V.Context(0)
    try:
        c.upload_octree(sc["tex"], sc["dim"])
        c.set_tile_scheduling(0)
        c.set_option(V.OPT_MISS_TILES, 1)
        _camera(c, V, sc)
        for _ in range(160):   # the box list is made once the tree has stood for max(64, records / 512) mask requests
            c.dispatch(W, H, 0)
        ip, iv, cp, _ = V.camera_block((70.5, 58.5, 120.5), -95.0, -8.0, W, H)
        assert V.miss_mask(sc["tex"], ip, iv, cp, W, H) is not None
        c.set_camera(ip, iv, cp)
        c.set_option(V.OPT_MISS_TILES, 0)
        ref = c.dispatch(W, H, 0)
        c.set_option(V.OPT_MISS_TILES, 1)
        for sighting in ("first", "second (builds the mask)", "third (reads it)"):
            c.set_profiling(4)
            got = c.dispatch(W, H, 0)
            _entries(c, 1, f"{sighting} sighting of a view")
            _same(got, ref, f"{sighting} sighting")
    finally:
        c.close()


def test_refused_calls_take_nothing(V, T, ctx, scenes):
    """A bad mode, an open patch batch, no camera: no slot, and prof_seen does not advance -- under a stride of 2, launch, refusal,
    launch times the first launch alone (had the refusal counted, the second would be timed too), and refusal, launch times the launch."""
    c, sc = ctx, scenes["dragon"]
    W, H = sc["W"], sc["H"]
    _load(c, V, sc)
    b = Bufs(T, W, H, 1)
    r0, i0 = b.rgba[0].data_ptr(), b.idd[0].data_ptr()
    o, d = _rays(sc, 100)
    rb = RayBufs(T, o, d)
    launch = lambda: c.dispatch_rows(W, H, 0, H, 0, r0, i0)

    def in_batch(call):
        def run():
            c.patch_begin()
            try:
                call()
            finally:
                c.patch_end()
        return run

    refusals = [("frame, bad mode", lambda: c.dispatch_rows(W, H, 0, H, 7, r0, i0)),
                ("host frame, bad mode", lambda: c.dispatch(W, H, 3)),
                ("frame, open patch batch", in_batch(launch)),
                ("ray batch, bad mode", lambda: rb.plain(c, 5, 1)(None)),
                ("ray batch, open patch batch", in_batch(lambda: rb.hdr(c, 2, 1)(None)))]
    for what, call in refusals:
        c.set_profiling(4, every=2)
        launch()
        with pytest.raises(V.VrtError):
            call()
        launch()
        _entries(c, 1, f"launch, refused call ({what}), launch under a stride of 2")
        c.set_profiling(4, every=2)
        with pytest.raises(V.VrtError):
            call()
        launch()
        _entries(c, 1, f"refused call ({what}), launch under a stride of 2")
        c.set_profiling(4)
        with pytest.raises(V.VrtError):
            call()
        assert len(c.profile_read()) == 0, what
    c.set_profiling(0)
    c2 = V.Context(0)   # no camera yet
    try:
        c2.upload_octree(sc["tex"], sc["dim"])
        c2.set_profiling(4, every=2)
        with pytest.raises(V.VrtError, match="no camera"):
            c2.dispatch(W, H, 0)
        _camera(c2, V, sc)
        c2.dispatch(W, H, 0)
        _entries(c2, 1, "no camera, then a launch under a stride of 2")
    finally:
        c2.close()


def test_bookkeeping(V, T, ctx, scenes):
    c, sc = ctx, scenes["dragon"]
    W, H = sc["W"], sc["H"]
    _load(c, V, sc)
    b = Bufs(T, W, H, 1)
    r0, i0 = b.rgba[0].data_ptr(), b.idd[0].data_ptr()
    L, h = c._L, c._h

    def launches(n):
        for _ in range(n):
            c.dispatch_rows(W, H, 0, H, 0, r0, i0)

    c.set_profiling(8)          # a context that has asked for more slots before
    launches(8)
    _entries(c, 8, "8 of 8")
    c.set_profiling(3)
    launches(5)
    _entries(c, 3, "set_profiling(3), 5 launches")
    c.set_profiling(3)
    launches(3)
    ms = c.profile_read(cap=2)  # today's behaviour: the read empties the record, what does not fit is dropped
    assert len(ms) == 2 and len(c.profile_read()) == 0
    c.set_profiling(0)
    launches(2)
    assert len(c.profile_read()) == 0
    c.set_profiling(8, every=3)
    launches(7)                 # launches 0, 3, 6
    _entries(c, 3, "every=3, 7 launches")
    assert L.vrt_set_profiling(h, 8) == 0   # the stride of the call before persists
    launches(7)
    _entries(c, 3, "the stride persists")
    c.set_profiling(2, every=2)
    launches(7)                 # 0, 2 -- and no more than the two slots
    _entries(c, 2, "every=2, two slots")
    c.set_profiling(0, every=1)
    import ctypes as C
    out = (C.c_float * 4)()
    assert L.vrt_set_profiling_stride(h, 0) == E_INVALID
    assert L.vrt_profile_read(h, None, 4) == E_INVALID
    assert L.vrt_profile_read(h, out, -1) == E_INVALID
    timed = lambda row0, row1, iters, ms: L.vrt_dispatch_timed(h, W, H, row0, row1, 0, r0, i0, None, iters, ms)
    assert timed(0, H, 0, out) == E_INVALID
    assert timed(0, H, 2, None) == E_INVALID
    assert timed(5, 5, 2, out) == E_INVALID and timed(6, 5, 2, out) == E_INVALID
    assert timed(0, H, 2, out) == 0 and out[0] > 0 and out[1] > 0


def _brackets_each(T, steps):
    ev = [T.bracket(fn) for fn in steps]
    T.s.synchronize()
    return np.array([a.elapsed_time(z) for a, z in ev], np.float64)


@pytest.fixture(scope="module")
def contrast(V, T, ctx, scenes):
    """H: mode 2 on the room at 256 x 144 under the explicit-AABB kernels (variant 1, 4 ms; under the default kernels a mode-2 frame of
    the room is as long as its longest wave, 0.9 ms at every size, and one 8 x 8 tile of it 0.04 ms). L: mode 0, one 8 x 8 tile, or a
    one-wave ray batch, under the default kernels. The brackets must differ by 20 times or the contrasts could pass vacuously."""
    c, sc = ctx, scenes["room"]
    _load(c, V, sc)
    b = Bufs(T, 256, 144, 1)
    r0, i0 = b.rgba[0].data_ptr(), b.idd[0].data_ptr()
    o, d = _rays(sc, 64)
    rb = RayBufs(T, o, d)
    shade = rb.plain(c, 0, 1, width=8)

    def heavy(s):
        c.set_variant(1)
        c.dispatch_rows(256, 144, 0, 144, 2, r0, i0, s)

    def light_frame(s):
        c.set_variant(0)
        c.dispatch_rows(8, 8, 0, 8, 0, r0, i0, s)

    def light_rays(s):
        c.set_variant(0)
        shade(s)

    light = {"frame": light_frame, "rays": light_rays}
    for fn in (heavy, light_frame, light_rays):
        for _ in range(WARM):
            fn(T.s.cuda_stream)
    bl = max(float(np.median(T.brackets(fn))) for fn in light.values())
    bh = float(np.median(T.brackets(heavy)))
    _log(f"contrast: H = room mode 2 256x144 variant 1, bracket {bh:.6f}; L brackets at most {bl:.6f}; ratio {bh / bl:.1f}")
    assert bh >= 20.0 * bl, f"H's bracket {bh} is not 20 times L's {bl}"
    return dict(heavy=heavy, light=light, keep=(b, rb))


@pytest.mark.parametrize("kind", ["frame", "rays"])
def test_each_entry_belongs_to_its_launch(V, T, ctx, scenes, contrast, kind):
    """H L H L H L on one context (L a frame launch, then a ray batch: they share the slots): every=1, every H entry above every L
    entry; every=2, H's alone; every=2 one launch later (L H L H L H), L's alone. Then a refusal in the sequence under every=2."""
    c = ctx
    _load(c, V, scenes["room"])
    Hh, Ll = contrast["heavy"], contrast["light"][kind]
    s = T.s.cuda_stream
    keep = contrast["keep"][0]
    c.set_profiling(6)
    _brackets_each(T, [Hh, Ll] * 3)
    ms = _entries(c, 6, "H L H L H L")
    _log(f"contrast ({kind}): H entries {ms[0::2].min():.6f}..{ms[0::2].max():.6f}, L entries {ms[1::2].min():.6f}..{ms[1::2].max():.6f}")
    assert ms[0::2].min() > ms[1::2].max(), ms
    h_min, l_max = ms[0::2].min(), ms[1::2].max()
    c.set_profiling(3, every=2)
    _brackets_each(T, [Hh, Ll] * 3)
    ms = _entries(c, 3, "H L H L H L, every=2")
    assert ms.min() > l_max, ms            # all H's
    c.set_profiling(3, every=2)
    _brackets_each(T, [Ll, Hh] * 3)
    ms = _entries(c, 3, "L H L H L H, every=2")
    assert ms.max() < h_min, ms            # all L's
    c.set_profiling(3, every=2)            # a refusal between two launches does not change which of them is timed
    Hh(s)
    with pytest.raises(V.VrtError):
        c.dispatch_rows(8, 8, 0, 8, 9, keep.rgba[0].data_ptr(), keep.idd[0].data_ptr(), s)
    Ll(s)
    Hh(s)
    ms = _entries(c, 2, "H refusal L H, every=2")
    assert ms.min() > l_max, ms
    c.set_profiling(0)


def test_a_slot_never_reports_an_earlier_launch(V, T, ctx, scenes, contrast):
    """The stale-slot form of a dropped event pair: six H launches profiled and read, then vrt_set_profiling again and mode-2 launches
    of the unit-internal stream and the [-64, 192)^3 world at 64 x 48 (the record-array fallbacks of trace_full) into the same slots:
    every entry is below the smallest H entry (4 ms; the [-64, 192)^3 world's own frame takes 1.2 ms) -- not H's time read again."""
    c = ctx
    _load(c, V, scenes["room"])
    c.set_profiling(6)
    _brackets_each(T, [contrast["heavy"]] * 6)
    h_min = _entries(c, 6, "six H launches").min()
    b = Bufs(T, 64, 48, 1)
    r0, i0 = b.rgba[0].data_ptr(), b.idd[0].data_ptr()
    for name in ("unit-internal", "world192"):
        _load(c, V, scenes[name], 64, 48)
        c.set_profiling(6)
        for _ in range(3):
            c.dispatch_rows(64, 48, 0, 48, 2, r0, i0, T.s.cuda_stream)
        ms = _entries(c, 3, f"{name} mode 2 after six H launches")
        _log(f"stale slots: {name} 64x48 mode 2 entries {ms.min():.6f}..{ms.max():.6f}, smallest H entry {h_min:.6f}")
        assert ms.max() < h_min, (name, ms, h_min)
    c.set_profiling(0)


def test_dispatch_timed_against_the_profiler_and_the_brackets(V, T, ctx, scenes):
    """vrt_dispatch_timed(iters=3) with profiling on, inside the test's bracket: sum(ms_out) <= outer bracket + B (its event pairs lie
    inside the test's), prof[i] <= ms_out[i] + B (the packet lies inside its pair)."""
    c, sc = ctx, scenes["room"]
    W, H = sc["W"], sc["H"]
    _load(c, V, sc)
    b = Bufs(T, W, H, 1)
    r0, i0 = b.rgba[0].data_ptr(), b.idd[0].data_ptr()
    for mode in (0, 2):
        got = []
        fn = lambda s: got.append(c.dispatch_timed(W, H, 0, H, mode, r0, i0, 3, s))
        for _ in range(WARM):
            fn(T.s.cuda_stream)
        got.clear()
        br, pr = _timed(c, T, fn, 3)
        ms = np.array(got, np.float64)
        assert ms.shape == (REPS, 3) and np.all(ms > 0)
        _log(f"vrt_dispatch_timed room {W}x{H} mode {mode} iters 3: outer bracket {np.median(br):.6f}, sum(ms_out) {np.median(ms.sum(axis=1)):.6f}, "
             f"ms_out {np.median(ms, axis=0)}, profiler {np.median(pr, axis=0)}")
        assert np.median(br - ms.sum(axis=1)) >= -T.B
        assert np.all(np.median(ms - pr, axis=0) >= -T.B)


SIZES = ((256, 144), (640, 360), (1280, 720), (1920, 1080))
SPANS = {   # route -> (scene, variant, VRT_OPT_FULL_OPAQUE, views)
    "general kernel (room)": ("room", 0, 6, 1),
    "two kernels and a seed buffer (FULL_OPAQUE 1)": ("dragon", 0, 1, 1),
    "one opaque kernel, 5 waves": ("dragon", 0, 5, 1),
    "one opaque kernel, 6 waves": ("dragon", 0, 6, 1),
    "one opaque kernel, 7 waves": ("dragon", 0, 7, 1),
    "general kernel on an opaque scene (FULL_OPAQUE 0)": ("dragon", 0, 0, 1),
    "trav 3 (variant 20)": ("room", 20, 6, 1),
    "trav 2 (variant 4)": ("room", 4, 6, 1),
    "trav 1 (variant 1)": ("room", 1, 6, 1),
    "four views": ("room", 0, 6, 4),
}


def _span(c, T, what, ladder):
    """ladder: (label, fn) from the smallest launch up; the first that lasts 10 B by the bracket is the one checked"""
    for label, fn in ladder:
        for _ in range(WARM):
            fn(T.s.cuda_stream)
        br, pr = _timed(c, T, fn)
        mb = float(np.median(br))
        if mb >= 10.0 * T.B:
            break
    d = float(np.median(br - pr[:, 0]))
    _log(f"span {what} [{label}]: bracket {mb:.6f} profiler {np.median(pr):.6f} difference {d:.6f} = {d / T.B:.2f} B")
    assert mb >= 10.0 * T.B, f"{what}: no launch of the ladder lasts 10 B ({mb} against B {T.B})"
    assert d >= -T.B, f"{what}: the profiler's time exceeds the bracket by {-d}"
    assert d <= 3.0 * T.B, f"{what}: {d} ms of the bracket ({d / T.B:.2f} B) are outside the profiler's span"


@pytest.mark.parametrize("what", list(SPANS))
def test_nothing_is_left_out_of_the_timed_span_of_a_full_frame(V, T, ctx, scenes, what):
    """Mode 2, every form: bracket - prof <= 3 B for a launch of at least 10 B. For the two-pass form this is what catches a span
    that starts at pass 2 or ends at pass 1."""
    name, variant, form, n_views = SPANS[what]
    c, sc = ctx, scenes[name]
    _load(c, V, sc)
    c.set_variant(variant)
    c.set_option(V.OPT_FULL_OPAQUE, form)
    b = Bufs(T, SIZES[-1][0], SIZES[-1][1], n_views)
    r0, i0 = b.rgba[0].data_ptr(), b.idd[0].data_ptr()
    ladder = []
    for W, H in SIZES:
        if n_views == 1:
            def fn(s, W=W, H=H, cam=V.camera_block(sc["pos"], sc["yaw"], sc["pitch"], W, H)[:3]):
                c.set_camera(*cam)
                c.dispatch_rows(W, H, 0, H, 2, r0, i0, s)
        else:
            def fn(s, W=W, H=H, views=b.views(c, V, sc, W, H, n_views)):
                c.dispatch_views(W, H, H, 0, 1, 2, views, s)
        ladder.append((f"{W}x{H}", fn))
    try:
        _span(c, T, what, ladder)
    finally:
        _plain(c, V)


@pytest.mark.parametrize("hdr", [False, True])
def test_nothing_is_left_out_of_the_timed_span_of_a_ray_batch(V, T, ctx, scenes, hdr):
    """vrt_shade_rays_device / vrt_shade_rays_hdr_device, mode 2, 4099 rays, samples per ray raised until the launch lasts 10 B"""
    c, sc = ctx, scenes["room"]
    _load(c, V, sc)
    o, d = _rays(sc, 4099)
    rb = RayBufs(T, o, d)
    ladder = [(f"{n} samples", (rb.hdr if hdr else rb.plain)(c, 2, n, width=64)) for n in (8, 64, 512, 4096)]
    _span(c, T, "vrt_shade_rays_hdr_device" if hdr else "vrt_shade_rays_device", ladder)
