"""Auto-exposure on the MI355X (vrt_meter_hdr, vrt_tonemap_hdr, vrt_accum_resolve_hdr_metered and their host and device forms)
against the checker (tests/oracle_meter.c), bit for bit on the histogram, the record and the bytes: the smallest frames, every head
and tail length of the histogram's vector loop, rectangles with odd corners, a frame of more pixels than one pass of the capped grid
covers, a constant image, an image that fills all 256 bins with NaN, infinities, negatives and values on both sides of every bin edge,
the same call twice and on two streams, a dirty workspace, the record chained on the device over eight frames, the tone map without a
record against vrt_accum_resolve_hdr and with one against E9, the accumulation forms against the chain by hand, the accumulation's
other resolves untouched, and the error codes."""
import ctypes as C

import numpy as np
import pytest

import guide_worlds as GW
import oracle_meter as M
from test_meter import nasty_pixels

pytestmark = pytest.mark.gpu

f32 = np.float32
MODE_FULL = 2
FIRST, N = GW.FIRST, 2
# The histogram pass runs at most 512 workgroups of 256 lanes, four pixels a lane (csrc/vrt_meter.hip.h kMaxBlocks, kBlock): one
# pass of the capped grid covers 512 * 256 * 4 = 524,288 pixels. 1024 x 768 = 786,432 takes a second trip of the grid-stride loop.
ONE_PASS = 512 * 256 * 4
BIG = (1024, 768)


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return M.build(tmp_path_factory.mktemp("oracle_meter"))


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def image(seed, h, w, lo=-14.0, hi=12.0):
    """luminances over 26 octaves"""
    rng = np.random.default_rng(seed)
    return (2.0 ** rng.uniform(lo, hi, (h, w, 3))).astype(f32)


@pytest.fixture(scope="module")
def big():
    """the large frame and the checker's histogram of it, computed once"""
    assert BIG[0] * BIG[1] > ONE_PASS
    return image(1, BIG[1], BIG[0])


def same_record(got, want, what):
    assert M.bits(got) == M.bits(want), f"{what}: {got} != {want}"


def check_host(ctx, L, rgb, m, what, state=None):
    want, want_hist = M.meter(L, rgb, m, state)
    got, hist = ctx.meter_hdr(rgb, M.keys(m), state)
    assert np.array_equal(hist, want_hist), f"{what}: histogram"
    same_record(got, want, what)
    return want, want_hist


def device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def workspace(torch, state=None, fill=0):
    """-> (histogram int32[256] filled with `fill`, the record as int32[4])"""
    e = M.from_record(state)
    return (torch.full((M.BINS,), fill, dtype=torch.int32, device="cuda:0"),
            device(torch, np.frombuffer(bytes(e), np.int32).copy()))


def read_record(t):
    return M.record(M.Exposure.from_buffer_copy(t.cpu().numpy().tobytes()))


def read_hist(t):
    return t.cpu().numpy().view(np.uint32)


# ---- the histogram pass and the finishing step ----

@pytest.mark.parametrize("size", [(1, 1), (3, 1), (67, 33), (1, 9), (257, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_frames_are_the_checkers(ctx, L, size):
    w, h = size
    rgb = image(w * 100 + h, h, w)
    for m in (M.make(), M.make(low=0, high=1000, adapt=0.5), M.make(key=0.5, low=10, high=20)):
        first, _ = check_host(ctx, L, rgb, m, f"{size}")
        check_host(ctx, L, rgb[::-1].copy(), m, f"{size}: second frame", first)


def test_every_head_and_tail_of_the_vector_loop(ctx, L):
    """the device form on pointers 0, 4, 8 and 12 bytes past a multiple of 16 -- the first whole quad starts 0, 1, 2 or 3 pixels in --
    with 1 to 9 pixels and 263, so that every tail length follows every head length, with and without whole quads between them"""
    import torch
    src = image(7, 1, 300)
    buf = torch.zeros(4 + 300 * 3, dtype=torch.float32, device="cuda:0")
    m = M.make(low=0, high=1000)
    for shift in range(4):
        buf.zero_()
        buf[shift:shift + 900] = device(torch, src.ravel())
        for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 263):
            hist, rec = workspace(torch)
            torch.cuda.synchronize()
            ctx.meter_hdr_device(n, 1, buf.data_ptr() + 4 * shift, hist.data_ptr(), rec.data_ptr(), M.keys(m))
            ctx.synchronize()
            want, want_hist = M.meter(L, src[:, :n], m)
            assert np.array_equal(read_hist(hist), want_hist), (shift, n)
            same_record(read_record(rec), want, f"shift {shift}, {n} pixels")


@pytest.mark.parametrize("rect", [(5, 3, 64, 30), (0, 7, 67, 8), (0, 0, 67, 33), (66, 32, 67, 33), (1, 0, 2, 33), (0, 0, 1, 1), (3, 2, 66, 3),
                                  (0, 5, 67, 33)], ids=str)
def test_rectangles_with_odd_corners(ctx, L, rect):
    rgb = image(9, 33, 67)
    for m in (M.make(low=0, high=1000, rect=rect), M.make(rect=rect)):
        _, hist = check_host(ctx, L, rgb, m, f"{rect}")
    assert hist.sum() == (rect[2] - rect[0]) * (rect[3] - rect[1])


def test_a_frame_of_more_pixels_than_one_pass_of_the_capped_grid(ctx, L, big):
    _, hist = check_host(ctx, L, big, M.make(), "1024 x 768")
    assert hist.sum() == BIG[0] * BIG[1] > ONE_PASS
    # ... and a rectangle of it: 700 rows of 901 pixels, more rows than the grid has workgroups for
    check_host(ctx, L, big, M.make(rect=(61, 33, 962, 733)), "a rectangle of 1024 x 768")


def test_a_constant_image_puts_every_lane_into_one_bin(ctx, L):
    w, h = BIG
    rgb = np.empty((h, w, 3), f32)
    rgb[:] = (0.6, 0.7, 1.0)   # sky
    want, hist = check_host(ctx, L, rgb, M.make(), "sky")
    assert np.count_nonzero(hist) == 1 and hist.max() == w * h and want["window"] == w * h * 950 // 1000 - w * h * 500 // 1000
    rgb[:] = 0.0
    want, hist = check_host(ctx, L, rgb, M.make(), "black")
    assert hist[0] == w * h and want["window"] == 0 and want["exposure"] == 1.0


def test_every_bin_and_every_kind_of_bad_channel(ctx, L):
    px = nasty_pixels()
    rgb = px[:len(px) // 7 * 7].reshape(7, -1, 3).copy()
    _, hist = check_host(ctx, L, rgb, M.make(low=0, high=1000), "nasty pixels")
    assert np.count_nonzero(hist) == 256
    check_host(ctx, L, rgb, M.make(low=3, high=997, rect=(2, 1, rgb.shape[1] - 3, 6)), "nasty pixels, a rectangle")


def test_twice_and_on_two_streams_with_two_workspaces(ctx, L, big):
    import torch
    w, h = BIG
    d = device(torch, big)
    m = M.make(adapt=0.5)
    state = {"exposure": 2.0, "metered": 1.0, "window": 1, "frames": 3}
    want, want_hist = M.meter(L, big, m, state)
    a, b = workspace(torch, state), workspace(torch, state)
    s1, s2 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    ctx.meter_hdr_device(w, h, d.data_ptr(), a[0].data_ptr(), a[1].data_ptr(), M.keys(m), stream=s1.cuda_stream)
    ctx.meter_hdr_device(w, h, d.data_ptr(), b[0].data_ptr(), b[1].data_ptr(), M.keys(m), stream=s2.cuda_stream)
    torch.cuda.synchronize()
    for hist, rec in (a, b):
        assert np.array_equal(read_hist(hist), want_hist)
        same_record(read_record(rec), want, "two streams")
    # the same call again on the context's stream, the record reset: identical bits
    c = workspace(torch, state)
    for _ in range(2):
        c[1].copy_(workspace(torch, state)[1])
        torch.cuda.synchronize()
        ctx.meter_hdr_device(w, h, d.data_ptr(), c[0].data_ptr(), c[1].data_ptr(), M.keys(m))
        ctx.synchronize()
        assert np.array_equal(read_hist(c[0]), want_hist)
        same_record(read_record(c[1]), want, "the same call twice")


def test_a_dirty_workspace_is_zeroed_by_the_call(ctx, L):
    import torch
    rgb = image(4, 33, 67)
    hist, rec = workspace(torch, fill=-1)
    torch.cuda.synchronize()
    ctx.meter_hdr_device(67, 33, device(torch, rgb).data_ptr(), hist.data_ptr(), rec.data_ptr())
    ctx.synchronize()
    want, want_hist = M.meter(L, rgb, M.make())
    assert np.array_equal(read_hist(hist), want_hist)
    same_record(read_record(rec), want, "dirty workspace")


def test_the_device_record_chained_over_eight_frames(ctx, V, L):
    """adapt 0.25, the record never read by the host between the frames; equal to vrt_meter_resolve chained on the host"""
    import torch
    w, h = 67, 33
    frames = [image(20 + k, h, w, lo=-10.0 + 3 * (k % 3), hi=-4.0 + 3 * (k % 3)) for k in range(8)]
    frames[5][:] = 0.0   # a black frame keeps the exposure
    m = M.make(adapt=0.25)
    d = [device(torch, f) for f in frames]
    hists = [workspace(torch)[0] for _ in frames]
    rec = workspace(torch)[1]
    torch.cuda.synchronize()
    for k in range(8):
        ctx.meter_hdr_device(w, h, d[k].data_ptr(), hists[k].data_ptr(), rec.data_ptr(), M.keys(m))
    ctx.synchronize()
    state = want = None
    for k in range(8):
        assert np.array_equal(read_hist(hists[k]), M.histogram(L, frames[k])), k
        state = V.meter_resolve(read_hist(hists[k]), M.keys(m), state)
        want = M.resolve(L, M.histogram(L, frames[k]), m, want)
        same_record(state, want, f"frame {k}")
    same_record(read_record(rec), want, "the device's record after eight frames")
    assert want["frames"] == 8


# ---- the tone map ----

@pytest.fixture(scope="module")
def room(V, ctx):
    """a 64 x 48 HDR accumulation of the room, with moments"""
    w = GW.world(V, "room")
    ctx.upload_octree(*w.flatten())
    w.close()
    ctx.set_params(ctx.default_params())
    ctx.set_camera(*GW.camera(V, "room", (64, 48)))
    ctx.set_lens(0.0, 1.0)
    ctx.accum_begin(64, 48, FIRST, mode=MODE_FULL, hdr=True, moments=True)
    assert ctx.accum_add(N) == N
    return ctx.accum_resolve_hdr()[0]


@pytest.mark.parametrize("tm", [("clamp", 1.0), ("reinhard", 0.8), ("clamp", 3.0), (None, 1.0)], ids=str)
def test_tonemap_without_a_record_is_the_resolves(ctx, room, tm):
    op, e = tm
    want = ctx.accum_resolve_hdr(op or "clamp", e)[1]
    assert np.array_equal(ctx.tonemap_hdr(room, op, e), want)
    assert 0 < want[..., :3].mean() < 255


@pytest.mark.parametrize("op", ["clamp", "reinhard"])
def test_tonemap_with_a_record_is_e9(ctx, L, op):
    import torch
    px = nasty_pixels()
    for e_tm, e_rec in ((1.0, 0.37), (0.5, 6.0), (3e30, 3e30), (1.0, 2.0 ** -10)):
        state = {"exposure": e_rec, "metered": 1.0, "window": 1, "frames": 1}
        assert np.array_equal(ctx.tonemap_hdr(px, op, e_tm, state), M.tonemap(L, px, op, e_tm, state)), (e_tm, e_rec)
    # the device form: every tail of the vector loop, and pointers that send it down the one-pixel form
    state = {"exposure": 0.8, "metered": 1.0, "window": 1, "frames": 1}
    rec = workspace(torch, state)[1]
    src = torch.zeros(4 + 3 * 1100, dtype=torch.float32, device="cuda:0")
    out = torch.zeros(4 + 1100, dtype=torch.int32, device="cuda:0")
    for shift_in, shift_out in ((0, 0), (1, 0), (0, 1), (3, 2)):
        for n in (1, 2, 3, 4, 5, 7, 1024, 1027):
            src.zero_()
            src[shift_in:shift_in + 3 * n] = device(torch, px[:n].ravel())
            out.fill_(-1)
            torch.cuda.synchronize()
            ctx.tonemap_hdr_device(n, src.data_ptr() + 4 * shift_in, out.data_ptr() + 4 * shift_out, rec.data_ptr(), op, 1.5)
            ctx.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got[shift_out:shift_out + n].view(np.uint8).reshape(n, 4), M.tonemap(L, px[:n], op, 1.5, state)), (shift_in, shift_out, n)
            assert (got[:shift_out] == -1).all() and (got[shift_out + n:] == -1).all(), "nothing written outside the n pixels"


def test_tonemap_of_a_large_frame(ctx, L, big):
    state = {"exposure": 0.05, "metered": 1.0, "window": 1, "frames": 1}
    assert np.array_equal(ctx.tonemap_hdr(big, "reinhard", 2.0, state), M.tonemap(L, big, "reinhard", 2.0, state))


# ---- the accumulation forms ----

def test_the_accumulation_forms_are_the_chain_by_hand(ctx, V, L, room):
    import torch
    w, h = 64, 48
    before = ctx.accum_resolve() + ctx.accum_resolve_hdr() + (ctx.accum_variance(),) + tuple(ctx.accum_guides().values())
    m = M.make(low=200, high=900, adapt=0.5, rect=(3, 5, 61, 40))
    state = {"exposure": 4.0, "metered": 0.5, "window": 10, "frames": 2}
    # by hand: resolve_hdr, meter_hdr, tonemap_hdr
    rec_hand, hist_hand = ctx.meter_hdr(room, M.keys(m), state)
    bytes_hand = ctx.tonemap_hdr(room, "reinhard", 0.9, rec_hand)
    want, want_hist = M.meter(L, room, m, state)
    same_record(rec_hand, want, "by hand")
    assert np.array_equal(hist_hand, want_hist) and np.array_equal(bytes_hand, M.tonemap(L, room, "reinhard", 0.9, want))
    # the host form
    rec, rgb, rgba, hist = ctx.accum_resolve_hdr_metered(M.keys(m), "reinhard", 0.9, state)
    same_record(rec, want, "the host form")
    assert np.array_equal(rgb.view(np.uint32), room.view(np.uint32)) and np.array_equal(rgba, bytes_hand) and np.array_equal(hist, want_hist)
    # the device form on a caller's stream, every optional output given and then none
    side = torch.cuda.Stream(device="cuda:0")
    for given in (True, False):
        d_hist, d_rec = workspace(torch, state, fill=-1)
        d_rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        d_rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        opt = [t.data_ptr() if given else None for t in (d_hist, d_rgb, d_rgba)]
        ctx.accum_resolve_hdr_metered_device(d_rec.data_ptr(), *opt, M.keys(m), "reinhard", 0.9, stream=side.cuda_stream)
        ctx.synchronize()
        torch.cuda.synchronize()
        same_record(read_record(d_rec), want, f"the device form, outputs {given}")
        if given:
            assert np.array_equal(read_hist(d_hist), want_hist) and np.array_equal(d_rgba.cpu().numpy(), bytes_hand)
            assert np.array_equal(d_rgb.cpu().numpy().view(np.uint32), room.view(np.uint32))
        else:
            assert (d_hist == -1).all() and not d_rgb.any() and not d_rgba.any()
    # a NULL vrt_meter and a NULL vrt_tonemap are the defaults; the first frame of a record
    rec, _, rgba, hist = ctx.accum_resolve_hdr_metered(None, None)
    want, want_hist = M.meter(L, room, M.make())
    same_record(rec, want, "defaults")
    assert np.array_equal(hist, want_hist) and np.array_equal(rgba, M.tonemap(L, room, None, 1.0, want))
    after = ctx.accum_resolve() + ctx.accum_resolve_hdr() + (ctx.accum_variance(),) + tuple(ctx.accum_guides().values())
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the accumulation's other resolves, variance and guides are unchanged"
    assert ctx.accum_add(1) == N + 1                              # ... and the sums go on
    assert not np.array_equal(ctx.accum_resolve_hdr()[0], room)


def _fresh(V, size=(40, 24)):
    """a context of its own with the room loaded and a camera set"""
    w = GW.world(V, "room")
    c = V.Context(0)
    c.upload_octree(*w.flatten())
    w.close()
    c.set_params(c.default_params())
    c.set_camera(*GW.camera(V, "room", size))
    return c


def test_an_adaptive_accumulations_counts_are_unchanged(V):
    c = _fresh(V, (43, 21))
    try:
        c.accum_begin(43, 21, 0, adaptive=(2, 6, 3), hdr=True)
        c.accum_add(4)
        counts = c.accum_counts()
        c.accum_resolve_hdr_metered()
        again = c.accum_counts()
        assert np.array_equal(counts[0], again[0]) and counts[1] == again[1]
    finally:
        c.close()


# ---- what is refused ----

def test_invalid_arguments(ctx, V):
    import torch
    lib = V.hip_lib()
    w, h = 16, 8
    rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    out = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
    hist, rec = workspace(torch)
    P = dict(rgb=rgb.data_ptr(), hist=hist.data_ptr(), rec=rec.data_ptr(), out=out.data_ptr())
    torch.cuda.synchronize()

    def meter(size=(w, h), rgb=P["rgb"], hist=P["hist"], rec=P["rec"], **kw):
        m = M.make(**kw)
        return lib.vrt_meter_hdr(ctx._h, size[0], size[1], rgb, C.byref(V.Meter.from_buffer_copy(bytes(m))), hist, rec, None)

    assert meter() == 0
    nan, inf = float("nan"), float("inf")
    assert meter(rgb=None) == -1 and meter(hist=None) == -1 and meter(rec=None) == -1
    assert meter(hist=P["rgb"]) == -1 and meter(rec=P["rgb"]) == -1 and meter(hist=P["rec"]) == -1       # aliases
    assert meter(rgb=P["rgb"] + 2) == -1 and meter(hist=P["hist"] + 1) == -1 and meter(rec=P["rec"] + 3) == -1   # no multiple of 4
    assert meter(size=(0, h)) == -1 and meter(size=(w, -1)) == -1 and meter(size=(1 << 16, 1 << 15)) == -1
    for rect in ((0, 0, w + 1, h), (0, 0, w, h + 1), (-1, 0, w, h), (4, 0, 4, h), (5, 0, 4, h), (0, 3, w, 3), (0, 0, 0, h), (0, 0, w, 0), (1, 1, 0, 0)):
        assert meter(rect=rect) == -1, rect
    assert meter(rect=(0, 0, w, h)) == 0 and meter(rect=(w - 1, h - 1, w, h)) == 0
    for kw in (dict(key=0.0), dict(key=nan), dict(key=inf), dict(low=-1), dict(low=500, high=500), dict(high=1001), dict(min_exposure=0.0),
               dict(min_exposure=nan), dict(max_exposure=inf), dict(min_exposure=2.0, max_exposure=1.0), dict(adapt=0.0), dict(adapt=1.5), dict(adapt=nan)):
        assert meter(**kw) == -1, kw
    assert b"adapt must be in (0, 1]" in lib.vrt_last_error(ctx._h)
    assert lib.vrt_meter_hdr(None, w, h, P["rgb"], None, P["hist"], P["rec"], None) == -1
    assert lib.vrt_meter_hdr(ctx._h, w, h, P["rgb"], None, P["hist"], P["rec"], None) == 0                 # a NULL vrt_meter: the default
    host = np.zeros((h, w, 3), f32)
    e = V.Exposure()
    assert lib.vrt_meter_hdr_host(ctx._h, w, h, None, None, None, C.byref(e)) == -1
    assert lib.vrt_meter_hdr_host(ctx._h, w, h, host.ctypes.data, None, None, None) == -1
    assert lib.vrt_meter_hdr_host(ctx._h, w, h, host.ctypes.data, None, None, C.byref(e)) == 0 and e.frames == 1   # no histogram asked for

    def tone(n=w * h, rgb=P["rgb"], out=P["out"], rec=P["rec"], op=0, e=1.0):
        return lib.vrt_tonemap_hdr(ctx._h, n, rgb, C.byref(V.Tonemap(op, e)), rec, out, None)

    assert tone() == 0 and tone(rec=None) == 0
    assert tone(rgb=None) == -1 and tone(out=None) == -1 and tone(n=0) == -1 and tone(n=(1 << 30) + 1) == -1
    assert tone(out=P["rgb"]) == -1 and tone(out=P["rec"]) == -1 and tone(rgb=P["rgb"] + 1) == -1 and tone(out=P["out"] + 2) == -1
    assert tone(op=2) == -1 and tone(e=0.0) == -1 and tone(e=nan) == -1 and tone(e=inf) == -1
    assert lib.vrt_tonemap_hdr(None, 4, P["rgb"], None, None, P["out"], None) == -1
    out8 = np.zeros((h, w, 4), np.uint8)
    assert lib.vrt_tonemap_hdr_host(ctx._h, w * h, None, None, None, out8.ctypes.data) == -1
    assert lib.vrt_tonemap_hdr_host(ctx._h, w * h, host.ctypes.data, None, None, None) == -1
    assert lib.vrt_tonemap_hdr_host(ctx._h, 0, host.ctypes.data, None, None, out8.ctypes.data) == -1
    assert lib.vrt_tonemap_hdr_host(ctx._h, w * h, host.ctypes.data, None, None, out8.ctypes.data) == 0


@pytest.mark.parametrize("form", ["host", "device"])
def test_state_errors_of_the_accumulation_forms(V, form):
    import torch
    c = _fresh(V)
    try:
        d_rec = workspace(torch)[1]
        torch.cuda.synchronize()
        call = (lambda: c.accum_resolve_hdr_metered()) if form == "host" else (lambda: c.accum_resolve_hdr_metered_device(d_rec.data_ptr(), None, None, None))
        with pytest.raises(V.VrtError, match="vrt error -5"):               # no begin
            call()
        c.accum_begin(40, 24, FIRST, hdr=True)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # no sample
            call()
        c.accum_begin(40, 24, FIRST)
        c.accum_add(1)
        with pytest.raises(V.VrtError, match="vrt error -5"):               # without HDR
            call()
        c.accum_begin(40, 24, FIRST, hdr=True)
        c.accum_add(1)
        call()
        c.synchronize()
        lib = V.hip_lib()
        assert lib.vrt_accum_resolve_hdr_metered(c._h, None, None, None, None, None, None) == -1          # no record
        assert lib.vrt_accum_resolve_hdr_metered_device(c._h, None, None, None, None, None, None, None) == -1
        p = d_rec.data_ptr()
        assert lib.vrt_accum_resolve_hdr_metered_device(c._h, None, None, p, p, None, None, None) == -1       # record and histogram in one place
        assert lib.vrt_accum_resolve_hdr_metered_device(c._h, None, None, p + 2, None, None, None, None) == -1
        with pytest.raises(V.VrtError, match="vrt error -1"):
            c.accum_resolve_hdr_metered({"x0": 0, "y0": 0, "x1": 41, "y1": 24})                               # a rectangle outside the frame
        assert lib.vrt_accum_resolve_hdr_metered(c._h, None, C.byref(V.Tonemap(7, 1.0)), C.byref(V.Exposure()), None, None, None) == -1
        assert lib.vrt_accum_resolve_hdr_metered(None, None, None, None, None, None, None) == -1
    finally:
        c.close()
