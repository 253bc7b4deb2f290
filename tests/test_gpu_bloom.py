"""Bloom on the MI355X (vrt_bloom_hdr, its host form, vrt_accum_resolve_hdr_bloomed and its device twin) against the checker
(tests/oracle_bloom.c), bit for bit on f and on the bytes: the smallest frames at every depth of the pyramid with and without KARIS,
frames on both sides of every tile edge of the down-sampling kernel, a large frame, input pointers at every offset inside 16 bytes,
NaN, infinities and negatives, a workspace full of NaN and guarded outputs, the same call twice and on two streams, a record chained
on the device from vrt_meter_hdr, the NULL tone map and the NULL record, the accumulation forms against the chain by hand with the
accumulation's other resolves untouched, and the error codes."""
import ctypes as C

import numpy as np
import pytest

import guide_worlds as GW
import oracle_bloom as B
import oracle_meter as M
from test_meter import nasty_pixels

pytestmark = pytest.mark.gpu

f32 = np.float32
MODE_FULL = 2
FIRST, N = GW.FIRST, 2
# The down-sampling kernel gives a workgroup a tile of TX x TY destination pixels (csrc/vrt_bloom.hip.h kTX, kTY), which reads a
# window of 2 TX + 2 by 2 TY + 2 source pixels; the up-sampling kernel tiles its destination the same way.
TX, TY = 32, 8
BIG = (1024, 768)


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return B.build(tmp_path_factory.mktemp("oracle_bloom"))


@pytest.fixture(scope="module")
def LM(tmp_path_factory):
    return M.build(tmp_path_factory.mktemp("oracle_meter"))


@pytest.fixture(scope="module")
def ctx(V):
    c = V.Context(0)
    yield c
    c.close()


def image(seed, h, w, lo=-14.0, hi=12.0):
    """channels over 26 octaves"""
    rng = np.random.default_rng(seed)
    return (2.0 ** rng.uniform(lo, hi, (h, w, 3))).astype(f32)


def state_of(e):
    return None if e is None else {"exposure": e, "metered": 1.0, "window": 1, "frames": 1}


def same(got, want, what):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), f"{what}: f"
    assert np.array_equal(got[1], want[1]), f"{what}: the bytes"


def check_host(ctx, L, rgb, b, what, op="clamp", e=1.0, rec=None):
    want = B.run(L, rgb, b, op, e, state_of(rec))
    same(ctx.bloom_hdr(rgb, B.keys(b), op, e, state_of(rec)), want, what)
    return want


def device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def record_on_device(torch, state=None):
    return device(torch, np.frombuffer(bytes(M.from_record(state)), np.int32).copy())


class Buffers:
    """the device buffers of one call: the workspace between two guards, every word a NaN pattern; f and the bytes between guards too"""
    GUARD = 64          # int32 words on either side
    NAN = 0x7fc0beef    # a quiet NaN with a payload, as an int32

    def __init__(self, torch, w, h, levels):
        self.torch, self.w, self.h = torch, w, h
        self.ws_words = B.workspace_bytes(w, h, levels) // 4
        g = self.GUARD
        self.ws = torch.full((self.ws_words + 2 * g,), self.NAN, dtype=torch.int32, device="cuda:0")
        self.f = torch.full((w * h * 3 + 2 * g,), self.NAN, dtype=torch.int32, device="cuda:0")
        self.rgba = torch.full((w * h + 2 * g,), self.NAN, dtype=torch.int32, device="cuda:0")
        assert (self.ws.data_ptr() + 4 * g) % 16 == 0

    def pointers(self):
        g = 4 * self.GUARD
        return self.ws.data_ptr() + g, self.f.data_ptr() + g, self.rgba.data_ptr() + g

    def result(self):
        """(f, bytes), after checking that nothing was written outside the two outputs and the workspace"""
        g = self.GUARD
        out = []
        for t, n in ((self.f, self.w * self.h * 3), (self.rgba, self.w * self.h), (self.ws, self.ws_words)):
            a = t.cpu().numpy()
            assert (a[:g] == self.NAN).all() and (a[g + n:] == self.NAN).all(), "written outside the buffer"
            out.append(a[g:g + n])
        return out[0].view(f32).reshape(self.h, self.w, 3), out[1].view(np.uint8).reshape(self.h, self.w, 4)


# ---- the pyramid ----

@pytest.mark.parametrize("size", [(1, 1), (2, 1), (3, 1), (1, 9), (67, 33), (257, 5), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_frames_are_the_checkers(ctx, L, size):
    w, h = size
    rgb = image(w * 100 + h, h, w)
    for levels in (1, 2, 5, 8):
        for karis in (False, True):
            b = B.make(levels=levels, karis=karis, threshold=0.5, knee=0.25, intensity=0.6)
            check_host(ctx, L, rgb, b, f"{size}, L {levels}, karis {karis}", "reinhard", 0.9, 0.7)


def test_frames_on_both_sides_of_every_tile_edge(ctx, L):
    """one pixel below, at and one above a multiple of the tile's source footprint (2 TX by 2 TY) in each axis -- the first level's
    last tile is then full, one short, or a single column or row -- and of twice that, where the second level's is"""
    widths = [k * 2 * TX + d for k in (1, 2) for d in (-1, 0, 1)]
    heights = [k * 2 * TY + d for k in (1, 2) for d in (-1, 0, 1)]
    b = B.make(levels=3, karis=True, threshold=0.5, knee=0.5, intensity=1.0)
    for i, w in enumerate(widths):
        for j, h in enumerate(heights):
            check_host(ctx, L, image(i * 10 + j, h, w, -6.0, 6.0), b, f"{w}x{h}")


@pytest.fixture(scope="module")
def big():
    return image(1, BIG[1], BIG[0])


def test_a_large_frame(ctx, L, big):
    check_host(ctx, L, big, B.make(), "1024 x 768", "reinhard", 1.0, 0.05)


def test_every_kind_of_bad_channel(ctx, L):
    px = nasty_pixels()
    rgb = px[:len(px) // 43 * 43].reshape(43, -1, 3).copy()
    for b in (B.make(), B.make(levels=3, karis=False, threshold=0.0, knee=0.0, intensity=65504.0)):
        for op, e, rec in (("clamp", 1.0, None), ("reinhard", 3e30, 3e30), ("clamp", 0.5, 2.0 ** -10)):
            f, _ = check_host(ctx, L, rgb, b, f"nasty pixels, {op}", op, e, rec)
            assert np.isfinite(f).all() and f.min() >= 0 and f.max() == 65504.0


def test_tm_null_and_record_null(ctx, L):
    rgb = image(8, 33, 67, -4.0, 6.0)
    b = B.make()
    want = check_host(ctx, L, rgb, b, "NULL tone map, no record", None, 1.0, None)
    same(want, B.run(L, rgb, b, "clamp", 1.0, None), "the NULL tone map is clamp at exposure 1")
    check_host(ctx, L, rgb, b, "NULL tone map, a record", None, 1.0, 0.3)
    same(ctx.bloom_hdr(rgb), want, "a NULL vrt_bloom is the default")
    assert (want[1][..., :3] == 255).mean() > 0.2 and (want[1][..., :3] < 255).mean() > 0.2


# ---- the device form ----

def test_input_pointers_at_every_offset_inside_16_bytes(ctx, L):
    import torch
    w, h = 67, 33
    rgb = image(7, h, w, -6.0, 6.0)
    b = B.make(levels=3)
    want = B.run(L, rgb, b, "clamp", 1.0, None)
    src = torch.zeros(4 + w * h * 3, dtype=torch.float32, device="cuda:0")
    assert src.data_ptr() % 16 == 0
    for shift in range(4):
        src.zero_()
        src[shift:shift + w * h * 3] = device(torch, rgb.ravel())
        bufs = Buffers(torch, w, h, b.levels)
        torch.cuda.synchronize()
        ws, f, rgba = bufs.pointers()
        ctx.bloom_hdr_device(w, h, src.data_ptr() + 4 * shift, ws, f, rgba, None, B.keys(b))
        ctx.synchronize()
        same(bufs.result(), want, f"{4 * shift} bytes past a multiple of 16")
    # the outputs 4 bytes past one too
    out_f = torch.zeros(4 + w * h * 3, dtype=torch.float32, device="cuda:0")
    out_b = torch.zeros(4 + w * h, dtype=torch.int32, device="cuda:0")
    bufs = Buffers(torch, w, h, b.levels)
    torch.cuda.synchronize()
    ctx.bloom_hdr_device(w, h, src.data_ptr() + 12, bufs.pointers()[0], out_f.data_ptr() + 4, out_b.data_ptr() + 12, None, B.keys(b))
    ctx.synchronize()
    got = (out_f.cpu().numpy()[1:1 + w * h * 3].reshape(h, w, 3), out_b.cpu().numpy()[3:3 + w * h].view(np.uint8).reshape(h, w, 4))
    same(got, want, "outputs past a multiple of 16")
    assert out_f[0] == 0 and not out_f[1 + w * h * 3:].any() and not out_b[:3].any() and not out_b[3 + w * h:].any()


def test_a_workspace_of_nan_and_one_output_at_a_time(ctx, L):
    """the workspace needs no initialising: every word of it a NaN, which any read of an unwritten word would carry into the glow"""
    import torch
    for w, h, levels in ((67, 33, 8), (130, 70, 5), (1, 1, 8), (3, 1, 2)):
        rgb = image(w + h, h, w, -6.0, 6.0)
        b = B.make(levels=levels, threshold=0.25, knee=0.25, intensity=1.0)
        want = B.run(L, rgb, b, "reinhard", 1.0, None)
        d = device(torch, rgb)
        for give_f, give_bytes in ((True, True), (True, False), (False, True)):
            bufs = Buffers(torch, w, h, levels)
            torch.cuda.synchronize()
            ws, f, rgba = bufs.pointers()
            ctx.bloom_hdr_device(w, h, d.data_ptr(), ws, f if give_f else None, rgba if give_bytes else None, None, B.keys(b), "reinhard", 1.0)
            ctx.synchronize()
            got = bufs.result()
            if give_f:
                assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (w, h, levels)
            else:
                assert (got[0].view(np.int32) == Buffers.NAN).all()
            if give_bytes:
                assert np.array_equal(got[1], want[1]), (w, h, levels)
            else:
                assert (got[1].view(np.int32) == Buffers.NAN).all()


def test_twice_and_on_two_streams_with_two_workspaces(ctx, L, big):
    import torch
    w, h = BIG
    d = device(torch, big)
    b = B.make(levels=6)
    state = state_of(0.05)
    want = B.run(L, big, b, "reinhard", 1.0, state)
    rec = record_on_device(torch, state)
    one, two = Buffers(torch, w, h, b.levels), Buffers(torch, w, h, b.levels)
    s1, s2 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    for bufs, s in ((one, s1), (two, s2)):
        ws, f, rgba = bufs.pointers()
        ctx.bloom_hdr_device(w, h, d.data_ptr(), ws, f, rgba, rec.data_ptr(), B.keys(b), "reinhard", 1.0, stream=s.cuda_stream)
    torch.cuda.synchronize()
    same(one.result(), want, "stream 1")
    same(two.result(), want, "stream 2")
    assert M.bits(M.record(M.Exposure.from_buffer_copy(rec.cpu().numpy().tobytes()))) == M.bits(state), "the record is only read"
    # the same call again into the workspace the first call left behind: identical bits
    ws, f, rgba = one.pointers()
    ctx.bloom_hdr_device(w, h, d.data_ptr(), ws, f, rgba, rec.data_ptr(), B.keys(b), "reinhard", 1.0)
    ctx.synchronize()
    same(one.result(), want, "the same call twice")


def test_a_record_chained_on_the_device_from_the_meter(ctx, L, LM):
    """four frames, each metered into one device record (adapt 0.5) and bloomed by it, the host never reading the record between"""
    import torch
    w, h = 67, 33
    frames = [image(30 + k, h, w, lo=-8.0 + 3 * (k % 3), hi=2.0 + 3 * (k % 3)) for k in range(4)]
    m = M.make(adapt=0.5)
    b = B.make(levels=4)
    d = [device(torch, f) for f in frames]
    hist = torch.zeros(M.BINS, dtype=torch.int32, device="cuda:0")
    rec = record_on_device(torch)
    bufs = [Buffers(torch, w, h, b.levels) for _ in frames]
    torch.cuda.synchronize()
    for k in range(4):
        ctx.meter_hdr_device(w, h, d[k].data_ptr(), hist.data_ptr(), rec.data_ptr(), M.keys(m))
        ws, f, rgba = bufs[k].pointers()
        ctx.bloom_hdr_device(w, h, d[k].data_ptr(), ws, f, rgba, rec.data_ptr(), B.keys(b), "reinhard", 0.9)
    ctx.synchronize()
    state, exposures = None, set()
    for k in range(4):
        state, _ = M.meter(LM, frames[k], m, state)
        exposures.add(state["exposure"])
        same(bufs[k].result(), B.run(L, frames[k], b, "reinhard", 0.9, state), f"frame {k}")
    assert len(exposures) == 4 and state["frames"] == 4


# ---- the accumulation forms ----

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


def test_the_accumulation_forms_are_the_chain_by_hand(ctx, L, LM, room):
    import torch
    w, h = 64, 48
    before = ctx.accum_resolve() + ctx.accum_resolve_hdr() + (ctx.accum_variance(),) + tuple(ctx.accum_guides().values())
    m = M.make(low=200, high=900, adapt=0.5, rect=(3, 5, 61, 40))
    b = B.make(levels=4, threshold=0.5, knee=0.25, intensity=0.8)
    state = {"exposure": 4.0, "metered": 0.5, "window": 10, "frames": 2}
    # by hand: resolve_hdr, meter_hdr, bloom_hdr
    rec_hand, _ = ctx.meter_hdr(room, M.keys(m), state)
    hand = ctx.bloom_hdr(room, B.keys(b), "reinhard", 0.9, rec_hand)
    want_rec, _ = M.meter(LM, room, m, state)
    assert M.bits(rec_hand) == M.bits(want_rec)
    same(hand, B.run(L, room, b, "reinhard", 0.9, want_rec), "by hand")
    assert not np.array_equal(hand[0], room), "the room's lamp blooms"
    # the host form
    rec, f, rgba = ctx.accum_resolve_hdr_bloomed(M.keys(m), B.keys(b), "reinhard", 0.9, state)
    assert M.bits(rec) == M.bits(want_rec)
    same((f, rgba), hand, "the host form")
    # ... with io NULL: no metering, no record
    none, f, rgba = ctx.accum_resolve_hdr_bloomed(M.keys(m), B.keys(b), "reinhard", 0.9, metering=False)
    assert none is None
    same((f, rgba), B.run(L, room, b, "reinhard", 0.9, None), "the host form, io NULL")
    # the device form on a caller's stream: with a record, without one, and one output at a time
    side = torch.cuda.Stream(device="cuda:0")
    for metered, give_f, give_bytes in ((True, True, True), (False, True, True), (True, False, True), (True, True, False)):
        d_rec = record_on_device(torch, state)
        d_f = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        d_rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ctx.accum_resolve_hdr_bloomed_device(d_rec.data_ptr() if metered else None, d_f.data_ptr() if give_f else None,
                                             d_rgba.data_ptr() if give_bytes else None, M.keys(m), B.keys(b), "reinhard", 0.9, stream=side.cuda_stream)
        ctx.synchronize()
        torch.cuda.synchronize()
        got_rec = M.record(M.Exposure.from_buffer_copy(d_rec.cpu().numpy().tobytes()))
        assert M.bits(got_rec) == M.bits(want_rec if metered else state), f"the device form, metered {metered}"
        want = hand if metered else B.run(L, room, b, "reinhard", 0.9, None)
        if give_f:
            assert np.array_equal(d_f.cpu().numpy().view(np.uint32), want[0].view(np.uint32)), metered
        else:
            assert not d_f.any()
        if give_bytes:
            assert np.array_equal(d_rgba.cpu().numpy(), want[1]), metered
        else:
            assert not d_rgba.any()
    # a NULL vrt_meter, a NULL vrt_bloom and a NULL vrt_tonemap are the defaults; the first frame of a record
    rec, f, rgba = ctx.accum_resolve_hdr_bloomed(None, None, None)
    want_rec, _ = M.meter(LM, room, M.make())
    assert M.bits(rec) == M.bits(want_rec)
    same((f, rgba), B.run(L, room, B.make(), None, 1.0, want_rec), "defaults")
    after = ctx.accum_resolve() + ctx.accum_resolve_hdr() + (ctx.accum_variance(),) + tuple(ctx.accum_guides().values())
    for x, y in zip(before, after):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "the accumulation's other resolves, variance and guides are unchanged"
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
        c.accum_resolve_hdr_bloomed()
        again = c.accum_counts()
        assert np.array_equal(counts[0], again[0]) and counts[1] == again[1]
    finally:
        c.close()


# ---- what is refused ----

def test_invalid_arguments(ctx, V):
    """every case is refused by the host before any launch"""
    import torch
    lib = V.hip_lib()
    w, h = 16, 8
    rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    f = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    out = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
    ws = torch.zeros(B.workspace_bytes(w, h, 8) // 4 + 4, dtype=torch.int32, device="cuda:0")
    rec = record_on_device(torch, state_of(1.0))
    P = dict(rgb=rgb.data_ptr(), f=f.data_ptr(), out=out.data_ptr(), ws=ws.data_ptr(), rec=rec.data_ptr())
    assert P["ws"] % 16 == 0
    torch.cuda.synchronize()

    def call(size=(w, h), rgb=P["rgb"], ws=P["ws"], f=P["f"], out=P["out"], rec=P["rec"], tm=None, null_bloom=False, **kw):
        b = None if null_bloom else C.byref(V.Bloom.from_buffer_copy(bytes(B.make(**kw))))
        t = None if tm is None else C.byref(V.Tonemap(*tm))
        return lib.vrt_bloom_hdr(ctx._h, size[0], size[1], rgb, b, t, rec, ws, f, out, None)

    assert call() == 0 and call(rec=None) == 0 and call(null_bloom=True) == 0 and call(f=None) == 0 and call(out=None) == 0
    nan, inf = float("nan"), float("inf")
    assert call(rgb=None) == -1 and call(ws=None) == -1 and call(f=None, out=None) == -1                       # NULL required pointers
    assert b"one of the two outputs" in lib.vrt_last_error(ctx._h)
    assert call(ws=P["ws"] + 4) == -1 and call(ws=P["ws"] + 8) == -1                                           # the workspace: a multiple of 16
    assert b"multiple of 16" in lib.vrt_last_error(ctx._h)
    assert call(rgb=P["rgb"] + 2) == -1 and call(f=P["f"] + 1) == -1 and call(out=P["out"] + 3) == -1 and call(rec=P["rec"] + 2) == -1
    assert call(f=P["rgb"]) == -1 and call(out=P["rgb"]) == -1 and call(f=P["rec"]) == -1 and call(out=P["rec"]) == -1   # an output equal to an input
    assert call(f=P["ws"]) == -1 and call(out=P["ws"]) == -1 and call(f=P["out"]) == -1                        # ... the workspace, each other
    assert call(size=(0, h)) == -1 and call(size=(w, -1)) == -1 and call(size=(1 << 16, 1 << 15)) == -1
    for kw in (dict(levels=0), dict(levels=9), dict(levels=-1)):
        assert call(**kw) == -1, kw
    assert b"levels" in lib.vrt_last_error(ctx._h)
    bad = V.Bloom.from_buffer_copy(bytes(B.make()))
    bad.flags = 2
    assert lib.vrt_bloom_hdr(ctx._h, w, h, P["rgb"], C.byref(bad), None, None, P["ws"], P["f"], P["out"], None) == -1
    assert b"unknown flags" in lib.vrt_last_error(ctx._h)
    for kw in (dict(knee=-0.5), dict(threshold=0.25, knee=0.5), dict(threshold=65505.0), dict(threshold=-1.0, knee=0.0), dict(threshold=nan),
               dict(knee=nan), dict(threshold=inf), dict(intensity=-0.5), dict(intensity=nan), dict(intensity=inf), dict(intensity=65505.0)):
        assert call(**kw) == -1, kw
    assert call(threshold=65504.0, knee=65504.0, intensity=65504.0) == 0 and call(threshold=0.0, knee=0.0, intensity=0.0) == 0 and call(levels=8) == 0
    assert call(tm=(2, 1.0)) == -1 and call(tm=(0, 0.0)) == -1 and call(tm=(1, nan)) == -1 and call(tm=(0, inf)) == -1
    assert call(tm=(1, 2.0)) == 0
    assert lib.vrt_bloom_hdr(None, w, h, P["rgb"], None, None, None, P["ws"], P["f"], P["out"], None) == -1
    ctx.synchronize()
    host = np.zeros((h, w, 3), f32)
    out_f, out8 = np.zeros((h, w, 3), f32), np.zeros((h, w, 4), np.uint8)
    assert lib.vrt_bloom_hdr_host(ctx._h, w, h, None, None, None, None, out_f.ctypes.data, out8.ctypes.data) == -1
    assert lib.vrt_bloom_hdr_host(ctx._h, w, h, host.ctypes.data, None, None, None, None, None) == -1
    assert lib.vrt_bloom_hdr_host(ctx._h, 0, h, host.ctypes.data, None, None, None, out_f.ctypes.data, out8.ctypes.data) == -1
    assert lib.vrt_bloom_hdr_host(ctx._h, w, h, host.ctypes.data, C.byref(bad), None, None, out_f.ctypes.data, out8.ctypes.data) == -1
    assert lib.vrt_bloom_hdr_host(ctx._h, w, h, host.ctypes.data, None, C.byref(V.Tonemap(5, 1.0)), None, out_f.ctypes.data, out8.ctypes.data) == -1
    assert lib.vrt_bloom_hdr_host(None, w, h, host.ctypes.data, None, None, None, out_f.ctypes.data, out8.ctypes.data) == -1
    assert lib.vrt_bloom_hdr_host(ctx._h, w, h, host.ctypes.data, None, None, None, out_f.ctypes.data, None) == 0
    assert lib.vrt_bloom_hdr_host(ctx._h, w, h, host.ctypes.data, None, None, None, None, out8.ctypes.data) == 0
    assert (out8[..., 3] == 255).all() and not out8[..., :3].any()


@pytest.mark.parametrize("form", ["host", "device"])
def test_state_errors_of_the_accumulation_forms(V, form):
    import torch
    c = _fresh(V)
    try:
        d_rec = record_on_device(torch)
        d_f = torch.zeros((24, 40, 3), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        call = (lambda: c.accum_resolve_hdr_bloomed()) if form == "host" else (lambda: c.accum_resolve_hdr_bloomed_device(d_rec.data_ptr(), d_f.data_ptr(), None))
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
        e = V.Exposure()
        out8 = np.zeros((24, 40, 4), np.uint8)
        assert lib.vrt_accum_resolve_hdr_bloomed(c._h, None, None, None, C.byref(e), None, None) == -1             # no output
        assert lib.vrt_accum_resolve_hdr_bloomed(c._h, None, None, None, None, None, None) == -1
        assert lib.vrt_accum_resolve_hdr_bloomed_device(c._h, None, None, None, None, None, None, None) == -1
        p, q = d_rec.data_ptr(), d_f.data_ptr()
        assert lib.vrt_accum_resolve_hdr_bloomed_device(c._h, None, None, None, p, p, None, None) == -1            # record and f in one place
        assert lib.vrt_accum_resolve_hdr_bloomed_device(c._h, None, None, None, p, q, q, None) == -1               # f and the bytes in one place
        assert lib.vrt_accum_resolve_hdr_bloomed_device(c._h, None, None, None, p + 2, q, None, None) == -1
        assert lib.vrt_accum_resolve_hdr_bloomed_device(c._h, None, None, None, p, q + 1, None, None) == -1
        with pytest.raises(V.VrtError, match="vrt error -1"):
            c.accum_resolve_hdr_bloomed({"x0": 0, "y0": 0, "x1": 41, "y1": 24})                                    # a rectangle outside the frame
        bad_meter = V.Meter.from_buffer_copy(bytes(M.make(adapt=1.5)))
        assert lib.vrt_accum_resolve_hdr_bloomed(c._h, C.byref(bad_meter), None, None, C.byref(e), None, out8.ctypes.data) == -1
        assert lib.vrt_accum_resolve_hdr_bloomed(c._h, C.byref(bad_meter), None, None, None, None, out8.ctypes.data) == 0   # no metering: m is not read
        bad_bloom = V.Bloom.from_buffer_copy(bytes(B.make(levels=9)))
        assert lib.vrt_accum_resolve_hdr_bloomed(c._h, None, C.byref(bad_bloom), None, C.byref(e), None, out8.ctypes.data) == -1
        assert lib.vrt_accum_resolve_hdr_bloomed(c._h, None, None, C.byref(V.Tonemap(7, 1.0)), C.byref(e), None, out8.ctypes.data) == -1
        assert lib.vrt_accum_resolve_hdr_bloomed(None, None, None, None, None, None, out8.ctypes.data) == -1
        assert e.frames == 0, "a refused call leaves the record alone"
    finally:
        c.close()
