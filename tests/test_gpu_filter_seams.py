"""The guided filter's lattice levels on the MI355X at frames that cross tile seams (vrt_filter_hdr, vrt_filter_hdr_var) against the
checkers (tests/oracle_filter_hdr.c, tests/oracle_filter_var.c), bit for bit on every output.

The frames are tests/filter_geometry.py's SEAM_SHAPES: between them every lattice step has, in both axes, an interior tile, a ragged
last tile, a residue class with fewer tiles than class 0 (the workgroup that returns whole) and an exact fit, and steps 2 and 4 run
as a middle and as the last level (tests/test_filter_geometry.py asserts that of the compiled tile, without a device). Two inputs per
frame (tests/filter_seam_cases.py): random planes with NaN, Inf, dead pixels and negative depths, and smooth planes on which every
tap carries weight.

The sensitivity condition, asserted on the checkers alone before the device is asked anything (the `cases` fixture): doubling one
input line that only the step-4 taps can carry across a seam -- column 121 for the seam at x = 128, row 25 for y = 32, and columns
134 / rows 38 back across it -- changes the checker's output beyond the seam: every seam-adjacent pixel on the smooth planes, at
least one eighth of them on the random ones, and none with the step-4 level left out. So a halo staged wrongly at a seam cannot
compare equal. Measured at 257 x 33, 3 levels (guide-only checker; pixels changed of pixels observed):
  smooth  column 121: 264 of 264   column 134: 264 of 264   row 25: 257 of 257
  random  column 121:  72 of 264   column 134:  99 of 264   row 25: 134 of 257
The accumulation routes launch the same kernels and stay at the sizes of tests/test_gpu_filter_hdr.py and test_gpu_filter_var.py."""
import numpy as np
import pytest

import filter_geometry as FG
import filter_seam_cases as SC
import oracle_filter_hdr as F
import oracle_filter_var as FV

pytestmark = pytest.mark.gpu

KINDS = ("random", "smooth")
SWEPT, SWEPT_VAR = SC.SWEPT, SC.SWEPT_VAR
OPTIONS = ((True, "clamp", 1.0), (False, "reinhard", 0.6))                      # demodulation, tone map, exposure
_ids = dict(ids=lambda s: f"{s[0]}x{s[1]}")


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return FV.build(tmp_path_factory.mktemp("oracle_filter_seams"))             # holds the guide-only checker too


@pytest.fixture(scope="module")
def K(V):
    return FG.constants(V)


@pytest.fixture(scope="module")
def cases(L, K):
    """(kind, (W, H)) -> (rgb, guides, variance plane), each made once and held to the sensitivity condition first"""
    no_event, no_form = FG.missing(K, FG.SEAM_SHAPES, FG.SEAM_LEVELS)
    assert not no_event and not no_form, (no_event, no_form)
    out = {}
    for w, h in FG.SEAM_SHAPES:
        for kind in KINDS:
            rgb, g, var = SC.make(kind, w, h)
            SC.assert_sensitive(L, K, kind, w, h, rgb, g, var)
            out[kind, (w, h)] = (rgb, g, var)
    return out


@pytest.fixture(scope="module")
def ctx(V, cases):                                                              # after `cases`: the checkers are asked first
    c = V.Context(0)
    yield c
    c.close()


def _f(levels, demod, **kw):
    return {"levels": levels, "demodulate": demod, **kw}


def _same_all(got, want, what):
    for a, b, name in zip(got, want, ("floats", "bytes", "variance")):
        F.same(a, b, f"{what}: {name}")
    assert len(got) == len(want)


@pytest.mark.parametrize("levels", FG.SEAM_LEVELS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", FG.SEAM_SHAPES, **_ids)
def test_guide_only_filter_is_the_checkers(ctx, L, cases, size, kind, levels):
    rgb, g, _ = cases[kind, size]
    for demod, tonemap, exposure in OPTIONS:
        want = F.filter(L, rgb, g, F.make(levels, demod, **SWEPT), tonemap, exposure)
        _same_all(ctx.filter_hdr(rgb, g, _f(levels, demod, **SWEPT), tonemap, exposure), want, f"{size} {kind} levels {levels} demod {demod} {tonemap}")
        assert (want[0] != F.h_of(rgb)).any()


@pytest.mark.parametrize("plane", [False, True], ids=["spatial", "plane"])
@pytest.mark.parametrize("levels", FG.SEAM_LEVELS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", FG.SEAM_SHAPES, **_ids)
def test_variance_guided_filter_is_the_checkers(ctx, L, cases, size, kind, levels, plane):
    rgb, g, var = cases[kind, size]
    var = var if plane else None
    for demod, tonemap, exposure in OPTIONS:
        want = FV.filter(L, rgb, g, FV.make(levels, demod, **SWEPT_VAR), var, tonemap, exposure)
        _same_all(ctx.filter_hdr_var(rgb, g, var, _f(levels, demod, **SWEPT_VAR), tonemap, exposure), want,
                  f"{size} {kind} levels {levels} plane {plane} demod {demod} {tonemap}")
        assert want[2].any() and np.isfinite(want[2]).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", [(257, 33), (131, 35)], **_ids)
def test_each_output_null_in_turn(ctx, L, cases, size, kind):
    """the device forms at 3 levels (step 4 stores the outputs): what is not asked for is not written, the rest is the checker's"""
    import torch
    rgb, g, var = cases[kind, size]
    w, h = size
    ins = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (rgb, g["normal"], g["albedo"], g["depth"], g["coverage"])]
    d_var = torch.from_numpy(var).to("cuda:0")
    outs = (torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"), torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0"),
            torch.zeros((h, w), dtype=torch.float32, device="cuda:0"))
    ptrs = [t.data_ptr() for t in ins]

    def check(used, want, what):
        torch.cuda.synchronize()
        for o, u, w_, name in zip(outs, used, want, ("floats", "bytes", "variance")):
            if u:
                F.same(o.cpu().numpy(), w_, f"{what}: {name}")
            else:
                assert not o.any(), f"{what}: {name} written though NULL"
            o.zero_()
        torch.cuda.synchronize()

    torch.cuda.synchronize()
    want = F.filter(L, rgb, g, F.make(3, True, **SWEPT), "reinhard", 0.6)
    for used in ((1, 1), (1, 0), (0, 1)):
        ctx.filter_hdr_device(w, h, *ptrs, *(o.data_ptr() if u else None for o, u in zip(outs, used)), _f(3, True, **SWEPT), "reinhard", 0.6)
        check(used + (0,), want, f"{size} {kind} guide-only outputs {used}")
    for plane in (None, d_var):
        want = FV.filter(L, rgb, g, FV.make(3, True, **SWEPT_VAR), var if plane is not None else None, "reinhard", 0.6)
        for used in ((1, 1, 1), (1, 0, 1), (0, 1, 1), (1, 1, 0)):
            ctx.filter_hdr_var_device(w, h, *ptrs, plane.data_ptr() if plane is not None else None,
                                      *(o.data_ptr() if u else None for o, u in zip(outs, used)), _f(3, True, **SWEPT_VAR), "reinhard", 0.6)
            check(used, want, f"{size} {kind} variance-guided plane {plane is not None} outputs {used}")
    del ins, d_var
