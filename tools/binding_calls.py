"""What the Python binding hands to libvrt_hip.so, recorded without a device: drives every public method of Context from cast_rays
to accum_resolve_hdr_temporal_mom_device over a stand-in for the library and prints one JSON line per C call (name and normalised
arguments) and one per method outcome (the returned arrays' shapes and dtypes, or the exception's type and message). Two commits
whose outputs are equal pass the same values to C for these inputs. CPU only; needs the built libraries (vrt_*_default run)."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vrt_import  # noqa: E402

V = vrt_import.vrt()

FORWARDED = ("vrt_filter_default", "vrt_filter_var_default", "vrt_temporal_default", "vrt_temporal_mom_default")
COUNTS = {"vrt_emitters": 2, "vrt_emitter_cdf": 2, "vrt_accum_counts": 3, "vrt_profile_read": 2}
LABEL = [""]


def norm(a):
    """integers below 2^32 and floats as they are, larger integers "ptr", None null, a byref struct its field values"""
    if a is None or isinstance(a, (str, bool)):
        return a
    if isinstance(a, (int, np.integer)):
        return int(a) if -2 ** 31 <= int(a) < 2 ** 32 else "ptr"
    if isinstance(a, (float, np.floating)):
        return repr(float(a))   # repr: nan and inf survive json
    if isinstance(a, bytes):
        return a.hex()
    if hasattr(a, "_obj"):      # C.byref(x)
        return norm(a._obj)
    if isinstance(a, C.Structure):
        return {k: norm(getattr(a, k)) for k, _ in a._fields_}
    if isinstance(a, C.Array):
        return [norm(v) for v in a]
    if isinstance(a, C._Pointer):
        return "ptr" if a else None
    if hasattr(a, "value"):     # c_void_p, c_size_t, c_uint32, ...
        return norm(a.value)
    return repr(a)


def emit(**kw):
    print(json.dumps({"call": LABEL[0], **kw}))


class Recorder:
    """the library as Context sees it: the four *_default functions are the real ones, every other call is written down"""

    def __init__(self):
        self._real = V.hip_lib()

    def __getattr__(self, name):
        if name in FORWARDED:
            return getattr(self._real, name)

        def call(*args):
            emit(fn=name, args=[norm(a) for a in args])
            return COUNTS.get(name, 0)
        return call


def shape_of(r):
    if isinstance(r, np.ndarray):
        return [list(r.shape), str(r.dtype)]
    if isinstance(r, (tuple, list)):
        return [shape_of(v) for v in r]
    if isinstance(r, dict):
        return {k: shape_of(v) for k, v in r.items()}
    return norm(r)


def drive(ctx, label, method, *args, **kw):
    LABEL[0] = label
    try:
        emit(returns=shape_of(getattr(ctx, method)(*args, **kw)))
    except Exception as e:   # the outcome is what is recorded
        emit(raises=[type(e).__name__, str(e)])


def fresh(shape=None):
    ctx = V.Context.__new__(V.Context)
    ctx._h = C.c_void_p(0x51)
    ctx._L = Recorder()
    if shape:
        ctx._accum_shape = shape
    return ctx


H, W, N = 2, 3, 5
D = list(range(0x100, 0x1000, 0x100))   # "device pointers": small, distinct, so the record shows which went where
INF, NAN = float("inf"), float("nan")
BAD_INT = (True, 1.5, "1", None, -1, 2 ** 40)
BAD_F32 = (0.0, -1.0, NAN, INF, 1e39, 1e-50, True, None, "1")
BAD_FLAG = (2, -1, "yes", None, 1.0)
TONEMAPS = (dict(), dict(tonemap="reinhard", exposure=2.5), dict(tonemap="clamp", exposure=np.float32(0.5)))
TONEMAPS_N = TONEMAPS + (dict(tonemap=None),)
BAD_TM = [dict(tonemap="aces"), dict(tonemap=1)] + [dict(exposure=e) for e in BAD_F32]
FILTERS = (None, {}, {"levels": 3, "demodulate": False, "sigma_normal": 0.25}, {"sigma_depth": 2, "sigma_albedo": np.float32(0.125)})
FILTERS_VAR = FILTERS + ({"sigma_lum": 3.0, "levels": np.int32(0)},)
BAD_FILTERS = [{"nope": 1}, {"levels": 9}, {"levels": -1}, {"levels": True}, {"levels": 2.0}] + \
              [{k: v} for k in ("sigma_normal", "sigma_albedo", "sigma_depth") for v in BAD_F32]
BAD_FILTERS_VAR = BAD_FILTERS + [{"sigma_lum": v} for v in BAD_F32]
TEMPORALS = (None, {}, {"max_history": 8, "alpha_min": 0.25, "offset_x": 0.5, "offset_y": -0.5}, {"depth_tol": 1, "normal_min": 0.5,
                                                                                                 "alpha_moments_min": 0.125})
TEMPORALS_MOM = TEMPORALS + ({"measured_below": 4, "search": 0, "max_history": 3},)


def main():
    rng = np.random.default_rng(7)
    o1, o = rng.random(3), rng.random((N, 3))
    d = rng.random((N, 3)).astype(np.float32)
    rgb = rng.random((H, W, 3))
    guides = {"normal": rng.random((H, W, 3)), "albedo": rng.random((H, W, 4)), "depth": rng.random((H, W)), "coverage": np.ones((H, W))}
    idd = np.zeros((H, W, 2), np.int32)
    var = rng.random((H, W))
    hist = rng.random((3, H, W, 4))
    cam = (rng.random(16), rng.random((4, 4)), rng.random(4))
    prev = (rng.random((4, 4)), rng.random(3))
    prev4 = (rng.random(16), rng.random(4))
    c = fresh((H, W))
    none = fresh()          # no accumulation begun

    # ---- queries and ray batches
    drive(c, "cast_rays shared", "cast_rays", o1, d)
    drive(c, "cast_rays each", "cast_rays", o, d, ((0, 0, 0), (64, 64, 64)))
    drive(c, "cast_rays empty", "cast_rays", np.zeros((0, 3)), np.zeros((0, 3)))
    for bad in ((o1, np.zeros((4, 2)), None), (o1, np.zeros(12), None), (np.zeros((3, 3)), np.zeros((4, 3)), None),
                (o1, d, ((0, 0, 0),)), (np.zeros(3, complex), d, None), (o1, np.zeros((2, 3), bool), None), (o1, d, "box")):
        drive(c, "cast_rays bad", "cast_rays", bad[0], bad[1], *(() if bad[2] is None else (bad[2],)))
    drive(c, "cast_rays_device", "cast_rays_device", N, D[0], 3, D[1], D[2])
    drive(c, "cast_rays_device stream box", "cast_rays_device", np.int64(N), D[0], 0, D[1], D[2], ((1, 2, 3), (4, 5, 6)), D[3])
    for n in BAD_INT + (2 ** 31,):
        drive(c, "cast_rays_device bad n", "cast_rays_device", n, D[0], 3, D[1], D[2])
    drive(c, "cast_rays_device bad stride", "cast_rays_device", N, D[0], 1, D[1], D[2])
    drive(c, "cast_rays_device bad box", "cast_rays_device", N, D[0], 3, D[1], D[2], ((0, 0), (1, 1)))
    drive(c, "find_voxels", "find_voxels", np.arange(12).reshape(4, 3))
    drive(c, "find_voxels empty", "find_voxels", np.zeros((0, 3), np.int32))
    for bad in (np.zeros((4, 3)), np.zeros((4, 2), int), np.full((1, 3), 2 ** 31)):
        drive(c, "find_voxels bad", "find_voxels", bad)
    drive(c, "shade_rays", "shade_rays", o1, d)
    drive(c, "shade_rays all", "shade_rays", o, d, V.MODE_PRIMARY, 3, 2 ** 32 + 7, 4)
    drive(c, "shade_rays_device", "shade_rays_device", N, D[0], 3, D[1], D[2], D[3])
    drive(c, "shade_rays_device all", "shade_rays_device", N, D[0], 0, D[1], None, D[3], V.MODE_PRIMARY_SHADOW, 2, 9, 3, D[4])
    for n in BAD_INT + (2 ** 30 + 1,):
        drive(c, "shade_rays_device bad n", "shade_rays_device", n, D[0], 3, D[1], D[2], D[3])
    for kw in TONEMAPS:
        drive(c, "shade_rays_hdr", "shade_rays_hdr", o1, d, **kw)
        drive(c, "shade_rays_hdr_device", "shade_rays_hdr_device", N, D[0], 3, D[1], D[2], D[3], D[4], **kw)
    drive(c, "shade_rays_hdr all", "shade_rays_hdr", o, d, V.MODE_PRIMARY, 2, 11, 6)
    drive(c, "shade_rays_hdr_device all", "shade_rays_hdr_device", N, D[0], 0, D[1], None, D[3], D[4], D[5], 4, V.MODE_PRIMARY, 2, 11,
          6, stream=D[6])
    for kw in BAD_TM + [dict(n_samples=v) for v in (0, 2 ** 24 + 1, 1.5, True)]:
        drive(c, "shade_rays_hdr bad", "shade_rays_hdr", o1, d, **kw)
    for kw in BAD_TM + [dict(n_samples=0), dict(n_prior=-1), dict(n_prior=True), dict(n_prior=2 ** 24, d_sums=D[5]), dict(n_prior=3),
                        dict(n=-1), dict(n=2 ** 30 + 1), dict(n=1.0), dict(n=False)]:
        kw = dict(dict(n=N), **kw)
        drive(c, "shade_rays_hdr_device bad", "shade_rays_hdr_device", kw.pop("n"), D[0], 3, D[1], D[2], D[3], D[4], **kw)
    drive(c, "guide_rays", "guide_rays", o1, d)
    drive(c, "guide_rays width", "guide_rays", o, d, 2)
    drive(c, "guide_rays_device", "guide_rays_device", N, D[0], 3, D[1], D[2], D[3], D[4], D[5])
    drive(c, "guide_rays_device all", "guide_rays_device", N, D[0], 0, D[1], None, D[3], None, D[5], 2, D[6])
    for n in BAD_INT + (2 ** 30 + 1,):
        drive(c, "guide_rays_device bad n", "guide_rays_device", n, D[0], 3, D[1], D[2], D[3], D[4], D[5])

    # ---- the accumulation and its settings
    b = fresh()
    drive(b, "accum_begin", "accum_begin", W, H)
    drive(b, "accum_begin all", "accum_begin", np.int32(W), H, 5, V.MODE_PRIMARY, True, None, True, True)
    drive(b, "accum_begin adaptive", "accum_begin", W, H, 0, V.MODE_FULL, 1, (2, 8, 3), 1, np.bool_(True))
    drive(b, "accum_begin adaptive list", "accum_begin", W, H, adaptive=[np.int64(2), 2, 0])
    LABEL[0] = "accum_begin shape"
    emit(returns=list(b._accum_shape))
    bads = [dict(hdr=v) for v in BAD_FLAG] + [dict(hdr=True, moments=v) for v in BAD_FLAG] + [dict(moments=True)] + \
           [dict(mode=v) for v in (3, -1, True, 1.0, "full", None)] + [dict(jitter=v) for v in BAD_FLAG] + [dict(mode=0, jitter=3)] + \
           [dict(width=v) for v in (0, -1, 64.0, True, 2 ** 30 + 1)] + [dict(height=v) for v in (0, 1.5, None)] + \
           [dict(width=1 << 16, height=1 << 15)] + [dict(first_sample=v) for v in (-1, 1 << 32, 1.5, True)] + \
           [dict(adaptive=v) for v in ((1, 8, 0), (0, 8, 0), (9, 8, 0), (2, 2 ** 24 + 1, 0), (2, 8, -1), (2, 8, 65536), (2, 8), (2, 8, 0, 1), 5,
                                       "2,8,0", (2.0, 8, 0), (2, True, 0), (2, 8, None), [2, 8, 1.5])] + \
           [dict(hdr=2, mode=7), dict(mode=7, jitter=2), dict(jitter=2, width=0), dict(width=0, first_sample=-1),
            dict(first_sample=-1, adaptive=5)]   # the order of the checks
    for kw in bads:
        kw = dict(dict(width=W, height=H), **kw)
        drive(fresh(), "accum_begin bad", "accum_begin", **kw)
    drive(c, "accum_counts", "accum_counts")
    drive(none, "accum_counts none", "accum_counts")
    drive(c, "set_lens", "set_lens", 0, 5)
    drive(c, "set_lens floats", "set_lens", np.float32(0.25), 1e-3)
    for a in ((-1.0, 5.0), (-1e-30, 5.0), (NAN, 5.0), (INF, 5.0), (1e39, 5.0), (1.0, 0.0), (1.0, -2.0), (1.0, NAN), (1.0, INF), (1.0, 1e39),
              (True, 5.0), (1.0, None), ("1", 5.0), (1.0, 1e-50)):
        drive(c, "set_lens bad", "set_lens", *a)
    for v in (1, np.int64(8), 0, 9) + BAD_INT:
        drive(c, "set_path_depth", "set_path_depth", v)
    for v in (0, 0.5, np.float32(1.0), 2, NAN) + (True, None, "1"):
        drive(c, "set_sun_disc", "set_sun_disc", v)
    for v in (0, 1, True, False, np.int32(1), np.bool_(True)) + BAD_FLAG:
        drive(c, "set_emitter_sampling", "set_emitter_sampling", v)
        drive(c, "set_emitter_mis", "set_emitter_mis", v)
    for v in (V.EMIT_UNIFORM, V.EMIT_POWER, np.int8(1), 2) + BAD_INT:
        drive(c, "set_emitter_importance", "set_emitter_importance", v)
    drive(c, "emitters", "emitters")
    drive(c, "emitter_cdf", "emitter_cdf")
    for v in (1, np.int64(7), 2 ** 24, 0, 2 ** 24 + 1) + BAD_INT:
        drive(c, "accum_add", "accum_add", v)
    drive(c, "accum_add default", "accum_add")

    # ---- resolves
    for ctx, tag in ((c, ""), (none, " none")):
        drive(ctx, "accum_resolve" + tag, "accum_resolve")
        drive(ctx, "accum_variance" + tag, "accum_variance")
        drive(ctx, "accum_guides" + tag, "accum_guides")
        for kw in TONEMAPS + tuple(BAD_TM):
            drive(ctx, "accum_resolve_hdr" + tag, "accum_resolve_hdr", **kw)
        for kw in TONEMAPS_N + tuple(BAD_TM):
            drive(ctx, "accum_resolve_hdr_shown" + tag, "accum_resolve_hdr_shown", **kw)
    drive(c, "accum_resolve_device", "accum_resolve_device", D[0], D[1], D[2])
    drive(c, "accum_resolve_device stream", "accum_resolve_device", D[0], None, None, D[3])
    drive(c, "accum_variance_device", "accum_variance_device", D[0])
    drive(c, "accum_variance_device stream", "accum_variance_device", D[0], D[1])
    drive(c, "accum_guides_device", "accum_guides_device", D[0], D[1], D[2], D[3])
    drive(c, "accum_guides_device stream", "accum_guides_device", None, D[1], None, D[3], D[4])
    for kw in TONEMAPS + tuple(BAD_TM):
        drive(c, "accum_resolve_hdr_device", "accum_resolve_hdr_device", D[0], D[1], D[2], **kw)
    drive(c, "accum_resolve_hdr_device stream", "accum_resolve_hdr_device", None, D[1], None, stream=D[3])
    for kw in TONEMAPS_N + tuple(BAD_TM):
        drive(c, "accum_resolve_hdr_shown_device", "accum_resolve_hdr_shown_device", D[0], D[1], **kw)
        drive(c, "denoise_hdr", "denoise_hdr", rgb, idd, **kw)
        drive(c, "denoise_hdr_device", "denoise_hdr_device", W, H, D[0], D[1], D[2], D[3], **kw)
    drive(c, "accum_resolve_hdr_shown_device stream", "accum_resolve_hdr_shown_device", None, D[1], stream=D[2])
    drive(c, "denoise_hdr_device stream", "denoise_hdr_device", W, H, D[0], D[1], None, D[3], stream=D[4])
    for bad in ((rgb[..., :2], idd), (rgb[0], idd), (rgb, idd[:1]), (rgb, idd[..., 0])):
        drive(c, "denoise_hdr bad", "denoise_hdr", *bad)

    # ---- the guided filters
    no_albedo = {k: v for k, v in guides.items() if k != "albedo"}
    bad_planes = [(rgb[..., :2], guides), (rgb[0], guides), (rgb, dict(guides, normal=guides["normal"][:1])), (rgb, dict(guides, albedo=rgb)),
                  (rgb, dict(guides, depth=rgb)), (rgb, dict(guides, coverage=var[:, :2])), (rgb, no_albedo)]
    for name, filters, bad_filters in (("", FILTERS, BAD_FILTERS), ("_var", FILTERS_VAR, BAD_FILTERS_VAR)):
        extra = (D[5],) if name else ()       # d_variance / d_variance_in
        extra_out = (D[8],) if name else ()   # d_out_variance
        for f in tuple(filters) + tuple(bad_filters):
            for kw in (TONEMAPS_N if f is None else TONEMAPS[:1]):
                drive(c, "filter_hdr" + name, "filter_hdr" + name, rgb, guides, filter=f, **kw)
                drive(c, "filter_hdr" + name + "_device", "filter_hdr" + name + "_device", W, H, *D[:5], *extra, D[6], D[7], *extra_out, filter=f, **kw)
                drive(c, "accum_resolve_hdr_filtered" + name, "accum_resolve_hdr_filtered" + name, filter=f, **kw)
                drive(c, "accum_resolve_hdr_filtered" + name + "_device", "accum_resolve_hdr_filtered" + name + "_device", D[0], D[1], *extra, filter=f,
                      **kw)
        for kw in BAD_TM + [dict(tonemap="aces", filter={"nope": 1})]:   # the tone map is checked before the filter
            drive(c, "filter_hdr" + name + " bad tonemap", "filter_hdr" + name, rgb, guides, **kw)
            drive(c, "filter_hdr" + name + "_device bad tonemap", "filter_hdr" + name + "_device", W, H, *D[:5], *extra, D[6], D[7], *extra_out, **kw)
            drive(c, "accum_resolve_hdr_filtered" + name + " bad tonemap", "accum_resolve_hdr_filtered" + name, **kw)
            drive(c, "accum_resolve_hdr_filtered" + name + "_device bad tonemap", "accum_resolve_hdr_filtered" + name + "_device", D[0], D[1], *extra, **kw)
        for bad in bad_planes:
            drive(c, "filter_hdr" + name + " bad planes", "filter_hdr" + name, *bad)
        drive(c, "filter_hdr" + name + " bad filter before planes", "filter_hdr" + name, rgb[0], guides, filter={"nope": 1})
        drive(none, "accum_resolve_hdr_filtered" + name + " none", "accum_resolve_hdr_filtered" + name)
        drive(c, "filter_hdr" + name + "_device stream", "filter_hdr" + name + "_device", W, H, *D[:5], *((None,) if name else ()), None, D[7],
              *((None,) if name else ()), stream=D[8])
        drive(c, "accum_resolve_hdr_filtered" + name + "_device stream", "accum_resolve_hdr_filtered" + name + "_device", None, D[1],
              *((None,) if name else ()), stream=D[3])
    drive(c, "filter_hdr_var variance", "filter_hdr_var", rgb, guides, var, {"levels": 2}, "reinhard", 2.0)
    for bad in (var[:1], var[..., None], rgb):
        drive(c, "filter_hdr_var bad variance", "filter_hdr_var", rgb, guides, bad)
    drive(c, "filter_hdr_var planes before variance", "filter_hdr_var", rgb[0], guides, var[:1])

    # ---- the temporal passes
    no_normal = {k: v for k, v in guides.items() if k != "normal"}
    bad_tplanes = [(rgb[..., :2], guides), (rgb[0], guides), (rgb, dict(guides, normal=guides["normal"][:1])), (rgb, dict(guides, depth=rgb)),
                   (rgb, dict(guides, coverage=var[:, :2])), (rgb, no_normal)]
    bad_cams = [(cam[0][:15], cam[1], cam[2]), (cam[0], cam[1][:3], cam[2]), (cam[0], cam[1], cam[2][:3]), cam[:2]]
    bad_prevs = [(prev[0][:3], prev[1]), (prev[0], np.zeros(5)), (prev[0],)]
    for name, temporals in (("", TEMPORALS), ("_mom", TEMPORALS_MOM)):
        bad_t = [{"nope": 1}, {"max_history": "x"}] + ([{"measured_below": 1}, {"search": 1}] if not name else [{"search": None}])
        vin = (D[9],) if name else ()   # d_variance_in
        for t in tuple(temporals) + tuple(bad_t):
            for h_, p_ in ((None, None), (hist, prev), (hist, prev4), (None, prev)):
                drive(c, "temporal_hdr" + name, "temporal_hdr" + name, cam, rgb, guides, history=h_, prev_camera=p_, temporal=t)
                drive(c, "accum_resolve_hdr_temporal" + name, "accum_resolve_hdr_temporal" + name, h_, p_, t)
            for dh, p_ in ((None, None), (D[4], prev), (None, prev4)):
                drive(c, "temporal_hdr" + name + "_device", "temporal_hdr" + name + "_device", W, H, cam, *D[:4], *vin, dh, D[5], D[6], D[7],
                      prev_camera=p_, temporal=t)
                drive(c, "accum_resolve_hdr_temporal" + name + "_device", "accum_resolve_hdr_temporal" + name + "_device", dh, *D[5:10],
                      prev_camera=p_, temporal=t)
        if name:
            drive(c, "temporal_hdr_mom variance", "temporal_hdr_mom", cam, rgb, guides, var, hist, prev)
            drive(c, "temporal_hdr_mom variance alone", "temporal_hdr_mom", cam, rgb, guides, variance=var)
            for bad in (var[:1], rgb):
                drive(c, "temporal_hdr_mom bad variance", "temporal_hdr_mom", cam, rgb, guides, bad, hist, prev)
            drive(c, "temporal_hdr_mom variance before history", "temporal_hdr_mom", cam, rgb, guides, var[:1], hist[:2], prev)
        for bad in bad_tplanes:
            drive(c, "temporal_hdr" + name + " bad planes", "temporal_hdr" + name, cam, *bad)
        for bad in bad_cams:
            drive(c, "temporal_hdr" + name + " bad camera", "temporal_hdr" + name, bad, rgb, guides)
            drive(c, "temporal_hdr" + name + "_device bad camera", "temporal_hdr" + name + "_device", W, H, bad, *D[:4], *vin, None, D[5], D[6], D[7])
        drive(c, "temporal_hdr" + name + " camera before planes", "temporal_hdr" + name, bad_cams[0], rgb[0], guides)
        for bad in (hist[:2], hist[..., :3], rgb):
            drive(c, "temporal_hdr" + name + " bad history", "temporal_hdr" + name, cam, rgb, guides, history=bad, prev_camera=prev)
            drive(c, "accum_resolve_hdr_temporal" + name + " bad history", "accum_resolve_hdr_temporal" + name, bad, prev)
        drive(c, "temporal_hdr" + name + " no prev_camera", "temporal_hdr" + name, cam, rgb, guides, history=hist)
        drive(c, "accum_resolve_hdr_temporal" + name + " no prev_camera", "accum_resolve_hdr_temporal" + name, hist)
        for bad in bad_prevs:
            drive(c, "temporal_hdr" + name + " bad prev_camera", "temporal_hdr" + name, cam, rgb, guides, history=hist, prev_camera=bad)
            drive(c, "accum_resolve_hdr_temporal" + name + " bad prev_camera", "accum_resolve_hdr_temporal" + name, hist, bad)
            drive(c, "temporal_hdr" + name + "_device bad prev_camera", "temporal_hdr" + name + "_device", W, H, cam, *D[:4], *vin, D[4], D[5], D[6],
                  D[7], prev_camera=bad)
            drive(c, "accum_resolve_hdr_temporal" + name + "_device bad prev_camera", "accum_resolve_hdr_temporal" + name + "_device", D[4],
                  *D[5:10], prev_camera=bad)
        drive(c, "temporal_hdr" + name + "_device no prev_camera", "temporal_hdr" + name + "_device", W, H, cam, *D[:4], *vin, D[4], D[5], D[6], D[7])
        drive(c, "temporal_hdr" + name + "_device stream", "temporal_hdr" + name + "_device", W, H, cam, *D[:4], *((None,) if name else ()), None,
              D[5], None, None, stream=D[8])
        for f in FILTERS_VAR[1:] + tuple(BAD_FILTERS_VAR[:3]):
            drive(c, "accum_resolve_hdr_temporal" + name + " filter", "accum_resolve_hdr_temporal" + name, hist, prev, None, f)
            drive(c, "accum_resolve_hdr_temporal" + name + "_device filter", "accum_resolve_hdr_temporal" + name + "_device", D[4], *D[5:10],
                  prev_camera=prev, filter=f)
        for kw in TONEMAPS_N[1:] + tuple(BAD_TM) + (dict(tonemap="aces", filter={"nope": 1}, temporal={"nope": 1}),
                                                     dict(filter={"nope": 1}, temporal={"nope": 1})):
            drive(c, "accum_resolve_hdr_temporal" + name + " tonemap", "accum_resolve_hdr_temporal" + name, **kw)
            drive(c, "accum_resolve_hdr_temporal" + name + "_device tonemap", "accum_resolve_hdr_temporal" + name + "_device", None, *D[5:10], **kw)
        drive(c, "accum_resolve_hdr_temporal" + name + " filter before history", "accum_resolve_hdr_temporal" + name, hist[:2], prev,
              filter={"nope": 1})
        drive(none, "accum_resolve_hdr_temporal" + name + " none", "accum_resolve_hdr_temporal" + name)
        drive(none, "accum_resolve_hdr_temporal" + name + " none history", "accum_resolve_hdr_temporal" + name, hist, prev)
        drive(c, "accum_resolve_hdr_temporal" + name + "_device stream", "accum_resolve_hdr_temporal" + name + "_device", None, D[5], None, None,
              D[8], None, stream=D[3])

    # ---- the private builders tests and tools use
    LABEL[0] = "builders"
    for t, p_ in ((None, None), ({"offset_x": 1}, prev), (None, prev4)):
        emit(fn="_temporal", args=[norm(V.Context._temporal(t, p_))])
        emit(fn="_temporal_mom", args=[norm(V.Context._temporal_mom(t, p_))])
    emit(fn="defaults", args=[V.default_filter(), V.default_filter_var(), V.default_temporal(), V.default_temporal_mom()])
    emit(fn="default types", args=[[[k, type(v).__name__] for k, v in f().items()]
                                   for f in (V.default_filter, V.default_filter_var, V.default_temporal, V.default_temporal_mom)])
    drive(c, "profile_read", "profile_read", 4)


if __name__ == "__main__":
    main()
