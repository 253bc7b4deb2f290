"""ctypes bindings over the two C-ABI libraries of the MI355X ray-casting path.

    libvrt_host.so  (include/vrt_host.h)  host API kept from the reference:
                    octree build/flatten, .vox loader, camera block
    libvrt_hip.so   (include/vrt.h)       the gfx950 dispatch layer

The directory name carries a hyphen, so import it with
``importlib.import_module("voxel-raytracer_amd")`` (see ``vrt_import.py`` at the
repository root). There is no CPU fallback anywhere in this package: `Context`
raises if the HIP library is missing or no GPU is present.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
HIP_LIB = os.environ.get("VRT_HIP_LIB") or os.path.join(HERE, "libvrt_hip.so")   # VRT_HIP_LIB: an A/B build of the same library (tools)
HOST_LIB = os.path.join(HERE, "libvrt_host.so")
TEST_LIB = os.path.join(HERE, "libvrt_hip_test.so")   # test support, not product (csrc/test/vrt_test.hip)
OPT_RAY_TABLES, OPT_EMPTY_OCTANTS, OPT_DISPLAY_KERNEL, OPT_FULL_OPAQUE, OPT_HEAVY_TILES, OPT_MISS_TILES = 1, 2, 3, 4, 5, 6

MODE_PRIMARY, MODE_PRIMARY_SHADOW, MODE_FULL = 0, 1, 2
MODES = {"primary": MODE_PRIMARY, "primary_shadow": MODE_PRIMARY_SHADOW, "full": MODE_FULL}
ACCUM_JITTER = 1   # vrt_accum_begin_ex flags (include/vrt.h VRT_ACCUM_JITTER)
MAX_PATH_DEPTH = 8   # include/vrt.h VRT_MAX_PATH_DEPTH (Context.set_path_depth)
MAX_EMITTERS = 1 << 20   # include/vrt.h VRT_MAX_EMITTERS (Context.emitters, Context.set_emitter_sampling)
EMIT_UNIFORM, EMIT_POWER = 0, 1   # include/vrt.h VRT_EMIT_* (Context.set_emitter_importance)
TONEMAP_CLAMP, TONEMAP_REINHARD = 0, 1   # include/vrt.h VRT_TONEMAP_*
TONEMAPS = {"clamp": TONEMAP_CLAMP, "reinhard": TONEMAP_REINHARD}


class Tonemap(C.Structure):
    """include/vrt.h vrt_tonemap"""
    _fields_ = [("op", C.c_int32), ("exposure", C.c_float)]


class Filter(C.Structure):
    """include/vrt.h vrt_filter"""
    _fields_ = [("levels", C.c_int32), ("flags", C.c_uint32), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float),
                ("sigma_depth", C.c_float)]


class FilterVar(C.Structure):
    """include/vrt.h vrt_filter_var"""
    _fields_ = Filter._fields_ + [("sigma_lum", C.c_float)]


class Temporal(C.Structure):
    """include/vrt.h vrt_temporal"""
    _fields_ = [("prev_view_proj", C.c_float * 16), ("prev_camera_pos", C.c_float * 4), ("offset_x", C.c_float), ("offset_y", C.c_float),
                ("max_history", C.c_int32), ("alpha_min", C.c_float), ("alpha_moments_min", C.c_float), ("normal_min", C.c_float),
                ("depth_tol", C.c_float)]


class TemporalMom(C.Structure):
    """include/vrt.h vrt_temporal_mom"""
    _fields_ = Temporal._fields_ + [("measured_below", C.c_int32), ("search", C.c_int32)]


class Upsample(C.Structure):
    """include/vrt.h vrt_upsample"""
    _fields_ = [("factor", C.c_int32), ("flags", C.c_uint32), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float),
                ("sigma_depth", C.c_float), ("min_weight", C.c_float), ("offset_lo_x", C.c_float), ("offset_lo_y", C.c_float),
                ("offset_hi_x", C.c_float), ("offset_hi_y", C.c_float)]


class Meter(C.Structure):
    """include/vrt.h vrt_meter"""
    _fields_ = [("key", C.c_float), ("low_permille", C.c_int32), ("high_permille", C.c_int32), ("min_exposure", C.c_float),
                ("max_exposure", C.c_float), ("adapt", C.c_float), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32)]


class Exposure(C.Structure):
    """include/vrt.h vrt_exposure: the record a caller carries from frame to frame"""
    _fields_ = [("exposure", C.c_float), ("metered", C.c_float), ("window", C.c_uint32), ("frames", C.c_uint32)]


class Bloom(C.Structure):
    """include/vrt.h vrt_bloom"""
    _fields_ = [("levels", C.c_int32), ("flags", C.c_uint32), ("threshold", C.c_float), ("knee", C.c_float), ("intensity", C.c_float)]


TEMPORAL_KEYS = ("offset_x", "offset_y", "max_history", "alpha_min", "alpha_moments_min", "normal_min", "depth_tol")
TEMPORAL_MOM_KEYS = TEMPORAL_KEYS + ("measured_below", "search")
_TEMPORAL_INTS = ("max_history", "measured_below", "search")   # the keys that are int32 fields; the others are floats
# the two temporal structs as (mirror, the library's default function, the keys a caller may set)
_TEMPORAL = (Temporal, "vrt_temporal_default", TEMPORAL_KEYS)
_TEMPORAL_MOM = (TemporalMom, "vrt_temporal_mom_default", TEMPORAL_MOM_KEYS)
HISTORY_BYTES = 48       # include/vrt.h vrt_temporal_hdr: a history's bytes per pixel, three planes of 16-byte words

FILTER_MAX_LEVELS = 8    # include/vrt.h VRT_FILTER_MAX_LEVELS
FILTER_DEMODULATE = 1    # include/vrt.h VRT_FILTER_DEMODULATE
UPSAMPLE_MAX_FACTOR = 4  # include/vrt.h VRT_UPSAMPLE_MAX_FACTOR
UPSAMPLE_DEMODULATE = 1  # include/vrt.h VRT_UPSAMPLE_DEMODULATE
METER_BINS = 256         # include/vrt.h VRT_METER_BINS
BLOOM_MAX_LEVELS = 8     # include/vrt.h VRT_BLOOM_MAX_LEVELS
BLOOM_KARIS = 1          # include/vrt.h VRT_BLOOM_KARIS


class VrtError(RuntimeError):
    pass


def _filter_defaults(struct, default):
    f = struct()
    getattr(hip_lib(), default)(C.byref(f))
    d = {"levels": int(f.levels), "demodulate": bool(f.flags & FILTER_DEMODULATE)}
    d.update((k, float(getattr(f, k))) for k, _ in struct._fields_[2:])   # the sigmas
    return d


def default_filter():
    """vrt_filter_default as a dict: {"levels", "demodulate", "sigma_normal", "sigma_albedo", "sigma_depth"} -- the keyword
    arguments Context.filter_hdr and Context.accum_resolve_hdr_filtered take. Needs no device."""
    return _filter_defaults(Filter, "vrt_filter_default")


def default_filter_var():
    """vrt_filter_var_default as a dict: default_filter()'s keys and "sigma_lum" -- the keyword arguments Context.filter_hdr_var and
    Context.accum_resolve_hdr_filtered_var take. Needs no device."""
    return _filter_defaults(FilterVar, "vrt_filter_var_default")


def default_upsample():
    """vrt_upsample_default as a dict: {"factor", "demodulate", "sigma_normal", "sigma_albedo", "sigma_depth", "min_weight",
    "offset_lo_x", "offset_lo_y", "offset_hi_x", "offset_hi_y"} -- the keys the `upsample` argument of Context.upsample_hdr and
    Context.accum_resolve_hdr_upsampled takes. Needs no device."""
    u = Upsample()
    hip_lib().vrt_upsample_default(C.byref(u))
    d = {"factor": int(u.factor), "demodulate": bool(u.flags & UPSAMPLE_DEMODULATE)}
    d.update((k, float(getattr(u, k))) for k, _ in Upsample._fields_[2:])
    return d


_METER_INTS = ("low_permille", "high_permille", "x0", "y0", "x1", "y1")   # the keys that are int32 fields; the others are floats


def default_meter():
    """vrt_meter_default as a dict: {"key", "low_permille", "high_permille", "min_exposure", "max_exposure", "adapt", "x0", "y0", "x1",
    "y1"} -- the keys the `meter` argument of meter_resolve, Context.meter_hdr and Context.accum_resolve_hdr_metered takes. Needs no
    device."""
    m = Meter()
    hip_lib().vrt_meter_default(C.byref(m))
    return {k: (int if k in _METER_INTS else float)(getattr(m, k)) for k, _ in Meter._fields_}


def _meter(meter):
    """None (the NULL vrt_meter: vrt_meter_default) or a dict with any of default_meter()'s keys -> Meter or None; ValueError for an
    unknown key, a key that is not finite and > 0, a rank window that is not 0 <= low < high <= 1000, exposure bounds that are not
    finite with 0 < min <= max, an adapt outside (0, 1] or a rectangle with a negative or inverted side (its fit into the frame is the
    library's to check)"""
    if meter is None:
        return None
    d = default_meter()
    unknown = set(meter) - set(d)
    if unknown:
        raise ValueError(f"meter: unknown keys {sorted(unknown)}")
    d.update(meter)
    key = _check_f32("key", d["key"], _positive, "finite and > 0")
    high = _check_int("high_permille", d["high_permille"], "an integer in [1, 1000]", 1, 1000)
    low = _check_int("low_permille", d["low_permille"], "an integer in [0, high_permille)", 0, high - 1)
    lo = _check_f32("min_exposure", d["min_exposure"], _positive, "finite and > 0")
    hi = _check_f32("max_exposure", d["max_exposure"], lambda x: x >= lo, "finite and >= min_exposure")
    adapt = _check_f32("adapt", d["adapt"], lambda x: 0.0 < x <= 1.0, "in (0, 1]")
    rect = [_check_int(k, d[k], "an integer in [0, 2^30]", 0, 1 << 30) for k in ("x0", "y0", "x1", "y1")]
    if any(rect) and not (rect[0] < rect[2] and rect[1] < rect[3]):
        raise ValueError(f"rectangle: expected all zeros or x0 < x1 and y0 < y1, got {rect}")
    return Meter(key, low, high, lo, hi, adapt, *rect)


def _exposure(state):
    """None (a zeroed record: the first frame) or a dict as meter_resolve returns it -> Exposure"""
    if state is None:
        return Exposure()
    unknown = set(state) - {"exposure", "metered", "window", "frames"}
    if unknown:
        raise ValueError(f"state: unknown keys {sorted(unknown)}")
    return Exposure(float(np.float32(state.get("exposure", 0.0))), float(np.float32(state.get("metered", 0.0))),
                    _check_int("window", state.get("window", 0), "an integer in [0, 2^32)", 0, 0xffffffff),
                    _check_int("frames", state.get("frames", 0), "an integer in [0, 2^32)", 0, 0xffffffff))


def _exposure_dict(e):
    return {"exposure": float(e.exposure), "metered": float(e.metered), "window": int(e.window), "frames": int(e.frames)}


def meter_resolve(hist, meter=None, state=None):
    """vrt_meter_resolve: E4-E8 of include/vrt.h on the host from a histogram of METER_BINS counts. meter: None (vrt_meter_default) or
    a dict with any of default_meter()'s keys; state: None (a zeroed record) or the dict an earlier call returned -> the new record
    {"exposure", "metered", "window", "frames"}. Needs no device."""
    h = np.ascontiguousarray(hist, np.uint32)
    if h.shape != (METER_BINS,):
        raise ValueError(f"expected {METER_BINS} counts, got {h.shape}")
    if np.any(np.asarray(hist) != h):
        raise ValueError("every count must be an integer in [0, 2^32)")
    e = _exposure(state)
    r = hip_lib().vrt_meter_resolve(h.ctypes.data, _ref(_meter(meter)), C.byref(e))
    if r != 0:
        raise VrtError(f"vrt_meter_resolve: error {r} (the counts sum to more than 2^30)")
    return _exposure_dict(e)


def default_bloom():
    """vrt_bloom_default as a dict: {"levels", "karis", "threshold", "knee", "intensity"} -- the keys the `bloom` argument of
    Context.bloom_hdr and Context.accum_resolve_hdr_bloomed takes. Needs no device."""
    b = Bloom()
    hip_lib().vrt_bloom_default(C.byref(b))
    return {"levels": int(b.levels), "karis": bool(b.flags & BLOOM_KARIS), "threshold": float(b.threshold), "knee": float(b.knee),
            "intensity": float(b.intensity)}


def _bloom(bloom):
    """None (the NULL vrt_bloom: vrt_bloom_default) or a dict with any of default_bloom()'s keys -> Bloom or None; ValueError for an
    unknown key, levels outside 1..BLOOM_MAX_LEVELS, a karis that is no flag, not 0 <= knee <= threshold <= 65504 or an intensity
    outside [0, 65504]"""
    if bloom is None:
        return None
    d = default_bloom()
    unknown = set(bloom) - set(d)
    if unknown:
        raise ValueError(f"bloom: unknown keys {sorted(unknown)}")
    d.update(bloom)
    levels = _check_int("levels", d["levels"], f"an integer in [1, {BLOOM_MAX_LEVELS}]", 1, BLOOM_MAX_LEVELS)
    karis = _check_flag("karis", d["karis"], "a bool")
    threshold = _check_f32("threshold", d["threshold"], lambda x: 0.0 <= x <= 65504.0, "in [0, 65504]")
    knee = _check_f32("knee", d["knee"], lambda x: 0.0 <= x <= threshold, "in [0, threshold]")
    intensity = _check_f32("intensity", d["intensity"], lambda x: 0.0 <= x <= 65504.0, "in [0, 65504]")
    return Bloom(levels, BLOOM_KARIS if karis else 0, threshold, knee, intensity)


def bloom_workspace_bytes(width, height, levels):
    """vrt_bloom_workspace_bytes: the bytes of the workspace Context.bloom_hdr_device needs for a width x height frame and `levels`
    levels; 0 for arguments the call would refuse. Needs no device."""
    for name, v in (("width", width), ("height", height), ("levels", levels)):
        _check_int(name, v, "an int32", -(1 << 31), (1 << 31) - 1)
    return int(hip_lib().vrt_bloom_workspace_bytes(width, height, levels))


def _temporal_struct(kind, temporal=None, prev_camera=None):
    """kind: _TEMPORAL or _TEMPORAL_MOM. The library's defaults, then the caller's keys (ValueError for one the struct does not
    have), then the previous frame's camera where a history comes in -> the struct"""
    struct, default, keys = kind
    t = struct()
    getattr(hip_lib(), default)(C.byref(t))
    for k, v in (temporal or {}).items():
        if k not in keys:
            raise ValueError(f"unknown temporal key {k!r}; expected any of {keys}")
        setattr(t, k, int(v) if k in _TEMPORAL_INTS else float(v))
    if prev_camera is not None:
        vp = np.ascontiguousarray(prev_camera[0], np.float32).reshape(-1)
        cp = np.ascontiguousarray(prev_camera[1], np.float32).reshape(-1)
        if vp.size != 16 or cp.size not in (3, 4):
            raise ValueError("expected prev_camera = (prev_view_proj[16], prev_camera_pos[3 or 4])")
        t.prev_view_proj[:] = [float(v) for v in vp]
        t.prev_camera_pos[:cp.size] = [float(v) for v in cp]
    return t


def _temporal_defaults(kind):
    t = _temporal_struct(kind)
    return {k: (int if k in _TEMPORAL_INTS else float)(getattr(t, k)) for k in kind[2]}


def default_temporal():
    """vrt_temporal_default as a dict: {"offset_x", "offset_y", "max_history", "alpha_min", "alpha_moments_min", "normal_min",
    "depth_tol"} -- the keys the `temporal` argument of Context.temporal_hdr and Context.accum_resolve_hdr_temporal takes. The
    previous camera is an argument of its own there. Needs no device."""
    return _temporal_defaults(_TEMPORAL)


def default_temporal_mom():
    """vrt_temporal_mom_default as a dict: default_temporal()'s keys, "measured_below" and "search" -- the keys the `temporal`
    argument of Context.temporal_hdr_mom and Context.accum_resolve_hdr_temporal_mom takes. Needs no device."""
    return _temporal_defaults(_TEMPORAL_MOM)


def build(targets=("../libvrt_hip.so", "../libvrt_hip_test.so", "../libvrt_host.so")):
    """Compile the libraries in-tree (hipcc --offload-arch=gfx950 / g++)."""
    subprocess.check_call(["make", "-j8", "-C", CSRC, *targets])


class Params(C.Structure):
    _fields_ = [("voxel_scale", C.c_float), ("world_min", C.c_int32 * 3), ("world_max", C.c_int32 * 3),
                ("global_light", C.c_float * 4), ("light_dir", C.c_float * 3), ("highlighted", C.c_int32 * 3)]


class View(C.Structure):
    """vrt_view: one camera block and the two device images it renders into"""
    _fields_ = [("inv_projection", C.c_float * 16), ("inv_view", C.c_float * 16), ("camera_pos", C.c_float * 4),
                ("d_rgba8", C.c_void_p), ("d_id_dist", C.c_void_p)]


class Patch(C.Structure):
    """vrt_patch: an ancestor of an edited voxel, by depth and child-index path"""
    _fields_ = [("depth", C.c_int32), ("path", C.c_uint8 * 16)]


class SceneInfo(C.Structure):
    _fields_ = [("tex_dim", C.c_uint32), ("n_texels", C.c_uint32), ("n_records", C.c_uint32),
                ("n_internal", C.c_uint32), ("n_leaves", C.c_uint32), ("max_depth", C.c_uint32),
                ("lds_records", C.c_uint32), ("reserved", C.c_uint32)]


class RayHit(C.Structure):
    """vrt_ray_hit: one answer of vrt_cast_rays (40 bytes)"""
    _fields_ = [("hit", C.c_int32), ("coord", C.c_int32 * 3), ("place", C.c_int32 * 3), ("leaf", C.c_uint32 * 2),
                ("steps", C.c_int32)]


# the same record as a numpy dtype, for arrays of answers
RAY_HIT_DTYPE = np.dtype([("hit", np.int32), ("coord", np.int32, 3), ("place", np.int32, 3), ("leaf", np.uint32, 2),
                          ("steps", np.int32)])
WORLD_BOX = ((0.0, 0.0, 0.0), (1024.0, 1024.0, 1024.0))   # the box src/main.cpp:827 passes to octree_ray_cast


def _real_array(a, what):
    a = np.asarray(a)
    if a.dtype.kind not in "fiu":
        raise TypeError(f"{what}: expected real numbers, got dtype {a.dtype}")
    return a


# ---- The argument checks. Each takes the variable parts of its message: callers and tests read the texts.
def _check_int(name, v, want, lo=None, hi=None):
    """v: an int or np.integer, not a bool, in [lo, hi] (None: unbounded) -> int(v); ValueError "{name}: expected {want}, got ..."
    otherwise"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or (lo is not None and v < lo) or (hi is not None and v > hi):
        raise ValueError(f"{name}: expected {want}, got {v!r}")
    return int(v)


def _check_f32(name, v, ok, want):
    """v: a number, not a bool, whose float32 value is finite and satisfies ok() -> that value as a Python float; ValueError
    otherwise, "expected a float32 value {want}" for a number"""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name}: expected a number, got {v!r}")
    x = float(v)
    f = np.float32(x) if abs(x) <= float(np.finfo(np.float32).max) else np.float32(np.nan)
    if not (np.isfinite(f) and ok(f)):
        raise ValueError(f"{name}: expected a float32 value {want}, got {v!r}")
    return float(f)


def _positive(x):
    return x > 0.0


def _check_flag(name, v, want, bools=(bool, np.bool_)):
    """v: one of `bools`, or an int or np.integer that is 0 or 1 -> 0 or 1; ValueError "{name}: expected {want}, got ..." otherwise"""
    if not isinstance(v, bools) and not (isinstance(v, (int, np.integer)) and v in (0, 1)):
        raise ValueError(f"{name}: expected {want}, got {v!r}")
    return int(v)


def query_ray_args(origins, dirs, box=WORLD_BOX):
    """Checks and converts the arguments of Context.cast_rays (no device involved) -> (origins float32[k, 3] with k = 1
    (shared origin) or n, origin_stride 0 or 3, dirs float32[n, 3], box_min float32[3], box_max float32[3])."""
    o = _real_array(origins, "origins")
    d = _real_array(dirs, "dirs")
    if d.ndim != 2 or d.shape[1] != 3:
        raise ValueError(f"dirs: expected shape (n, 3), got {d.shape}")
    if o.shape == (3,):
        stride = 0
        o = o.reshape(1, 3)
    elif o.ndim == 2 and o.shape[1] == 3 and o.shape[0] == d.shape[0]:
        stride = 3
    else:
        raise ValueError(f"origins: expected shape (3,) or ({d.shape[0]}, 3), got {o.shape}")
    if d.shape[0] >= 2 ** 31:
        raise ValueError("at most 2^31 rays per call")
    b = _real_array(box, "box")
    if b.shape != (2, 3):
        raise ValueError(f"box: expected ((x, y, z), (x, y, z)), got shape {b.shape}")
    return (np.ascontiguousarray(o, np.float32), stride, np.ascontiguousarray(d, np.float32),
            np.ascontiguousarray(b[0], np.float32), np.ascontiguousarray(b[1], np.float32))


def shade_ray_args(origins, dirs):
    """Checks and converts the ray arguments of Context.shade_rays (no device involved) -> (origins float32[k, 3] with k = 1
    (shared origin) or n, origin_stride 0 or 3, dirs float32[n, 3])."""
    o, stride, d, _, _ = query_ray_args(origins, dirs)
    if d.shape[0] > 2 ** 30:
        raise ValueError("at most 2^30 rays per call")
    return o, stride, d


def query_point_args(coords):
    """Checks and converts the argument of Context.find_voxels (no device involved) -> int32[n, 3]."""
    c = np.asarray(coords)
    if c.dtype.kind not in "iu":
        raise TypeError(f"coords: expected integers, got dtype {c.dtype}")
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError(f"coords: expected shape (n, 3), got {c.shape}")
    if c.size and (c.min() < -2 ** 31 or c.max() >= 2 ** 31):
        raise ValueError("coords: values outside int32")
    if c.shape[0] >= 2 ** 31:
        raise ValueError("at most 2^31 points per call")
    return np.ascontiguousarray(c, np.int32)


# ---- The foreign-function signatures: one table per library, name -> (restype, argtypes), applied once when the library loads.
# HOST_API and HIP_API hold every function of include/vrt_host.h and include/vrt.h (tests/test_abi.py compares them with the
# prototypes); TEST_API the probes of libvrt_hip_test.so this module calls. A row reads like its prototype:
_i, _u32, _u64, _f, _sz, _long = C.c_int, C.c_uint32, C.c_uint64, C.c_float, C.c_size_t, C.c_long
_p, _s = C.c_void_p, C.c_char_p   # void *: handles, streams, host and device buffers; const char *: strings and Python bytes
_pi, _pi32, _pu32, _pu8, _pf, _pl, _psz, _pp = (C.POINTER(t) for t in (C.c_int, C.c_int32, C.c_uint32, C.c_uint8, C.c_float, C.c_long,
                                                                       C.c_size_t, C.c_void_p))
_tm, _flt, _fltv, _tmp, _tmpm, _ups = (C.POINTER(t) for t in (Tonemap, Filter, FilterVar, Temporal, TemporalMom, Upsample))
_mtr, _exp, _blm = C.POINTER(Meter), C.POINTER(Exposure), C.POINTER(Bloom)
_RECORDS_OUT = [_pp, _psz]        # uint32_t **records, size_t *n_records

HOST_API = {
    "vrth_world_create": (_p, [_pi32, _pi32]),
    "vrth_world_destroy": (None, [_p]),
    "vrth_world_root": (_p, [_p]),
    "vrth_world_load_vox": (_i, [_p, _s, _i, _i, _i]),
    "vrth_world_load_vox_mem": (_i, [_p, _s, _sz, _i, _i, _i, _pl]),
    "vrth_world_insert": (_i, [_p, _i, _i, _i, _u32, _f, _f, _f]),
    "vrth_world_insert_many": (_i, [_p, _p, _p, _sz, _f, _f, _f]),
    "vrth_world_remove": (_i, [_p, _i, _i, _i]),
    "vrth_world_find": (_i, [_p, _i, _i, _i, _pu32]),
    "vrth_world_ray_cast": (_i, [_p, _pf, _pf, _pi32, _pi]),
    "vrth_world_ray_cast_many": (_long, [_p, _pf, _p, _sz, _p, _p]),
    "vrth_world_texel_count": (_sz, [_p]),
    "vrth_world_flatten": (_i, [_p, _pp, _psz, _pu32]),
    "vrth_world_records": (_i, [_p] + _RECORDS_OUT + [_pu32]),
    "vrth_octree_records": (_i, [_p] + _RECORDS_OUT + [_pu32]),
    "vrth_octree_node_state": (_i, [_p, _pu8, _i]),
    "vrth_octree_subtree_records": (_i, [_p, _pu8, _i] + _RECORDS_OUT),
    "vrth_octree_path_records": (_i, [_p, _pu8, _i, _i, _i, _i] + _RECORDS_OUT),
    "vrth_world_path_records": (_i, [_p, _pu8, _i, _i, _i, _i] + _RECORDS_OUT),
    "vrth_octree_box_records": (_i, [_p, _pu8, _i, _pi32, _pi32] + _RECORDS_OUT),
    "vrth_world_box_records": (_i, [_p, _pu8, _i, _pi32, _pi32] + _RECORDS_OUT),
    "vrth_world_node_state": (_i, [_p, _pu8, _i]),
    "vrth_world_subtree_records": (_i, [_p, _pu8, _i] + _RECORDS_OUT),
    "vrth_free": (None, [_p]),
    "vrth_camera_block": (_i, [_pf, _f, _f, _i, _i, _pf, _pf, _pf, _pf]),
    "vrth_write_vox": (_i, [_s, _i, _i, _i, _p, _sz, _p]),
    "vrth_encode_vox": (_i, [_i, _i, _i, _p, _sz, _p, _pp, _psz]),
    "vrth_make_custom_vox": (_i, [_pp, _psz]),
    "vrth_world_fill_heights": (_i, [_p, _p] + [_i] * 8),
    "vrth_fnv1a64": (_u64, [_p, _sz]),
    "vrth_version": (_s, []),
}

_RAYS = [_p, _sz, _p, _i, _p]              # ctx, n, origins, origin_stride, dirs
_BATCH = _RAYS + [_i, _i, _u32, _u32]      # ... width, mode, first_sample, n_samples
_FRAME = [_p, _i, _i]                      # ctx, width, height
_CAMERA = [_p, _p, _p]                     # inv_projection[16], inv_view[16], camera_pos[4] of the temporal calls

HIP_API = {
    "vrt_create": (_i, [_i, _pp]),
    "vrt_destroy": (None, [_p]),
    "vrt_last_error": (_s, [_p]),
    "vrt_default_params": (None, [C.POINTER(Params)]),
    "vrt_set_params": (_i, [_p, C.POINTER(Params)]),
    "vrt_upload_octree": (_i, [_p, _p, _sz, _u32]),
    "vrt_get_scene_info": (_i, [_p, C.POINTER(SceneInfo)]),
    "vrt_patch_plan": (_i, [_p, _i, _i, _i, _i, C.POINTER(Patch)]),
    "vrt_patch_plan_box": (_i, [_p, _pi32, _pi32, _i, C.POINTER(Patch)]),
    "vrt_patch_apply": (_i, [_p, C.POINTER(Patch), _p, _sz]),
    "vrt_patch_begin": (_i, [_p]),
    "vrt_patch_end": (_i, [_p]),
    "vrt_compact": (_i, [_p]),
    "vrt_upload_records": (_i, [_p, _p, _sz, _u32]),
    "vrt_cast_rays": (_i, _RAYS + [_p, _p, _p]),
    "vrt_cast_rays_device": (_i, _RAYS + [_p, _p, _p, _p]),
    "vrt_find_voxels": (_i, [_p, _sz, _p, _p]),
    "vrt_shade_rays": (_i, _BATCH + [_p, _p]),
    "vrt_shade_rays_device": (_i, _BATCH + [_p, _p, _p]),
    "vrt_accum_begin": (_i, _FRAME + [_u32]),
    "vrt_accum_begin_ex": (_i, _FRAME + [_i, _u32, _u32]),
    "vrt_accum_add": (_i, [_p, _u32, _pu32]),
    "vrt_accum_resolve": (_i, [_p, _p, _p, _p]),
    "vrt_accum_resolve_device": (_i, [_p, _p, _p, _p, _p]),
    "vrt_set_lens": (_i, [_p, _f, _f]),
    "vrt_set_path_depth": (_i, [_p, _i]),
    "vrt_set_sun_disc": (_i, [_p, _f]),
    "vrt_set_emitter_sampling": (_i, [_p, _i]),
    "vrt_emitters": (_long, [_p, _p, _sz]),
    "vrt_set_emitter_importance": (_i, [_p, _i]),
    "vrt_emitter_cdf": (_long, [_p, _p, _sz]),
    "vrt_set_emitter_mis": (_i, [_p, _i]),
    "vrt_accum_begin_adaptive": (_i, _FRAME + [_i, _u32, _u32, _u32, _u32, _u32]),
    "vrt_accum_counts": (_i, [_p, _p]),
    "vrt_accum_keep_hdr": (_i, [_p, _i]),
    "vrt_accum_resolve_hdr": (_i, [_p, _p, _tm, _p, _p]),
    "vrt_accum_resolve_hdr_device": (_i, [_p, _p, _tm, _p, _p, _p]),
    "vrt_shade_rays_hdr": (_i, _BATCH + [_tm, _p, _p, _p]),
    "vrt_shade_rays_hdr_device": (_i, _BATCH + [_u32, _p, _tm, _p, _p, _p, _p]),
    "vrt_set_camera": (_i, [_p, _pf, _pf, _pf]),
    "vrt_dispatch": (_i, _FRAME + [_i, _p, _p]),
    "vrt_dispatch_async": (_i, _FRAME + [_i, _p, _p, _pi]),
    "vrt_dispatch_wait": (_i, [_p, _i]),
    "vrt_host_alloc": (_i, [_p, _sz, _pp]),
    "vrt_host_free": (_i, [_p, _p]),
    "vrt_dispatch_rows": (_i, _FRAME + [_i, _i, _i, _p, _p, _p]),
    "vrt_dispatch_shard": (_i, _FRAME + [_i, _i, _i, _i, _p, _p, _p]),
    "vrt_shard_rows": (_i, [_i, _i, _i, _i]),
    "vrt_dispatch_tiles": (_i, _FRAME + [_i, _i, _i, _i, _p, _p, _p]),
    "vrt_device_alloc": (_i, [_p, _sz, _pp]),
    "vrt_device_free": (_i, [_p, _p]),
    "vrt_device_read": (_i, [_p, _p, _p, _sz, _p]),
    "vrt_device_write": (_i, [_p, _p, _p, _sz, _p]),
    "vrt_device_copy": (_i, [_p, _p, _p, _sz, _p]),
    "vrt_ipc_export": (_i, [_p, _p, _s]),
    "vrt_ipc_open": (_i, [_p, _s, _pp]),
    "vrt_ipc_close": (_i, [_p, _p]),
    "vrt_stream_write_flag": (_i, [_p, _p, _u32, _p]),
    "vrt_stream_wait_flag": (_i, [_p, _p, _u32, _p]),
    "vrt_create_multi": (_i, [_i, _pi, _pp]),
    "vrt_destroy_multi": (None, [_p]),
    "vrt_multi_last_error": (_s, [_p]),
    "vrt_multi_devices": (_i, [_p]),
    "vrt_multi_context": (_p, [_p, _i]),
    "vrt_multi_upload_octree": (_i, [_p, _p, _sz, _u32]),
    "vrt_multi_set_camera": (_i, [_p, _pf, _pf, _pf]),
    "vrt_multi_set_params": (_i, [_p, C.POINTER(Params)]),
    "vrt_multi_frame_alloc": (_i, _FRAME + [_pp, _pp]),
    "vrt_multi_frame_free": (_i, [_p, _p, _p]),
    "vrt_multi_dispatch": (_i, _FRAME + [_i, _i, _i, _p, _p]),
    "vrt_multi_dispatch_frame": (_i, _FRAME + [_i, _p]),
    "vrt_multi_synchronize": (_i, [_p]),
    "vrt_multi_stream": (_p, [_p]),
    "vrt_dispatch_views": (_i, _FRAME + [_i, _i, _i, _i, C.POINTER(View), _i, _p]),
    "vrt_dispatch_timed": (_i, _FRAME + [_i, _i, _i, _p, _p, _p, _i, _pf]),
    "vrt_denoise": (_i, _FRAME + [_p, _p, _p, _p]),
    "vrt_denoise_host": (_i, _FRAME + [_p, _p, _p]),
    "vrt_denoise_hdr": (_i, _FRAME + [_p, _p, _tm, _p, _p, _p]),
    "vrt_denoise_hdr_host": (_i, _FRAME + [_p, _p, _tm, _p, _p]),
    "vrt_accum_resolve_hdr_shown": (_i, [_p, _tm, _p, _p]),
    "vrt_accum_resolve_hdr_shown_device": (_i, [_p, _tm, _p, _p, _p]),
    "vrt_accum_guides": (_i, [_p, _p, _p, _p, _p]),
    "vrt_accum_guides_device": (_i, [_p, _p, _p, _p, _p, _p]),
    "vrt_set_guide_glass": (_i, [_p, _i]),
    "vrt_guide_rays": (_i, _RAYS + [_i, _p, _p, _p, _p]),
    "vrt_guide_rays_device": (_i, _RAYS + [_i, _p, _p, _p, _p, _p]),
    "vrt_filter_default": (None, [_flt]),
    "vrt_filter_hdr": (_i, _FRAME + [_p] * 5 + [_flt, _tm, _p, _p, _p]),
    "vrt_filter_hdr_host": (_i, _FRAME + [_p] * 5 + [_flt, _tm, _p, _p]),
    "vrt_accum_resolve_hdr_filtered": (_i, [_p, _flt, _tm, _p, _p]),
    "vrt_accum_resolve_hdr_filtered_device": (_i, [_p, _flt, _tm, _p, _p, _p]),
    "vrt_filter_var_default": (None, [_fltv]),
    "vrt_filter_hdr_var": (_i, _FRAME + [_p] * 6 + [_fltv, _tm] + [_p] * 4),
    "vrt_filter_hdr_var_host": (_i, _FRAME + [_p] * 6 + [_fltv, _tm] + [_p] * 3),
    "vrt_accum_resolve_hdr_filtered_var": (_i, [_p, _fltv, _tm, _p, _p, _p]),
    "vrt_accum_resolve_hdr_filtered_var_device": (_i, [_p, _fltv, _tm, _p, _p, _p, _p]),
    "vrt_accum_keep_moments": (_i, [_p, _i]),
    "vrt_accum_variance": (_i, [_p, _p]),
    "vrt_accum_variance_device": (_i, [_p, _p, _p]),
    "vrt_temporal_default": (None, [_tmp]),
    "vrt_temporal_hdr": (_i, _FRAME + _CAMERA + [_p] * 5 + [_tmp] + [_p] * 4),
    "vrt_temporal_hdr_host": (_i, _FRAME + _CAMERA + [_p] * 5 + [_tmp] + [_p] * 3),
    "vrt_accum_resolve_hdr_temporal": (_i, [_p, _tmp, _fltv, _tm] + [_p] * 6),
    "vrt_accum_resolve_hdr_temporal_device": (_i, [_p, _tmp, _fltv, _tm] + [_p] * 7),
    "vrt_temporal_mom_default": (None, [_tmpm]),
    "vrt_temporal_hdr_mom": (_i, _FRAME + _CAMERA + [_p] * 6 + [_tmpm] + [_p] * 4),
    "vrt_temporal_hdr_mom_host": (_i, _FRAME + _CAMERA + [_p] * 6 + [_tmpm] + [_p] * 3),
    "vrt_accum_resolve_hdr_temporal_mom": (_i, [_p, _tmpm, _fltv, _tm] + [_p] * 6),
    "vrt_accum_resolve_hdr_temporal_mom_device": (_i, [_p, _tmpm, _fltv, _tm] + [_p] * 7),
    "vrt_upsample_default": (None, [_ups]),
    "vrt_guide_frame": (_i, _FRAME + [_p] * 4),
    "vrt_guide_frame_device": (_i, _FRAME + [_p] * 5),
    "vrt_upsample_hdr": (_i, _FRAME + [_p] * 9 + [_ups, _tm] + [_p] * 4),
    "vrt_upsample_hdr_host": (_i, _FRAME + [_p] * 9 + [_ups, _tm] + [_p] * 3),
    "vrt_accum_resolve_hdr_upsampled": (_i, [_p, _ups, _tm] + [_p] * 3),
    "vrt_accum_resolve_hdr_upsampled_device": (_i, [_p, _ups, _tm] + [_p] * 4),
    "vrt_meter_default": (None, [_mtr]),
    "vrt_meter_resolve": (_i, [_p, _mtr, _exp]),
    "vrt_meter_hdr": (_i, _FRAME + [_p, _mtr, _p, _p, _p]),
    "vrt_meter_hdr_host": (_i, _FRAME + [_p, _mtr, _p, _exp]),
    "vrt_tonemap_hdr": (_i, [_p, _sz, _p, _tm, _p, _p, _p]),
    "vrt_tonemap_hdr_host": (_i, [_p, _sz, _p, _tm, _exp, _p]),
    "vrt_accum_resolve_hdr_metered": (_i, [_p, _mtr, _tm, _exp] + [_p] * 3),
    "vrt_accum_resolve_hdr_metered_device": (_i, [_p, _mtr, _tm] + [_p] * 5),
    "vrt_bloom_default": (None, [_blm]),
    "vrt_bloom_workspace_bytes": (_sz, [_i, _i, _i]),
    "vrt_bloom_hdr": (_i, _FRAME + [_p, _blm, _tm] + [_p] * 5),
    "vrt_bloom_hdr_host": (_i, _FRAME + [_p, _blm, _tm, _exp, _p, _p]),
    "vrt_accum_resolve_hdr_bloomed": (_i, [_p, _mtr, _blm, _tm, _exp, _p, _p]),
    "vrt_accum_resolve_hdr_bloomed_device": (_i, [_p, _mtr, _blm, _tm] + [_p] * 4),
    "vrt_dispatch_frame": (_i, _FRAME + [_i, _p, _p, _p]),
    "vrt_set_profiling": (_i, [_p, _i]),
    "vrt_set_profiling_stride": (_i, [_p, _i]),
    "vrt_profile_read": (_i, [_p, _pf, _i]),
    "vrt_synchronize": (_i, [_p]),
    "vrt_stream": (_p, [_p]),
    "vrt_device": (_i, [_p]),
    "vrt_set_variant": (_i, [_p, _i]),
    "vrt_variant_available": (_i, [_i]),
    "vrt_set_tile_scheduling": (_i, [_p, _i]),
    "vrt_set_option": (_i, [_p, _i, _i]),
    "vrt_get_tile_order": (_long, [_p, _p, _p, _sz]),
    "vrt_set_tile_order": (_i, [_p, _i, _p, _p]),
    "vrt_version": (_s, []),
}

_TREE = [_p, _sz]                          # texels, used_bytes
_WORLD = [_pi32, _pi32]                    # wmin[3], wmax[3]

TEST_API = {   # csrc/test/vrt_test.hip has no header: these rows are kept right by review
    "vrt_test_math": (_i, [_i, _i, _p, _p, _p, _i]),
    "vrt_test_build_layout": (_long, _TREE + [_p, _sz, C.POINTER(SceneInfo)]),
    "vrt_test_patch_check": (_long, _TREE + _TREE + _WORLD + [_i, _i, _i, _p, _sz, _p, _i]),
    "vrt_test_extract_subtree": (_long, _TREE + [_p, _i, _p, _sz]),
    "vrt_test_patch_session_upload": (_p, [_p] + _TREE + [_u32] + _WORLD),
    "vrt_test_patch_session_close": (None, [_p]),
    "vrt_test_patch_session_plan": (_i, [_p, _pi32, _pi32, _i, _p, _p]),
    "vrt_test_patch_session_begin": (_i, [_p]),
    "vrt_test_patch_session_end": (_i, [_p]),
    "vrt_test_patch_session_apply": (_i, [_p, _i, _p, _p, _sz, _p]),
    "vrt_test_patch_session_compact": (_i, [_p]),
    "vrt_test_patch_session_counts": (None, [_p, _p]),
    "vrt_test_patch_session_check": (_i, [_p] + _TREE + [_u32, _p, _sz, _pi32, _i, _p, _p, _p, _sz]),
    "vrt_test_ray_table": (_i, [_p, _i, _i, _p, _p, _p]),
    "vrt_test_root0": (_i, _TREE + _WORLD + [_pi32, _pi32]),
    "vrt_test_view_in_range": (_i, [_p]),
    "vrt_test_wide_find": (_i, _TREE + _WORLD + [_p, _sz, _p, _p]),
    "vrt_test_adaptive_rule": (_i, [_u32, _u64, _u64, _u32, _u32, _u32]),
    "vrt_test_adaptive_rule_device": (_i, [_i, _p, _p, _p, _u32, _u32, _u32, _p, _i]),
    "vrt_test_lens_select": (_i, _TREE + _WORLD + [_f, _pf, _pf, _f, _pi32]),
    "vrt_test_miss_mask": (_i, _TREE + _WORLD + [_f, _pf, _pf, _pf, _i, _i, _p, _pi32]),
    "vrt_test_tile_order": (_i, [_i, _p, _u32, _u32, _p, _p]),
    "vrt_test_tree_is_opaque": (_i, _TREE),
}

_host = None
_hip = None
_test = None


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise VrtError(f"{HOST_LIB} is missing: run __graft_entry__.build() (make -C {CSRC})")
        L = C.CDLL(HOST_LIB)
        for name, (res, args) in HOST_API.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _host = L
    return _host


def hip_lib():
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB):
            raise VrtError(f"{HIP_LIB} is missing: the HIP extension must be built (make -C {CSRC}); "
                           "there is no CPU fallback")
        # One HIP runtime per process: torch bundles its own libamdhip64 (SONAME libamdhip64.so.7). Loading it
        # first lets libvrt_hip.so bind to that copy; the other order ends with two HIP/HSA runtimes and
        # torch reporting "No HIP GPUs are available".
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(HIP_LIB)
        for name, (res, args) in HIP_API.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _hip = L
    return _hip


def test_lib():
    """libvrt_hip_test.so: device probes of the kernels' arithmetic and host-only views of the uploader's layouts, for the
    parity suite (csrc/test/vrt_test.hip). Not part of the product; libvrt_hip.so exports none of it."""
    global _test
    if _test is None:
        if not os.path.exists(TEST_LIB):
            raise VrtError(f"{TEST_LIB} is missing: make -C {CSRC}")
        try:
            import torch  # noqa: F401  (one HIP runtime per process, see hip_lib())
        except ImportError:
            pass
        L = C.CDLL(TEST_LIB)
        for name, (res, args) in TEST_API.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _test = L
    return _test


def available_variants(upto=64):
    """the kernel variants vrt_set_variant() accepts (0, 1, 4, 20, 22)"""
    L = hip_lib()
    return [v for v in range(upto) if L.vrt_variant_available(v)]


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class World:
    """An octree root plus the host API calls around it (octree.hpp / voxReader.hpp)."""

    def __init__(self, world_min=None, world_max=None):
        L = host_lib()
        mn = (C.c_int32 * 3)(*world_min) if world_min is not None else None
        mx = (C.c_int32 * 3)(*world_max) if world_max is not None else None
        self._h = L.vrth_world_create(mn, mx)
        if not self._h:
            raise VrtError("vrth_world_create failed")

    def close(self):
        if getattr(self, "_h", None):
            try:
                host_lib().vrth_world_destroy(self._h)
            except TypeError:  # interpreter shutdown: module globals already cleared
                pass
            self._h = None

    __del__ = close

    def load_vox(self, path, offset=(0, 0, 0)):
        return bool(host_lib().vrth_world_load_vox(self._h, str(path).encode(), *offset))

    def load_vox_bytes(self, data, offset=(0, 0, 0)):
        n = C.c_long(0)
        ok = host_lib().vrth_world_load_vox_mem(self._h, bytes(data), len(data), *offset, C.byref(n))
        return bool(ok), n.value

    def insert(self, x, y, z, rgba, refraction=3.0, illumination=0.0, k=0.0):
        host_lib().vrth_world_insert(self._h, x, y, z, rgba, refraction, illumination, k)

    def insert_many(self, xyz, rgba, refraction=3.0, illumination=0.0, k=0.0):
        xyz = np.ascontiguousarray(xyz, np.int32).reshape(-1, 3)
        rgba = np.ascontiguousarray(rgba, np.uint32).reshape(-1)
        assert xyz.shape[0] == rgba.shape[0]
        host_lib().vrth_world_insert_many(self._h, xyz.ctypes.data, rgba.ctypes.data, xyz.shape[0], refraction,
                                          illumination, k)

    def remove(self, x, y, z):
        host_lib().vrth_world_remove(self._h, x, y, z)

    def find(self, x, y, z):
        out = (C.c_uint32 * 7)()
        host_lib().vrth_world_find(self._h, x, y, z, out)
        f = np.array(out[4:7], np.uint32).view(np.float32)
        return {"coord": tuple(int(np.int32(np.uint32(v))) for v in out[0:3]), "color": int(out[3]),
                "refraction": float(f[0]), "illumination": float(f[1]), "k": float(f[2])}

    def ray_cast(self, origin, direction):
        o = (C.c_float * 3)(*origin)
        d = (C.c_float * 3)(*direction)
        hit = (C.c_int32 * 3)()
        has = C.c_int(0)
        r = host_lib().vrth_world_ray_cast(self._h, o, d, hit, C.byref(has))
        return (tuple(hit), bool(has.value)) if r == 1 else None

    def ray_cast_many(self, origin, dirs):
        """octree_ray_cast for every direction of dirs[n, 3] from one origin -> (hit uint8[n]: 0 miss / 1 voxel / 2 node, coords int32[n, 3])"""
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        hit = np.zeros(d.shape[0], np.uint8)
        coords = np.zeros((d.shape[0], 3), np.int32)
        if host_lib().vrth_world_ray_cast_many(self._h, (C.c_float * 3)(*origin), d.ctypes.data, d.shape[0], hit.ctypes.data,
                                               coords.ctypes.data) < 0:
            raise VrtError("vrth_world_ray_cast_many failed")
        return hit, coords

    def texel_count(self):
        return host_lib().vrth_world_texel_count(self._h)

    def flatten(self):
        """-> (uint8 ndarray with the octree_texture() bytes, tex_dim)"""
        p = C.c_void_p()
        n = C.c_size_t(0)
        d = C.c_uint32(0)
        if host_lib().vrth_world_flatten(self._h, C.byref(p), C.byref(n), C.byref(d)) != 0:
            raise VrtError("vrth_world_flatten failed")
        if not p.value:
            return np.zeros(0, np.uint8), int(d.value)
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,)).copy()
        host_lib().vrth_free(p)
        return arr, int(d.value)

    def records(self):
        """EXTENSION: the device record array straight from the tree -> (uint32[n,2], tex_dim), or None when the
        root is itself a leaf (texel path only)."""
        L = host_lib()
        p, n, d = C.c_void_p(), C.c_size_t(0), C.c_uint32(0)
        r = L.vrth_world_records(self._h, C.byref(p), C.byref(n), C.byref(d))
        if r == -2:
            return None
        if r != 0:
            raise VrtError("vrth_world_records failed")
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n.value, 2)).copy()
        L.vrth_free(p)
        return arr, int(d.value)

    def box_records(self, path, lo, hi):
        """EXTENSION: the sub-tree under the node reached by `path` (child indices from the root) as device records, only the nodes
        that meet the box of voxels [lo, hi] (inclusive) expanded, the rest "keep" records (vrth_world_box_records) -> uint32[n, 2]"""
        L = host_lib()
        p, n = C.c_void_p(), C.c_size_t(0)
        pa = (C.c_uint8 * 16)(*list(path))
        r = L.vrth_world_box_records(self._h, pa, len(path), (C.c_int32 * 3)(*[int(v) for v in lo]), (C.c_int32 * 3)(*[int(v) for v in hi]),
                                     C.byref(p), C.byref(n))
        if r != 0:
            raise VrtError(f"vrth_world_box_records failed ({r})")
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n.value, 2)).copy()
        L.vrth_free(p)
        return arr

    def fill_heights(self, heights, x0, z0, nx, nz, band=8, floor_y=20):
        """config 4 terrain: the reference's generator (src/main.cpp:487-503) over a uint16 height field [size_z, size_x]"""
        h = np.ascontiguousarray(heights, dtype=np.uint16)
        if host_lib().vrth_world_fill_heights(self._h, h.ctypes.data, h.shape[1], h.shape[0], x0, z0, nx, nz, band, floor_y) != 0:
            raise VrtError("vrth_world_fill_heights failed")


def camera_block(pos, yaw, pitch, width, height):
    """Camera(pos, up, yaw, pitch) -> (inv_projection[16], inv_view[16], camera_pos[4], front[3]) float32."""
    ip, iv = np.zeros(16, np.float32), np.zeros(16, np.float32)
    cp, fr = np.zeros(4, np.float32), np.zeros(3, np.float32)
    p = (C.c_float * 3)(*pos)
    if host_lib().vrth_camera_block(p, yaw, pitch, width, height, _fptr(ip), _fptr(iv), _fptr(cp), _fptr(fr)) != 0:
        raise VrtError("vrth_camera_block failed")
    return ip, iv, cp, fr


def encode_vox(size, xyzi, palette=None):
    xyzi = np.ascontiguousarray(xyzi, np.uint8).reshape(-1, 4)
    pal = np.ascontiguousarray(palette, np.uint8).reshape(256, 4) if palette is not None else None
    out, n = C.c_void_p(), C.c_size_t(0)
    r = host_lib().vrth_encode_vox(size[0], size[1], size[2], xyzi.ctypes.data, xyzi.shape[0],
                                   pal.ctypes.data if pal is not None else None, C.byref(out), C.byref(n))
    if r != 0:
        raise VrtError("vrth_encode_vox failed")
    data = C.string_at(out, n.value)
    host_lib().vrth_free(out)
    return data


def make_custom_vox():
    out, n = C.c_void_p(), C.c_size_t(0)
    if host_lib().vrth_make_custom_vox(C.byref(out), C.byref(n)) != 0:
        raise VrtError("vrth_make_custom_vox failed")
    data = C.string_at(out, n.value)
    host_lib().vrth_free(out)
    return data


def fnv1a64(arr):
    a = np.ascontiguousarray(arr)
    return int(host_lib().vrth_fnv1a64(a.ctypes.data, a.nbytes))


def build_layout(texels):
    """Host-only: the device record array the uploader would build -> (uint32[n,2], SceneInfo)."""
    L = test_lib()
    t = np.ascontiguousarray(texels, np.uint8)
    info = SceneInfo()
    n = L.vrt_test_build_layout(t.ctypes.data if t.size else None, t.size, None, 0, C.byref(info))
    if n < 0:
        raise VrtError("malformed texel stream")
    rec = np.zeros((n, 2), np.uint32)
    L.vrt_test_build_layout(t.ctypes.data if t.size else None, t.size, rec.ctypes.data, n, None)
    return rec, info


def patch_check(texels_before, texels_after, voxel, points, world_min=(-1023, -1023, -1023), world_max=(1024, 1024, 1024),
                sparse=False):
    """Host-only (vrt_test_patch_check): patch the layouts of the tree before an edit of `voxel` with the sub-tree of
    the tree after it and compare point lookups with freshly built layouts.
    -> (mismatching points, depth of the node replaced or 0, records appended, wide cells appended, texel count ok)"""
    L = test_lib()
    tb = np.ascontiguousarray(texels_before, np.uint8)
    ta = np.ascontiguousarray(texels_after, np.uint8)
    pts = np.ascontiguousarray(points, np.int32).reshape(-1, 3)
    info = np.zeros(4, np.uint32)
    r = L.vrt_test_patch_check(tb.ctypes.data if tb.size else None, tb.size, ta.ctypes.data if ta.size else None, ta.size,
                                (C.c_int32 * 3)(*world_min), (C.c_int32 * 3)(*world_max), int(voxel[0]), int(voxel[1]),
                                int(voxel[2]), pts.ctypes.data, pts.shape[0], info.ctypes.data, 1 if sparse else 0)
    if r < 0:
        raise VrtError(f"vrt_test_patch_check failed ({r})")
    return int(r), int(info[0]), int(info[1]), int(info[2]), bool(info[3])


def subtree_records(texels, path):
    """Host-only (vrt_test_extract_subtree): the sub-tree under the node `path` (child indices from the root) reaches in a fresh layout of
    a texel stream, as vrt_patch_apply takes it -> uint32[n, 2]. For hand-written streams, which hold what World never emits."""
    L = test_lib()
    t = np.ascontiguousarray(texels, np.uint8)
    pa = (C.c_uint8 * 16)(*list(path))
    n = L.vrt_test_extract_subtree(t.ctypes.data, t.size, pa, len(path), None, 0)
    if n < 0:
        raise VrtError(f"vrt_test_extract_subtree failed ({n})")
    out = np.zeros((n, 2), np.uint32)
    L.vrt_test_extract_subtree(t.ctypes.data, t.size, pa, len(path), out.ctypes.data, n)
    return out


class PatchSession:
    """Host-only (vrt_test_patch_session_*): one record array and one wide layout that take a whole chain of patches, batches and
    compactions by the rules of vrt_patch.cpp, with no device. The editing methods carry Context's names and answers (patch_voxel,
    patch_box, patch_begin, patch_end, compact, upload_octree), so that one driver serves both; check() holds the patched structures
    to a fresh layout of a stream."""

    def __init__(self, texels, tex_dim, world_min=(-1023, -1023, -1023), world_max=(1024, 1024, 1024)):
        self._L = test_lib()
        self._mn, self._mx = (C.c_int32 * 3)(*world_min), (C.c_int32 * 3)(*world_max)
        self._h = None
        self.last = (0, 0, 0)            # of the last patch: it voided the wide layout, re-pointed a cell, changed a root
        self.upload_octree(texels, tex_dim)

    def close(self):
        if getattr(self, "_h", None):
            self._L.vrt_test_patch_session_close(self._h)
            self._h = None

    __del__ = close

    def upload_octree(self, texels, tex_dim):
        t = np.ascontiguousarray(texels, np.uint8)
        h = self._L.vrt_test_patch_session_upload(self._h, t.ctypes.data if t.size else None, t.size, int(tex_dim), self._mn, self._mx)
        if not h:
            raise VrtError("vrt_test_patch_session_upload failed")
        self._h = h

    def _patch(self, world, lo, hi, voxel, max_depth):
        H = host_lib()
        lo3, hi3 = (C.c_int32 * 3)(*[int(v) for v in lo]), (C.c_int32 * 3)(*[int(v) for v in hi])
        depth, path = C.c_int32(0), (C.c_uint8 * 16)()
        while max_depth >= 1:
            if self._L.vrt_test_patch_session_plan(self._h, lo3, hi3, max_depth, C.byref(depth), path) != 0:
                return None
            if H.vrth_world_node_state(world._h, path, depth.value) == 2:
                p, n = C.c_void_p(), C.c_size_t(0)
                if voxel:
                    r = H.vrth_world_path_records(world._h, path, depth.value, int(lo[0]), int(lo[1]), int(lo[2]), C.byref(p), C.byref(n))
                else:
                    r = H.vrth_world_box_records(world._h, path, depth.value, lo3, hi3, C.byref(p), C.byref(n))
                if r != 0:
                    return None
                info = (C.c_uint32 * 3)()
                try:
                    r = self._L.vrt_test_patch_session_apply(self._h, depth.value, path, p, n.value, info)
                finally:
                    H.vrth_free(p)
                if r != 0:
                    raise VrtError(f"vrt_test_patch_session_apply failed ({r})")
                self.last = tuple(int(v) for v in info)
                return depth.value
            max_depth = depth.value - 1
        return None

    def patch_voxel(self, world, x, y, z, max_depth=15):
        return self._patch(world, (x, y, z), (x, y, z), True, max_depth)

    def plan(self, x, y, z, max_depth=15):
        """vrt_patch_plan's answer for a voxel -> the path (a list of child indices), or None"""
        p3 = (C.c_int32 * 3)(int(x), int(y), int(z))
        depth, path = C.c_int32(0), (C.c_uint8 * 16)()
        if self._L.vrt_test_patch_session_plan(self._h, p3, p3, max_depth, C.byref(depth), path) != 0:
            return None
        return list(path[:depth.value])

    def apply(self, path, records):
        """vrt_patch_apply with a caller's sub-tree records -> (it voided the wide layout, re-pointed a cell, changed a root)"""
        r = np.ascontiguousarray(records, np.uint32).reshape(-1, 2)
        info = (C.c_uint32 * 3)()
        self._chk(self._L.vrt_test_patch_session_apply(self._h, len(path), (C.c_uint8 * 16)(*path), r.ctypes.data, r.shape[0], info), "apply")
        self.last = tuple(int(v) for v in info)
        return self.last

    def patch_box(self, world, lo, hi, max_depth=15):
        return self._patch(world, lo, hi, False, max_depth)

    def _chk(self, r, what):
        if r != 0:
            raise VrtError(f"vrt_test_patch_session_{what} failed ({r})")

    def patch_begin(self):
        self._chk(self._L.vrt_test_patch_session_begin(self._h), "begin")

    def patch_end(self):
        self._chk(self._L.vrt_test_patch_session_end(self._h), "end")

    def compact(self):
        self._chk(self._L.vrt_test_patch_session_compact(self._h), "compact")

    def counts(self):
        """-> dict(n_records, compactions, peak_records, n_cells)"""
        out = np.zeros(4, np.uint64)
        self._L.vrt_test_patch_session_counts(self._h, out.ctypes.data)
        return dict(n_records=int(out[0]), compactions=int(out[1]), peak_records=int(out[2]), n_cells=int(out[3]))

    def scene_info(self):
        return {"n_records": self.counts()["n_records"]}

    def check(self, texels, tex_dim, points, eye, stale=False):
        """the patched structures against a fresh layout of `texels` -> dict; list, cdf: the patched array's emitter list and thresholds;
        repointed: the last patch re-pointed a cell or a root and the layout was not rebuilt since; stale: with that cell or root at
        its old value (what bad_cells is there to notice)"""
        t = np.ascontiguousarray(texels, np.uint8)
        pts = np.ascontiguousarray(points, np.int32).reshape(-1, 3)
        out = np.zeros(28, np.uint32)
        probe = np.zeros(28, np.uint32)
        args = (self._h, t.ctypes.data if t.size else None, t.size, int(tex_dim), pts.ctypes.data if len(pts) else None, len(pts),
                (C.c_int32 * 3)(*[int(v) for v in eye]), 1 if stale else 0)
        self._chk(self._L.vrt_test_patch_session_check(*args, probe.ctypes.data, None, None, 0), "check")
        n = int(probe[5])
        lst, cdf = np.zeros((n, 4), np.int32), np.zeros(n, np.uint32)
        self._chk(self._L.vrt_test_patch_session_check(*args, out.ctypes.data, lst.ctypes.data if n else None, cdf.ctypes.data if n else None, n),
                  "check")
        o = [int(v) for v in out]
        return dict(bad_cells=o[0], bad_records=o[1], opaque=(bool(o[2]), bool(o[3])), emitters_equal=bool(o[4]), n_emitters=(o[5], o[6]),
                    wide=bool(o[7]), root0=(tuple(o[8:14]), tuple(o[14:20])), texels=(o[20], o[21]), tex_dim=(o[22], o[23]),
                    live_records=o[24], n_records=o[25], fresh_records=o[26], repointed=bool(o[27]), list=lst, cdf=cdf)


def ray_table(inv_projection, width, height):
    """Host-only: the per-column / per-row ray-generation table of a projection (vrt_test_ray_table)
    -> (x[width], y[height], z) float32, or None when the projection has no table."""
    L = test_lib()
    m = np.ascontiguousarray(inv_projection, np.float32).reshape(16)
    x, y, z = np.zeros(width, np.float32), np.zeros(height, np.float32), np.zeros(1, np.float32)
    r = L.vrt_test_ray_table(m.ctypes.data, width, height, x.ctypes.data, y.ctypes.data, z.ctypes.data)
    if r < 0:
        raise VrtError(f"vrt_test_ray_table failed ({r})")
    return (x, y, float(z[0])) if r == 1 else None


def root0_choice(texels, eye, world_min=(-1023, -1023, -1023), world_max=(1024, 1024, 1024)):
    """Host-only (vrt_test_root0): (root0_only, log2 side of the root chosen for this eye, its minimum corner (3), log2 side
    of build_wide()'s root), or None when the scene has no wide form."""
    L = test_lib()
    t = np.ascontiguousarray(texels, np.uint8)
    out = (C.c_int32 * 6)()
    r = L.vrt_test_root0(t.ctypes.data if t.size else None, t.size, (C.c_int32 * 3)(*world_min), (C.c_int32 * 3)(*world_max),
                          (C.c_int32 * 3)(*[int(v) for v in eye]), out)
    if r == -5:
        return None
    if r != 0:
        raise VrtError(f"vrt_test_root0 failed ({r})")
    return bool(out[0]), int(out[1]), (int(out[2]), int(out[3]), int(out[4])), int(out[5])

def adaptive_rule(n, s, q, min_samples, max_samples, tolerance):
    """Host probe (vrt_test_adaptive_rule): is a pixel with n samples, S = s and Q = q active under the adaptive accumulation's
    stopping rule (include/vrt.h vrt_accum_begin_adaptive)? The function the kernels evaluate, compiled for the host."""
    L = test_lib()
    return L.vrt_test_adaptive_rule(int(n), int(s), int(q), int(min_samples), int(max_samples), int(tolerance)) == 1


def adaptive_rule_device(n, s, q, min_samples, max_samples, tolerance, device=0):
    """Device probe (vrt_test_adaptive_rule_device): the same rule on the GPU for arrays of states -> bool array"""
    L = test_lib()
    n = np.ascontiguousarray(n, np.uint32)
    s = np.ascontiguousarray(s, np.uint64)
    q = np.ascontiguousarray(q, np.uint64)
    assert n.shape == s.shape == q.shape and n.ndim == 1
    out = np.zeros(n.shape, np.uint32)
    r = L.vrt_test_adaptive_rule_device(device, n.ctypes.data, s.ctypes.data, q.ctypes.data, int(min_samples), int(max_samples),
                                        int(tolerance), out.ctypes.data, n.size)
    if r != 0:
        raise VrtError(f"vrt_test_adaptive_rule_device failed ({r})")
    return out != 0


def lens_choice(texels, cam_pos, inv_view, aperture, voxel_scale=1.0, world_min=(-1023, -1023, -1023),
                world_max=(1024, 1024, 1024)):
    """Host-only (vrt_test_lens_select): which side of each one-eye shortcut an accumulation with a thin lens of this aperture
    takes -> dict(box_valid, eye_shared, first_shared, no_medium, empty, lo, hi, root_shift); root_shift -1: no wide form."""
    L = test_lib()
    t = np.ascontiguousarray(texels, np.uint8)
    cp = np.ascontiguousarray(cam_pos, np.float32)
    iv = np.ascontiguousarray(inv_view, np.float32)
    out = (C.c_int32 * 12)()
    r = L.vrt_test_lens_select(t.ctypes.data if t.size else None, t.size, (C.c_int32 * 3)(*world_min), (C.c_int32 * 3)(*world_max),
                               float(voxel_scale), _fptr(cp), _fptr(iv), float(aperture), out)
    if r != 0:
        raise VrtError(f"vrt_test_lens_select failed ({r})")
    return dict(box_valid=bool(out[0]), eye_shared=bool(out[1]), first_shared=bool(out[2]), no_medium=bool(out[3]),
                empty=bool(out[4]), lo=tuple(out[5:8]), hi=tuple(out[8:11]), root_shift=int(out[11]))


def miss_mask(texels, inv_proj, inv_view, cam_pos, width, height, voxel_scale=1.0, world_min=(-1023, -1023, -1023),
              world_max=(1024, 1024, 1024)):
    """Host-only (vrt_test_miss_mask): the miss-tile mask the dispatcher gives this view (VRT_OPT_MISS_TILES) -> (mask, boxes,
    whole_view) with mask a ((height + 7) // 8, (width + 7) // 8) uint8 array, 1 = traced, 0 = forward-pointing rays miss; or None
    when the view gets no mask."""
    L = test_lib()
    t = np.ascontiguousarray(texels, np.uint8)
    ip = np.ascontiguousarray(inv_proj, np.float32).reshape(-1)
    iv = np.ascontiguousarray(inv_view, np.float32).reshape(-1)
    cp = np.zeros(4, np.float32)
    cp[:len(cam_pos)] = np.asarray(cam_pos, np.float32).reshape(-1)[:4]
    mask = np.zeros(((height + 7) // 8, (width + 7) // 8), np.uint8)
    stats = (C.c_int32 * 2)()
    r = L.vrt_test_miss_mask(t.ctypes.data if t.size else None, t.size, (C.c_int32 * 3)(*world_min), (C.c_int32 * 3)(*world_max),
                             float(voxel_scale), _fptr(ip), _fptr(iv), _fptr(cp), int(width), int(height), mask.ctypes.data, stats)
    if r < 0:
        raise VrtError(f"vrt_test_miss_mask failed ({r})")
    if r == 0:
        return None
    return mask, int(stats[0]), bool(stats[1])


def test_tile_order(tile_ticks, wave_slots, device=0):
    """Device probe (vrt_test_tile_order): the feedback scheduler's order kernel on synthetic per-tile ticks (4 per group) ->
    (order of the groups, how many groups at its head the general full path tracer would trace as part-tile waves)."""
    L = test_lib()
    t = np.ascontiguousarray(tile_ticks, np.uint32).reshape(-1)
    assert t.size % 4 == 0
    n = t.size // 4
    order = np.zeros(n, np.uint32)
    split = np.zeros(1, np.uint32)
    r = L.vrt_test_tile_order(device, t.ctypes.data, n, wave_slots, order.ctypes.data, split.ctypes.data)
    if r:
        raise VrtError(f"vrt_test_tile_order failed ({r})")
    return order, int(split[0])



def tree_is_opaque(texels):
    """Host-only (vrt_test_tree_is_opaque): may VRT_MODE_FULL run without a ray stack on this tree (for an eye in empty space)?"""
    L = test_lib()
    t = np.ascontiguousarray(texels, np.uint8)
    r = L.vrt_test_tree_is_opaque(t.ctypes.data if t.size else None, t.size)
    if r < 0:
        raise VrtError(f"vrt_test_tree_is_opaque failed ({r})")
    return r == 1


def view_in_range(inv_view):
    m = np.ascontiguousarray(inv_view, np.float32).reshape(16)
    return test_lib().vrt_test_view_in_range(m.ctypes.data) == 1


def wide_find(texels, points, world_min=(-1023, -1023, -1023), world_max=(1024, 1024, 1024)):
    """Host-only: point queries through the wide (64-cell) layout the default kernels read.
    -> (uint32[n,8] = w0, w1, mn[3], mx[3], (wide nodes, roots)), or None when the scene has no wide form."""
    L = test_lib()
    t = np.ascontiguousarray(texels, np.uint8)
    pts = np.ascontiguousarray(points, np.int32).reshape(-1, 3)
    out = np.zeros((pts.shape[0], 8), np.uint32)
    stats = np.zeros(2, np.uint32)
    r = L.vrt_test_wide_find(t.ctypes.data if t.size else None, t.size, (C.c_int32 * 3)(*world_min),
                              (C.c_int32 * 3)(*world_max), pts.ctypes.data, pts.shape[0], out.ctypes.data,
                              stats.ctypes.data)
    if r == -5:
        return None
    if r != 0:
        raise VrtError(f"vrt_test_wide_find failed ({r})")
    return out, (int(stats[0]), int(stats[1]))


# ---- The pieces the HDR post chain's methods are made of (Context._tonemap .. accum_resolve_hdr_temporal_mom_device)
def _ref(struct):
    """a struct or None -> byref or the NULL pointer (the byref keeps the struct alive)"""
    return None if struct is None else C.byref(struct)


def _addr(a):
    """an optional host array -> its address or NULL; the caller holds the array while the library reads it"""
    return None if a is None else a.ctypes.data


_GUIDE_PLANES = {"normal": (3,), "albedo": (4,), "depth": (), "coverage": ()}   # accum_guides' planes: the floats per pixel past [H,W]


def _planes(rgb, guides, keys):
    """rgb[H,W,3] and the planes of `guides` named in `keys` as contiguous float32 arrays of matching shapes -> (rgb, [planes], H,
    W); ValueError otherwise"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    g = [np.ascontiguousarray(guides[k], np.float32) for k in keys]
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"expected rgb[H,W,3], got {rgb.shape}")
    h, w = rgb.shape[:2]
    if any(p.shape != (h, w) + _GUIDE_PLANES[k] for p, k in zip(g, keys)):
        want = ", ".join("[H,W" + "".join(f",{c}" for c in _GUIDE_PLANES[k]) + "]" for k in keys)
        raise ValueError(f"expected guides {want} for H, W = {h}, {w}; got {', '.join(str(p.shape) for p in g)}")
    return rgb, g, h, w


def _variance_plane(variance, h, w):
    """the optional variance[H,W] -> a contiguous float32 array or None; ValueError for another shape"""
    if variance is None:
        return None
    variance = np.ascontiguousarray(variance, np.float32)
    if variance.shape != (h, w):
        raise ValueError(f"expected variance[H,W] for H, W = {h}, {w}; got {variance.shape}")
    return variance


def _history_planes(history, prev_camera, h, w):
    """the optional history[3,H,W,4], which needs prev_camera -> a contiguous float32 array or None; ValueError otherwise"""
    if history is None:
        return None
    history = np.ascontiguousarray(history, np.float32)
    if history.shape != (3, h, w, 4):
        raise ValueError(f"expected history[3,H,W,4] for H, W = {h}, {w}; got {history.shape}")
    if prev_camera is None:
        raise ValueError("a history needs prev_camera")
    return history


def _zeros(h, w, *kinds):
    """zero-filled output planes by kind"""
    shapes = {"history": ((3, h, w, 4), np.float32), "rgb": ((h, w, 3), np.float32), "rgba8": ((h, w, 4), np.uint8),
              "plane": ((h, w), np.float32), "mask": ((h, w), np.uint8)}
    return [np.zeros(*shapes[k]) for k in kinds]


class Context:
    """One GPU's dispatch context (vrt_ctx)."""

    def __init__(self, device=0):
        L = hip_lib()
        h = C.c_void_p()
        r = L.vrt_create(device, C.byref(h))
        if r != 0:
            raise VrtError(f"vrt_create({device}) failed ({r}): {L.vrt_last_error(None).decode()}")
        self._h = h
        self._L = L

    def close(self):
        if getattr(self, "_h", None) and not getattr(self, "borrowed", False):
            self._L.vrt_destroy(self._h)
        self._h = None

    __del__ = close

    def _chk(self, r):
        if r != 0:
            raise VrtError(f"vrt error {r}: {self._L.vrt_last_error(self._h).decode()}")

    def upload_octree(self, texels, tex_dim):
        t = np.ascontiguousarray(texels, np.uint8)
        self._chk(self._L.vrt_upload_octree(self._h, t.ctypes.data if t.size else None, t.size, tex_dim))

    def upload_records(self, records, tex_dim):
        """EXTENSION: upload the record array World.records() returns (no texel stream, no 2^23-texel limit)."""
        r = np.ascontiguousarray(records, np.uint32).reshape(-1, 2)
        self._chk(self._L.vrt_upload_records(self._h, r.ctypes.data, r.shape[0], tex_dim))

    def scene_info(self):
        info = SceneInfo()
        self._chk(self._L.vrt_get_scene_info(self._h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in SceneInfo._fields_}

    def set_camera(self, inv_proj, inv_view, cam_pos):
        ip = np.ascontiguousarray(inv_proj, np.float32)
        iv = np.ascontiguousarray(inv_view, np.float32)
        cp = np.ascontiguousarray(cam_pos, np.float32)
        self._chk(self._L.vrt_set_camera(self._h, _fptr(ip), _fptr(iv), _fptr(cp)))

    def default_params(self):
        p = Params()
        self._L.vrt_default_params(C.byref(p))
        return p

    def set_params(self, p):
        self._chk(self._L.vrt_set_params(self._h, C.byref(p)))

    def set_variant(self, v):
        self._chk(self._L.vrt_set_variant(self._h, v))

    def dispatch(self, width, height, mode=MODE_PRIMARY):
        """Synchronous frame into host arrays -> (rgba8[H,W,4] uint8, id_dist[H,W,2] int32)."""
        rgba = np.zeros((height, width, 4), np.uint8)
        idd = np.zeros((height, width, 2), np.int32)
        self._chk(self._L.vrt_dispatch(self._h, width, height, mode, rgba.ctypes.data, idd.ctypes.data))
        return rgba, idd

    def dispatch_rows(self, width, height, row_begin, row_end, mode, d_rgba, d_id, stream=None):
        self._chk(self._L.vrt_dispatch_rows(self._h, width, height, row_begin, row_end, mode, d_rgba, d_id, stream))

    def dispatch_shard(self, width, height, tile_rows, shard, n_shards, mode, d_rgba, d_id, stream=None):
        self._chk(self._L.vrt_dispatch_shard(self._h, width, height, tile_rows, shard, n_shards, mode, d_rgba, d_id,
                                             stream))

    def host_alloc(self, shape, dtype):
        """a page-locked numpy array (vrt_host_alloc); release with host_free(arr)"""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._chk(self._L.vrt_host_alloc(self._h, n, C.byref(p)))
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n,)).view(dtype).reshape(shape)
        return arr

    def host_free(self, arr):
        self._chk(self._L.vrt_host_free(self._h, arr.ctypes.data))

    def dispatch_async(self, width, height, mode, out_rgba, out_id):
        t = C.c_int(-1)
        self._chk(self._L.vrt_dispatch_async(self._h, width, height, mode, out_rgba.ctypes.data if out_rgba is not None else None,
                                             out_id.ctypes.data if out_id is not None else None, C.byref(t)))
        return t.value

    def dispatch_wait(self, ticket):
        self._chk(self._L.vrt_dispatch_wait(self._h, ticket))

    def dispatch_tiles(self, width, height, tile_rows, shard, n_shards, mode, d_frame_rgba, d_frame_id, stream=None):
        """the shard's row tiles at their place in a FULL frame (local, peer or IPC-mapped device memory)"""
        self._chk(self._L.vrt_dispatch_tiles(self._h, width, height, tile_rows, shard, n_shards, mode, d_frame_rgba, d_frame_id, stream))

    def device_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self._L.vrt_device_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def device_free(self, ptr):
        self._chk(self._L.vrt_device_free(self._h, ptr))

    def device_read(self, ptr, shape, dtype, stream=None):
        out = np.empty(shape, dtype)
        self._chk(self._L.vrt_device_read(self._h, ptr, out.ctypes.data, out.nbytes, stream))
        return out

    def device_write(self, ptr, arr, stream=None):
        a = np.ascontiguousarray(arr)
        self._chk(self._L.vrt_device_write(self._h, ptr, a.ctypes.data, a.nbytes, stream))

    def device_copy(self, dst, src, nbytes, stream=None):
        """asynchronous device-to-device copy on `stream`; either side may be an IPC mapping of another rank's memory"""
        self._chk(self._L.vrt_device_copy(self._h, C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), C.c_void_p(stream)))

    def ipc_export(self, ptr):
        h = C.create_string_buffer(64)
        self._chk(self._L.vrt_ipc_export(self._h, ptr, h))
        return h.raw

    def ipc_open(self, handle):
        p = C.c_void_p()
        self._chk(self._L.vrt_ipc_open(self._h, bytes(handle), C.byref(p)))
        return p.value

    def ipc_close(self, ptr):
        self._chk(self._L.vrt_ipc_close(self._h, ptr))

    def stream_write_flag(self, d_flag, value, stream=None):
        self._chk(self._L.vrt_stream_write_flag(self._h, d_flag, value, stream))

    def stream_wait_flag(self, d_flag, value, stream=None):
        self._chk(self._L.vrt_stream_wait_flag(self._h, d_flag, value, stream))

    def dispatch_timed(self, width, height, row_begin, row_end, mode, d_rgba, d_id, iters, stream=None):
        ms = (C.c_float * iters)()
        self._chk(self._L.vrt_dispatch_timed(self._h, width, height, row_begin, row_end, mode, d_rgba, d_id, stream,
                                             iters, ms))
        return np.array(ms, np.float32)

    def set_profiling(self, max_launches, every=1):
        self._chk(self._L.vrt_set_profiling_stride(self._h, every))
        self._chk(self._L.vrt_set_profiling(self._h, max_launches))

    def profile_read(self, cap=4096):
        ms = (C.c_float * cap)()
        n = self._L.vrt_profile_read(self._h, ms, cap)
        if n < 0:
            self._chk(n)
        return np.array(ms[:n], np.float32)

    def cast_rays(self, origins, dirs, box=WORLD_BOX):
        """octree_ray_cast + get_placement_coord on the device tree (vrt_cast_rays). origins: (n, 3), or (3,) shared by
        all rays; dirs: (n, 3); box: the worldMin / worldMax pair. -> (hit bool[n], coord int32[n, 3], place int32[n, 3],
        leaf uint32[n, 2], steps int32[n]); coord and place are -1 where nothing is hit."""
        o, stride, d, bmin, bmax = query_ray_args(origins, dirs, box)
        n = d.shape[0]
        out = np.zeros(n, RAY_HIT_DTYPE)
        L = self._L
        self._chk(L.vrt_cast_rays(self._h, n, o.ctypes.data if n else None, stride, d.ctypes.data if n else None,
                                  bmin.ctypes.data, bmax.ctypes.data, out.ctypes.data if n else None))
        return out["hit"] != 0, out["coord"].copy(), out["place"].copy(), out["leaf"].copy(), out["steps"].copy()

    def cast_rays_device(self, n, d_origins, origin_stride, d_dirs, d_out, box=WORLD_BOX, stream=None):
        """vrt_cast_rays_device: DEVICE buffers (d_out receives n vrt_ray_hit, RAY_HIT_DTYPE), enqueued on `stream`"""
        b = _real_array(box, "box")
        if b.shape != (2, 3):
            raise ValueError(f"box: expected ((x, y, z), (x, y, z)), got shape {b.shape}")
        b = np.ascontiguousarray(b, np.float32)
        _check_int("n", n, "an integer in [0, 2^31)", 0, 2 ** 31 - 1)
        if origin_stride not in (0, 3):
            raise ValueError(f"origin_stride: expected 0 (one shared origin) or 3, got {origin_stride!r}")
        L = self._L
        self._chk(L.vrt_cast_rays_device(self._h, n, d_origins, origin_stride, d_dirs, b[0].ctypes.data, b[1].ctypes.data,
                                         d_out, stream))

    def find_voxels(self, coords):
        """octree_find as isVoxelSolid reads it, on the device tree (vrt_find_voxels). coords: int (n, 3)
        -> (present bool[n], leaf uint32[n, 2])."""
        c = query_point_args(coords)
        n = c.shape[0]
        out = np.zeros((n, 3), np.uint32)
        L = self._L
        self._chk(L.vrt_find_voxels(self._h, n, c.ctypes.data if n else None, out.ctypes.data if n else None))
        return out[:, 0] != 0, out[:, 1:].copy()

    def shade_rays(self, origins, dirs, mode=MODE_FULL, width=None, first_sample=0, n_samples=1):
        """pathTrace for the caller's own rays (vrt_shade_rays). origins: (n, 3), or (3,) shared by all rays; dirs: (n, 3),
        used as given; width: the batch as an image of that width for the random numbers (None: n); the mean of samples
        first_sample .. first_sample + n_samples - 1 -> (rgba8 uint8[n, 4], id_dist int32[n, 2])."""
        o, stride, d = shade_ray_args(origins, dirs)
        n = d.shape[0]
        rgba = np.zeros((n, 4), np.uint8)
        idd = np.zeros((n, 2), np.int32)
        w = max(n, 1) if width is None else int(width)
        self._chk(self._L.vrt_shade_rays(self._h, n, o.ctypes.data if n else None, stride, d.ctypes.data if n else None, w,
                                         int(mode), int(first_sample) & 0xFFFFFFFF, int(n_samples), rgba.ctypes.data,
                                         idd.ctypes.data))
        return rgba, idd

    def shade_rays_device(self, n, d_origins, origin_stride, d_dirs, d_rgba, d_id, mode=MODE_FULL, width=None, first_sample=0,
                          n_samples=1, stream=None):
        """vrt_shade_rays_device: DEVICE buffers (d_rgba: n x 4 bytes, d_id: n x 2 int32, either may be None), enqueued on
        `stream`"""
        _check_int("n", n, "an integer in [0, 2^30]", 0, 2 ** 30)
        w = max(int(n), 1) if width is None else int(width)
        self._chk(self._L.vrt_shade_rays_device(self._h, int(n), d_origins, int(origin_stride), d_dirs, w, int(mode),
                                                int(first_sample) & 0xFFFFFFFF, int(n_samples), d_rgba, d_id, stream))

    def accum_begin(self, width, height, first_sample=0, mode=MODE_FULL, jitter=False, adaptive=None, hdr=False, moments=False):
        """(Re)start the progressive accumulation of `mode` at sample index `first_sample` (vrt_accum_begin_ex); jitter=True
        moves each sample's ray inside the pixel (VRT_ACCUM_JITTER: anti-aliased frames). adaptive=(min_samples, max_samples,
        tolerance) makes it adaptive (vrt_accum_begin_adaptive): accum_add then adds rounds, in which only the pixels the
        stopping rule keeps active take a sample; accum_counts() reports them. hdr=True keeps float64 sums of the samples'
        unclamped colours too (vrt_accum_keep_hdr, set for this begin): accum_resolve_hdr() resolves them. moments=True (needs
        hdr=True) keeps two more float64 sums per pixel, of the samples' luminance and its square (vrt_accum_keep_moments, set for
        this begin): accum_variance() resolves them, and accum_resolve_hdr_filtered_var() takes that plane."""
        _check_flag("hdr", hdr, "a bool")
        _check_flag("moments", moments, "a bool")
        if moments and not hdr:
            raise ValueError("moments: the luminance moments ride with the HDR sums (hdr=True)")
        _check_int("mode", mode, "MODE_PRIMARY, MODE_PRIMARY_SHADOW or MODE_FULL", MODE_PRIMARY, MODE_FULL)
        _check_flag("jitter", jitter, "a bool")
        for name, v in (("width", width), ("height", height)):
            _check_int(name, v, "a positive integer", 1, 1 << 30)
        if width * height > 1 << 30:
            raise ValueError(f"width * height: at most 2^30 pixels, got {width * height}")
        _check_int("first_sample", first_sample, "an integer in [0, 2^32)", 0, (1 << 32) - 1)
        if adaptive is not None:
            if not isinstance(adaptive, (tuple, list)) or len(adaptive) != 3:
                raise ValueError(f"adaptive: expected None or (min_samples, max_samples, tolerance), got {adaptive!r}")
            names = ("min_samples", "max_samples", "tolerance")
            lo, hi, tol = (_check_int(f"adaptive {name}", v, "an integer") for name, v in zip(names, adaptive))
            if not 2 <= lo <= hi <= 1 << 24:
                raise ValueError(f"adaptive: need 2 <= min_samples <= max_samples <= 2^24, got {adaptive!r}")
            _check_int("adaptive tolerance", tol, "an integer in [0, 65535]", 0, 65535)
            self._chk(self._L.vrt_accum_keep_hdr(self._h, 1 if hdr else 0))
            self._chk(self._L.vrt_accum_keep_moments(self._h, 1 if moments else 0))
            self._chk(self._L.vrt_accum_begin_adaptive(self._h, int(width), int(height), int(mode), int(first_sample),
                                                       ACCUM_JITTER if jitter else 0, lo, hi, tol))
        else:
            self._chk(self._L.vrt_accum_keep_hdr(self._h, 1 if hdr else 0))
            self._chk(self._L.vrt_accum_keep_moments(self._h, 1 if moments else 0))
            self._chk(self._L.vrt_accum_begin_ex(self._h, int(width), int(height), int(mode), int(first_sample),
                                                 ACCUM_JITTER if jitter else 0))
        self._accum_shape = (int(height), int(width))

    def accum_counts(self):
        """An adaptive accumulation's per-pixel sample counts and how many pixels are still active (vrt_accum_counts)
        -> (counts uint32[H, W], active int)."""
        counts = np.zeros(self._accum_hw("accum_counts"), np.uint32)
        r = self._L.vrt_accum_counts(self._h, counts.ctypes.data)
        self._chk(min(r, 0))
        return counts, int(r)

    def set_lens(self, aperture, focus_distance):
        """Thin lens for the progressive accumulation (vrt_set_lens): lens radius `aperture` (0: a pinhole) and the distance of
        the plane of focus along the view axis, both in world units. Frames stay pinhole."""
        aperture = _check_f32("aperture", aperture, lambda x: x >= 0.0, "finite and >= 0")
        focus_distance = _check_f32("focus_distance", focus_distance, _positive, "finite and > 0")
        self._chk(self._L.vrt_set_lens(self._h, aperture, focus_distance))

    def set_path_depth(self, depth):
        """Path depth of the samples of MODE_FULL in accumulations and ray batches (vrt_set_path_depth): an integer in
        1..MAX_PATH_DEPTH, default 1 (the shader's one bounce). An opaque, non-emissive hit of a ray of depth d < depth casts a
        shadow ray, adds the direct term and bounces again; at d == depth it adds the shader's ambient term. Frames
        (dispatch*) stay the shader at any setting; the primary modes ignore it."""
        _check_int("depth", depth, f"an integer in [1, {MAX_PATH_DEPTH}]")   # the range is the library's to refuse
        self._chk(self._L.vrt_set_path_depth(self._h, int(depth)))
        self._path_depth = int(depth)

    @property
    def path_depth(self):
        """The path depth set_path_depth() last set through this object (1 until then). A copy kept in Python: the C-ABI has a
        setter only, so a vrt_set_path_depth call made past this wrapper is not seen here."""
        return getattr(self, "_path_depth", 1)

    def set_sun_disc(self, tan_radius):
        """Sun disc of the samples of MODE_FULL in accumulations and ray batches (vrt_set_sun_disc): the tangent of the sun's
        angular radius, a finite number in [0, 1], default 0 (the shader's point sun; the real sun is about 0.00465). Above 0 every
        vertex that casts a shadow ray draws its own light direction on the disc: soft shadows. Frames (dispatch*) and the primary
        modes ignore it. A value outside the range raises (VRT_E_INVALID) and the previous one holds."""
        if isinstance(tan_radius, bool) or not isinstance(tan_radius, (int, float, np.integer, np.floating)):
            raise ValueError(f"tan_radius: expected a number in [0, 1], got {tan_radius!r}")
        self._chk(self._L.vrt_set_sun_disc(self._h, float(tan_radius)))
        self._sun_disc = float(np.float32(tan_radius))

    @property
    def sun_disc(self):
        """The value set_sun_disc() last set through this object (0.0 until then), as the float32 the library holds. A copy kept
        in Python: the C-ABI has a setter only."""
        return getattr(self, "_sun_disc", 0.0)

    def set_emitter_sampling(self, on):
        """Emitter sampling of the samples of MODE_FULL in accumulations and ray batches (vrt_set_emitter_sampling): 0 / False
        (default) or 1 / True. On, every vertex that casts a shadow ray also connects to a random point of the emitter list
        (emitters()) and bounce rays that hit an emissive voxel add nothing: the same expectation, far less variance indoors. Frames
        (dispatch*) and the primary modes ignore it. Any other value raises (VRT_E_INVALID) and the previous one holds."""
        _check_flag("emitter sampling", on, "0 or 1", bools=bool)
        self._chk(self._L.vrt_set_emitter_sampling(self._h, int(on)))
        self._emitter_sampling = bool(on)

    @property
    def emitter_sampling(self):
        """The value set_emitter_sampling() last set through this object (False until then). A copy kept in Python: the C-ABI has
        a setter only."""
        return getattr(self, "_emitter_sampling", False)

    def emitters(self):
        """The emitter list of the current tree (vrt_emitters) -> int32[N, 4]: lo.x, lo.y, lo.z, size of every leaf with alpha and
        illumination above 0, ascending by (lo.x, lo.y, lo.z). Above MAX_EMITTERS entries the library holds none: that raises."""
        n = self._L.vrt_emitters(self._h, None, 0)
        if n < 0:
            self._chk(n)
        if n > MAX_EMITTERS:
            raise VrtError(f"emitters: the tree has {n} emitters, more than MAX_EMITTERS")
        out = np.zeros((n, 4), np.int32)
        if n:
            got = self._L.vrt_emitters(self._h, out.ctypes.data, n)
            if got < 0:
                self._chk(got)
            assert got == n
        return out

    def set_emitter_importance(self, mode):
        """How a vertex picks from the emitter list where emitter sampling is on (vrt_set_emitter_importance): EMIT_UNIFORM (0,
        default), one of N emitters and one of six faces, or EMIT_POWER (1), the emitter in proportion to its power (emitter_cdf())
        and the face among those turned towards the vertex: the same expectation, less variance where emitters differ much. Read
        only where sampling is on and the list is not empty. Any other value raises (VRT_E_INVALID) and the previous one holds."""
        _check_int("emitter importance", mode, "EMIT_UNIFORM (0) or EMIT_POWER (1)", EMIT_UNIFORM, EMIT_POWER)
        self._chk(self._L.vrt_set_emitter_importance(self._h, int(mode)))
        self._emitter_importance = int(mode)

    @property
    def emitter_importance(self):
        """The value set_emitter_importance() last set through this object (EMIT_UNIFORM until then). A copy kept in Python: the
        C-ABI has a setter only."""
        return getattr(self, "_emitter_importance", EMIT_UNIFORM)

    def set_emitter_mis(self, enable):
        """Weigh the emitter connection against the bounce ray by the balance heuristic (vrt_set_emitter_mis): 0 / False (default) or
        1 / True. Both keep their sample, so a vertex next to an emitter no longer carries an unbounded connection weight: the same
        expectation, no fireflies where emitters touch surfaces. Read only where sampling is on, the list is not empty and the mode
        is EMIT_POWER. Any other value raises before the library is touched and the previous one holds."""
        _check_flag("emitter MIS", enable, "0, 1 or a bool", bools=bool)
        self._chk(self._L.vrt_set_emitter_mis(self._h, int(enable)))
        self._emitter_mis = int(enable)

    @property
    def emitter_mis(self):
        """The value set_emitter_mis() last set through this object (0 until then). A copy kept in Python: the C-ABI has a setter
        only."""
        return getattr(self, "_emitter_mis", 0)

    def emitter_cdf(self):
        """The thresholds by which EMIT_POWER picks from the emitter list (vrt_emitter_cdf) -> uint32[N], in the order of
        emitters(): strictly increasing, the last one 2^24; entry j is picked with probability (T[j] - T[j - 1]) / 2^24. Above
        MAX_EMITTERS entries the library holds none: that raises."""
        n = self._L.vrt_emitter_cdf(self._h, None, 0)
        if n < 0:
            self._chk(n)
        if n > MAX_EMITTERS:
            raise VrtError(f"emitter_cdf: the tree has {n} emitters, more than MAX_EMITTERS")
        out = np.zeros(n, np.uint32)
        if n:
            got = self._L.vrt_emitter_cdf(self._h, out.ctypes.data, n)
            if got < 0:
                self._chk(got)
            assert got == n
        return out

    def accum_add(self, n_samples=1):
        """Enqueue n_samples more samples (vrt_accum_add) -> the samples now in the accumulation (n_samples after a restart)."""
        _check_int("n_samples", n_samples, "an integer in [1, 2^24]", 1, 1 << 24)
        total = C.c_uint32(0)
        self._chk(self._L.vrt_accum_add(self._h, int(n_samples), C.byref(total)))
        return int(total.value)

    def accum_resolve(self):
        """The resolved accumulation (vrt_accum_resolve) -> (rgba8[H,W,4], id_dist[H,W,2], shown rgba8[H,W,4])."""
        h, w = self._accum_hw("accum_resolve")
        rgba, shown = _zeros(h, w, "rgba8", "rgba8")
        idd = np.zeros((h, w, 2), np.int32)
        self._chk(self._L.vrt_accum_resolve(self._h, rgba.ctypes.data, idd.ctypes.data, shown.ctypes.data))
        return rgba, idd, shown

    def accum_resolve_device(self, d_rgba, d_id, d_shown, stream=None):
        """vrt_accum_resolve_device: DEVICE buffers (any may be None; d_shown needs d_rgba), enqueued on `stream`"""
        self._chk(self._L.vrt_accum_resolve_device(self._h, d_rgba, d_id, d_shown, stream))

    @staticmethod
    def _tonemap(tonemap, exposure):
        if tonemap not in TONEMAPS:
            raise ValueError(f"tonemap: expected 'clamp' or 'reinhard', got {tonemap!r}")
        return Tonemap(TONEMAPS[tonemap], _check_f32("exposure", exposure, _positive, "finite and > 0"))

    def _tonemap_ref(self, tonemap, exposure):
        """the tonemap / exposure arguments of the post chain -> a vrt_tonemap by reference; tonemap None: the NULL vrt_tonemap"""
        return None if tonemap is None else C.byref(self._tonemap(tonemap, exposure))

    def _accum_hw(self, who=None):
        """the current accumulation's (h, w). None begun: VrtError in `who`'s name, or without one (0, 0) and the library says so"""
        shape = getattr(self, "_accum_shape", None)
        if shape is None and who:
            raise VrtError(f"{who}: no accumulation (call accum_begin first)")
        return shape or (0, 0)

    @staticmethod
    def _hdr_samples(n_samples, n_prior):
        for name, v, lo in (("n_samples", n_samples, 1), ("n_prior", n_prior, 0)):
            _check_int(name, v, f"an integer in [{lo}, 2^24]", lo, 1 << 24)
        if int(n_prior) + int(n_samples) > 1 << 24:
            raise ValueError(f"n_prior + n_samples: at most 2^24 samples in all, got {int(n_prior) + int(n_samples)}")

    def shade_rays_hdr(self, origins, dirs, mode=MODE_FULL, width=None, first_sample=0, n_samples=1, tonemap="clamp",
                       exposure=1.0):
        """Context.shade_rays with the mean of the samples' unclamped colours (vrt_shade_rays_hdr) -> (rgb float32[n, 3];
        rgba8 uint8[n, 4]: its tone-mapped bytes, as accum_resolve_hdr maps them; id_dist int32[n, 2])."""
        tm = self._tonemap(tonemap, exposure)
        self._hdr_samples(n_samples, 0)
        o, stride, d = shade_ray_args(origins, dirs)
        n = d.shape[0]
        rgb = np.zeros((n, 3), np.float32)
        rgba = np.zeros((n, 4), np.uint8)
        idd = np.zeros((n, 2), np.int32)
        w = max(n, 1) if width is None else int(width)
        self._chk(self._L.vrt_shade_rays_hdr(self._h, n, o.ctypes.data if n else None, stride, d.ctypes.data if n else None, w,
                                             int(mode), int(first_sample) & 0xFFFFFFFF, int(n_samples), C.byref(tm),
                                             rgb.ctypes.data, rgba.ctypes.data, idd.ctypes.data))
        return rgb, rgba, idd

    def shade_rays_hdr_device(self, n, d_origins, origin_stride, d_dirs, d_rgb, d_rgba, d_id, d_sums=None, n_prior=0,
                              mode=MODE_FULL, width=None, first_sample=0, n_samples=1, tonemap="clamp", exposure=1.0, stream=None):
        """vrt_shade_rays_hdr_device: DEVICE buffers (d_rgb: n x 3 floats, d_rgba: n x 4 bytes, d_id: n x 2 int32, d_sums: n x 3
        float64 holding n_prior samples, read and written; any may be None, not all), enqueued on `stream`. Refining a batch:
        zero d_sums, then call with first_sample and n_prior advanced by the samples so far."""
        tm = self._tonemap(tonemap, exposure)
        self._hdr_samples(n_samples, n_prior)
        if n_prior != 0 and d_sums is None:
            raise ValueError("n_prior: needs d_sums")
        _check_int("n", n, "an integer in [0, 2^30]", 0, 2 ** 30)
        w = max(int(n), 1) if width is None else int(width)
        self._chk(self._L.vrt_shade_rays_hdr_device(self._h, int(n), d_origins, int(origin_stride), d_dirs, w, int(mode),
                                                    int(first_sample) & 0xFFFFFFFF, int(n_samples), int(n_prior), d_sums,
                                                    C.byref(tm), d_rgb, d_rgba, d_id, stream))

    def accum_resolve_hdr(self, tonemap="clamp", exposure=1.0):
        """An HDR accumulation's float resolve (vrt_accum_resolve_hdr) -> (rgb float32[H,W,3]: the mean of the samples' unclamped
        colours; rgba8[H,W,4]: its tone-mapped bytes, 'clamp' (exposure * x) or 'reinhard' (x' / (1 + x'), x' = exposure * x);
        shown rgba8[H,W,4]: the display pass on those bytes)."""
        tm = self._tonemap(tonemap, exposure)
        rgb, rgba, shown = _zeros(*self._accum_hw("accum_resolve_hdr"), "rgb", "rgba8", "rgba8")
        self._chk(self._L.vrt_accum_resolve_hdr(self._h, rgb.ctypes.data, C.byref(tm), rgba.ctypes.data, shown.ctypes.data))
        return rgb, rgba, shown

    def accum_resolve_hdr_device(self, d_rgb, d_rgba, d_shown, tonemap="clamp", exposure=1.0, stream=None):
        """vrt_accum_resolve_hdr_device: DEVICE buffers (any may be None; d_shown needs d_rgba), enqueued on `stream`"""
        tm = self._tonemap(tonemap, exposure)
        self._chk(self._L.vrt_accum_resolve_hdr_device(self._h, d_rgb, C.byref(tm), d_rgba, d_shown, stream))

    def accum_variance(self):
        """The variance of the mean's luminance of an accumulation begun with moments=True (vrt_accum_variance, M1-M3 of
        include/vrt.h) -> float32[H, W]; 65504^2 ("unknown") where a pixel holds fewer than two samples."""
        var, = _zeros(*self._accum_hw(), "plane")
        self._chk(self._L.vrt_accum_variance(self._h, var.ctypes.data))
        return var

    def accum_variance_device(self, ptr, stream=None):
        """vrt_accum_variance_device: a DEVICE buffer of H*W floats, enqueued on `stream`"""
        self._chk(self._L.vrt_accum_variance_device(self._h, ptr, stream))

    def accum_guides(self):
        """The accumulation's guide planes (vrt_accum_guides): first-hit features averaged over the samples in the sums ->
        {"normal": float32[H,W,3], "albedo": float32[H,W,4], "depth": float32[H,W], "coverage": float32[H,W]}."""
        h, w = self._accum_hw()
        out = {k: np.zeros((h, w) + c, np.float32) for k, c in _GUIDE_PLANES.items()}
        self._chk(self._L.vrt_accum_guides(self._h, *(p.ctypes.data for p in out.values())))
        return out

    def accum_guides_device(self, d_normal, d_albedo, d_depth, d_coverage, stream=None):
        """vrt_accum_guides_device: DEVICE buffers (H*W x 3, x 4, x 1, x 1 floats; any may be None), the resolve enqueued on `stream`"""
        self._chk(self._L.vrt_accum_guides_device(self._h, d_normal, d_albedo, d_depth, d_coverage, stream))

    def set_guide_glass(self, on):
        """Guides past glass (vrt_set_guide_glass, G0-G6 of include/vrt.h): 0 / False (default) or 1 / True. On, a guide sample
        follows the refracted ray through translucent surfaces to the first opaque one: its normal, RGB and the bent path's length,
        with the first surface's alpha. Read by the next accum_begin() (a change leaves an open accumulation's guides alone) and by
        guide_rays*() at the call. Any other value raises before the library is touched and the previous one holds."""
        _check_flag("guide glass", on, "0, 1 or a bool")
        self._chk(self._L.vrt_set_guide_glass(self._h, int(on)))
        self._guide_glass = bool(on)

    @property
    def guide_glass(self):
        """The value set_guide_glass() last set through this object (False until then). A copy kept in Python: the C-ABI has a
        setter only."""
        return getattr(self, "_guide_glass", False)

    def guide_rays(self, origins, dirs, width=None):
        """First-hit guides of the caller's own rays (vrt_guide_rays), one march each. origins, dirs as in shade_rays; width: the
        batch as an image of that width for the lane mapping (None: a list) -> {"normal": float32[n,3], "albedo": float32[n,4],
        "depth": float32[n], "hit": bool[n]}."""
        o, stride, d = shade_ray_args(origins, dirs)
        n = d.shape[0]
        normal = np.zeros((n, 3), np.float32)
        albedo = np.zeros((n, 4), np.float32)
        depth = np.zeros(n, np.float32)
        hit = np.zeros(n, np.uint8)
        w = max(n, 1) if width is None else int(width)
        self._chk(self._L.vrt_guide_rays(self._h, n, o.ctypes.data if n else None, stride, d.ctypes.data if n else None, w,
                                         normal.ctypes.data, albedo.ctypes.data, depth.ctypes.data, hit.ctypes.data))
        return {"normal": normal, "albedo": albedo, "depth": depth, "hit": hit != 0}

    def guide_rays_device(self, n, d_origins, origin_stride, d_dirs, d_normal, d_albedo, d_depth, d_hit, width=None, stream=None):
        """vrt_guide_rays_device: DEVICE buffers (n x 3, n x 4, n floats, n bytes; any may be None, not all), enqueued on `stream`"""
        _check_int("n", n, "an integer in [0, 2^30]", 0, 2 ** 30)
        w = max(int(n), 1) if width is None else int(width)
        self._chk(self._L.vrt_guide_rays_device(self._h, int(n), d_origins, int(origin_stride), d_dirs, w, d_normal, d_albedo,
                                                d_depth, d_hit, stream))

    def accum_resolve_hdr_shown(self, tonemap="clamp", exposure=1.0):
        """The HDR display pass on an HDR accumulation (vrt_accum_resolve_hdr_shown): the ID-aware blur on the float mean, then the
        tone map -> (shown_rgb float32[H,W,3]: the filtered mean; shown_rgba8[H,W,4]: its tone-mapped bytes)."""
        tm = self._tonemap_ref(tonemap, exposure)
        rgb, rgba = _zeros(*self._accum_hw("accum_resolve_hdr_shown"), "rgb", "rgba8")
        self._chk(self._L.vrt_accum_resolve_hdr_shown(self._h, tm, rgb.ctypes.data, rgba.ctypes.data))
        return rgb, rgba

    def accum_resolve_hdr_shown_device(self, d_shown_rgb, d_shown_rgba, tonemap="clamp", exposure=1.0, stream=None):
        """vrt_accum_resolve_hdr_shown_device: DEVICE buffers (either may be None, not both), enqueued on `stream`"""
        tm = self._tonemap_ref(tonemap, exposure)
        self._chk(self._L.vrt_accum_resolve_hdr_shown_device(self._h, tm, d_shown_rgb, d_shown_rgba, stream))

    def denoise_hdr(self, rgb, id_dist, tonemap="clamp", exposure=1.0):
        """The display pass in HDR through host arrays (vrt_denoise_hdr_host): quad.frag's ID-aware blur on a float image
        rgb[H,W,3], each float through h(c) = min(max(0, c), 65504), then the tone map of accum_resolve_hdr
        -> (rgb float32[H,W,3]: the filtered floats; rgba8 uint8[H,W,4]: their tone-mapped bytes)."""
        tm = self._tonemap_ref(tonemap, exposure)
        rgb = np.ascontiguousarray(rgb, np.float32)
        idd = np.ascontiguousarray(id_dist, np.int32)
        if rgb.ndim != 3 or rgb.shape[2] != 3 or idd.shape != rgb.shape[:2] + (2,):
            raise ValueError(f"expected rgb[H,W,3] and id_dist[H,W,2], got {rgb.shape} and {idd.shape}")
        h, w = rgb.shape[:2]
        out, out8 = _zeros(h, w, "rgb", "rgba8")
        self._chk(self._L.vrt_denoise_hdr_host(self._h, w, h, rgb.ctypes.data, idd.ctypes.data, tm, out.ctypes.data, out8.ctypes.data))
        return out, out8

    def denoise_hdr_device(self, width, height, d_rgb, d_id, d_out_rgb, d_out_rgba, tonemap="clamp", exposure=1.0, stream=None):
        """vrt_denoise_hdr: DEVICE buffers (d_rgb: W*H x 3 floats; d_out_rgb, d_out_rgba: either may be None, not both), enqueued
        on `stream`"""
        tm = self._tonemap_ref(tonemap, exposure)
        self._chk(self._L.vrt_denoise_hdr(self._h, width, height, d_rgb, d_id, tm, d_out_rgb, d_out_rgba, stream))

    @staticmethod
    def _filter_struct(filt, struct, defaults, sigmas):
        """None (the NULL filter: the library's default) or a dict with any of the keys of defaults() -> struct(levels, flags,
        *sigmas), every sigma named in `sigmas` a float32 value finite and > 0; ValueError otherwise"""
        if filt is None:
            return None
        d = defaults()
        unknown = set(filt) - set(d)
        if unknown:
            raise ValueError(f"filter: unknown keys {sorted(unknown)}")
        d.update(filt)
        lv = _check_int("levels", d["levels"], f"an integer in [0, {FILTER_MAX_LEVELS}]", 0, FILTER_MAX_LEVELS)
        sig = [_check_f32(name, d[name], _positive, "finite and > 0") for name in sigmas]
        return struct(lv, FILTER_DEMODULATE if d["demodulate"] else 0, *sig)

    @staticmethod
    def _filter(filt):
        """None (the NULL vrt_filter: vrt_filter_default) or a dict with any of default_filter()'s keys -> Filter or None"""
        return Context._filter_struct(filt, Filter, default_filter, ("sigma_normal", "sigma_albedo", "sigma_depth"))

    @staticmethod
    def _filter_var(filt):
        """None (the NULL vrt_filter_var: vrt_filter_var_default) or a dict with any of default_filter_var()'s keys -> FilterVar or
        None; the rules of _filter, for sigma_lum too"""
        return Context._filter_struct(filt, FilterVar, default_filter_var, ("sigma_normal", "sigma_albedo", "sigma_depth", "sigma_lum"))

    def filter_hdr(self, rgb, guides, filter=None, tonemap="clamp", exposure=1.0):
        """The guided filter through host arrays (vrt_filter_hdr_host): an edge-avoiding a-trous filter on a float image rgb[H,W,3]
        whose edge weights come from `guides` = {"normal": [H,W,3], "albedo": [H,W,4], "depth": [H,W], "coverage": [H,W]}, the
        planes accum_guides returns. filter: None (vrt_filter_default) or a dict with any of default_filter()'s keys
        -> (rgb float32[H,W,3]: the filtered floats; rgba8 uint8[H,W,4]: their tone-mapped bytes)."""
        tm = self._tonemap_ref(tonemap, exposure)
        f = _ref(self._filter(filter))
        rgb, planes, h, w = _planes(rgb, guides, tuple(_GUIDE_PLANES))
        out, out8 = _zeros(h, w, "rgb", "rgba8")
        self._chk(self._L.vrt_filter_hdr_host(self._h, w, h, rgb.ctypes.data, *(p.ctypes.data for p in planes), f, tm, out.ctypes.data,
                                              out8.ctypes.data))
        return out, out8

    def filter_hdr_device(self, width, height, d_rgb, d_normal, d_albedo, d_depth, d_coverage, d_out_rgb, d_out_rgba, filter=None,
                          tonemap="clamp", exposure=1.0, stream=None):
        """vrt_filter_hdr: DEVICE buffers (d_rgb: W*H x 3 floats; the planes as accum_guides_device writes them; d_out_rgb,
        d_out_rgba: either may be None, not both), enqueued on `stream`"""
        tm = self._tonemap_ref(tonemap, exposure)
        f = _ref(self._filter(filter))
        self._chk(self._L.vrt_filter_hdr(self._h, width, height, d_rgb, d_normal, d_albedo, d_depth, d_coverage, f, tm, d_out_rgb,
                                         d_out_rgba, stream))

    def accum_resolve_hdr_filtered(self, filter=None, tonemap="clamp", exposure=1.0):
        """The guided filter on an HDR accumulation (vrt_accum_resolve_hdr_filtered): its float mean filtered with its own guide
        planes -> (rgb float32[H,W,3]: the filtered mean; rgba8[H,W,4]: its tone-mapped bytes)."""
        tm = self._tonemap_ref(tonemap, exposure)
        f = _ref(self._filter(filter))
        rgb, rgba = _zeros(*self._accum_hw(), "rgb", "rgba8")
        self._chk(self._L.vrt_accum_resolve_hdr_filtered(self._h, f, tm, rgb.ctypes.data, rgba.ctypes.data))
        return rgb, rgba

    def accum_resolve_hdr_filtered_device(self, d_rgb, d_rgba, filter=None, tonemap="clamp", exposure=1.0, stream=None):
        """vrt_accum_resolve_hdr_filtered_device: DEVICE buffers (either may be None, not both), enqueued on `stream`"""
        tm = self._tonemap_ref(tonemap, exposure)
        f = _ref(self._filter(filter))
        self._chk(self._L.vrt_accum_resolve_hdr_filtered_device(self._h, f, tm, d_rgb, d_rgba, stream))

    def filter_hdr_var(self, rgb, guides, variance=None, filter=None, tonemap="clamp", exposure=1.0):
        """The variance-guided filter through host arrays (vrt_filter_hdr_var_host): filter_hdr with an edge-stopping luminance term
        whose width is each pixel's variance. variance: [H,W], the variance of the luminance of rgb at each pixel, or None: the
        filter estimates it spatially. filter: None (vrt_filter_var_default) or a dict with any of default_filter_var()'s keys
        -> (rgb float32[H,W,3], rgba8 uint8[H,W,4], variance float32[H,W]: the filtered image's)."""
        tm = self._tonemap_ref(tonemap, exposure)
        f = _ref(self._filter_var(filter))
        rgb, planes, h, w = _planes(rgb, guides, tuple(_GUIDE_PLANES))
        variance = _variance_plane(variance, h, w)
        out, out8, outv = _zeros(h, w, "rgb", "rgba8", "plane")
        self._chk(self._L.vrt_filter_hdr_var_host(self._h, w, h, rgb.ctypes.data, *(p.ctypes.data for p in planes), _addr(variance), f, tm,
                                                  out.ctypes.data, out8.ctypes.data, outv.ctypes.data))
        return out, out8, outv

    def filter_hdr_var_device(self, width, height, d_rgb, d_normal, d_albedo, d_depth, d_coverage, d_variance, d_out_rgb, d_out_rgba,
                              d_out_variance, filter=None, tonemap="clamp", exposure=1.0, stream=None):
        """vrt_filter_hdr_var: DEVICE buffers (filter_hdr_device's; d_variance: W*H floats or None; d_out_variance: W*H floats or
        None; d_out_rgb, d_out_rgba: either may be None, not both), enqueued on `stream`"""
        tm = self._tonemap_ref(tonemap, exposure)
        f = _ref(self._filter_var(filter))
        self._chk(self._L.vrt_filter_hdr_var(self._h, width, height, d_rgb, d_normal, d_albedo, d_depth, d_coverage, d_variance, f, tm,
                                             d_out_rgb, d_out_rgba, d_out_variance, stream))

    def accum_resolve_hdr_filtered_var(self, filter=None, tonemap="clamp", exposure=1.0):
        """The variance-guided filter on an HDR accumulation (vrt_accum_resolve_hdr_filtered_var): its float mean filtered with its
        own guide planes and its variance -> (rgb float32[H,W,3], rgba8[H,W,4], variance float32[H,W]). The variance is the
        measured one (accum_variance()'s plane) on an accumulation begun with moments=True that holds two samples or more, and a
        spatial estimate from the mean itself on every other."""
        tm = self._tonemap_ref(tonemap, exposure)
        f = _ref(self._filter_var(filter))
        rgb, rgba, var = _zeros(*self._accum_hw(), "rgb", "rgba8", "plane")
        self._chk(self._L.vrt_accum_resolve_hdr_filtered_var(self._h, f, tm, rgb.ctypes.data, rgba.ctypes.data, var.ctypes.data))
        return rgb, rgba, var

    def accum_resolve_hdr_filtered_var_device(self, d_rgb, d_rgba, d_variance, filter=None, tonemap="clamp", exposure=1.0, stream=None):
        """vrt_accum_resolve_hdr_filtered_var_device: DEVICE buffers (d_rgb, d_rgba: either may be None, not both; d_variance may be
        None), enqueued on `stream`"""
        tm = self._tonemap_ref(tonemap, exposure)
        f = _ref(self._filter_var(filter))
        self._chk(self._L.vrt_accum_resolve_hdr_filtered_var_device(self._h, f, tm, d_rgb, d_rgba, d_variance, stream))

    @staticmethod
    def _temporal(temporal, prev_camera):
        """a dict with any of default_temporal()'s keys (None: the defaults) and the previous frame's camera (prev_view_proj[16],
        prev_camera_pos[3 or 4]), or None where no history comes in -> Temporal; ValueError for an unknown key"""
        return _temporal_struct(_TEMPORAL, temporal, prev_camera)

    @staticmethod
    def _temporal_mom(temporal, prev_camera):
        """_temporal() for the calls that take a vrt_temporal_mom: a dict with any of default_temporal_mom()'s keys -> TemporalMom"""
        return _temporal_struct(_TEMPORAL_MOM, temporal, prev_camera)

    @staticmethod
    def _camera_block(camera):
        ip, iv, cp = (np.ascontiguousarray(v, np.float32).reshape(-1) for v in camera[:3])
        if ip.size != 16 or iv.size != 16 or cp.size != 4:
            raise ValueError("expected camera = (inv_projection[16], inv_view[16], camera_pos[4])")
        return ip, iv, cp

    # The four temporal entry points in their two flavours, as temporal_frame / temporal_accum of csrc/vrt_temporal.cpp: one body
    # each, told the C function by name (looked up when every argument has passed) and the builder of its struct; the _mom
    # flavour's one more plane comes as a tuple that the other flavour leaves empty.
    def _temporal_frame(self, fn, build, camera, rgb, guides, variance, history, prev_camera, temporal):
        ip, iv, cp = self._camera_block(camera)
        rgb, planes, h, w = _planes(rgb, guides, ("normal", "depth", "coverage"))
        planes += [_variance_plane(v, h, w) for v in variance]
        history = _history_planes(history, prev_camera, h, w)
        t = build(temporal, prev_camera if history is not None else None)
        outs = _zeros(h, w, "history", "rgb", "plane")
        self._chk(getattr(self._L, fn)(self._h, w, h, ip.ctypes.data, iv.ctypes.data, cp.ctypes.data, rgb.ctypes.data,
                                       *(_addr(p) for p in planes), _addr(history), C.byref(t), *(o.ctypes.data for o in outs)))
        return tuple(outs)

    def _temporal_frame_device(self, fn, build, width, height, camera, d_in, d_history_in, d_out, prev_camera, temporal, stream):
        ip, iv, cp = self._camera_block(camera)
        t = build(temporal, prev_camera if d_history_in is not None else None)
        self._chk(getattr(self._L, fn)(self._h, width, height, ip.ctypes.data, iv.ctypes.data, cp.ctypes.data, *d_in, d_history_in,
                                       C.byref(t), *d_out, stream))

    def _temporal_accum(self, fn, build, history, prev_camera, temporal, filter, tonemap, exposure):
        tm = self._tonemap_ref(tonemap, exposure)
        f = _ref(self._filter_var(filter))
        h, w = self._accum_hw()
        history = _history_planes(history, prev_camera, h, w)
        t = build(temporal, prev_camera if history is not None else None)
        outs = _zeros(h, w, "history", "rgb", "rgb", "rgba8", "plane")
        self._chk(getattr(self._L, fn)(self._h, C.byref(t), f, tm, _addr(history), *(o.ctypes.data for o in outs)))
        return tuple(outs)

    def _temporal_accum_device(self, fn, build, d_history_in, d_out, prev_camera, temporal, filter, tonemap, exposure, stream):
        tm = self._tonemap_ref(tonemap, exposure)
        f = _ref(self._filter_var(filter))
        t = build(temporal, prev_camera if d_history_in is not None else None)
        self._chk(getattr(self._L, fn)(self._h, C.byref(t), f, tm, d_history_in, *d_out, stream))

    def temporal_hdr(self, camera, rgb, guides, history=None, prev_camera=None, temporal=None):
        """The temporal pass through host arrays (vrt_temporal_hdr_host): last frame's `history` float32[3,H,W,4] (None: the first
        frame) reprojected into this frame -- rgb[H,W,3] with the "normal", "depth" and "coverage" planes of `guides` and the
        camera block they were made with, camera = (inv_projection, inv_view, camera_pos) as set_camera takes them -- tested
        against the planes and blended. prev_camera = (prev_view_proj[16], prev_camera_pos): the previous frame's forward
        projection * view and eye, needed with a history. temporal: None (vrt_temporal_default) or a dict with any of
        default_temporal()'s keys -> (history float32[3,H,W,4]: the next call's; rgb float32[H,W,3]: the integrated colour;
        variance float32[H,W]: of its luminance, the plane filter_hdr_var takes)."""
        return self._temporal_frame("vrt_temporal_hdr_host", self._temporal, camera, rgb, guides, (), history, prev_camera, temporal)

    def temporal_hdr_device(self, width, height, camera, d_rgb, d_normal, d_depth, d_coverage, d_history_in, d_history_out, d_out_rgb,
                            d_out_variance, prev_camera=None, temporal=None, stream=None):
        """vrt_temporal_hdr: DEVICE buffers (d_rgb: W*H x 3 floats; the planes as accum_guides_device writes them; the histories
        W*H x HISTORY_BYTES bytes each, d_history_in None on the first frame; d_out_rgb, d_out_variance: either may be None),
        enqueued on `stream`"""
        self._temporal_frame_device("vrt_temporal_hdr", self._temporal, width, height, camera, (d_rgb, d_normal, d_depth, d_coverage),
                                    d_history_in, (d_history_out, d_out_rgb, d_out_variance), prev_camera, temporal, stream)

    def accum_resolve_hdr_temporal(self, history=None, prev_camera=None, temporal=None, filter=None, tonemap="clamp", exposure=1.0):
        """The temporal pass and the variance-guided filter on an HDR accumulation (vrt_accum_resolve_hdr_temporal): its float mean
        with its own guide planes and the context's current camera, integrated with `history` (None: the first frame), then
        filtered with the temporal variance -> (history float32[3,H,W,4], integrated float32[H,W,3]: unfiltered, what the
        history holds; rgb float32[H,W,3], rgba8[H,W,4], variance float32[H,W]: the filter's)."""
        return self._temporal_accum("vrt_accum_resolve_hdr_temporal", self._temporal, history, prev_camera, temporal, filter, tonemap,
                                    exposure)

    def accum_resolve_hdr_temporal_device(self, d_history_in, d_history_out, d_integrated, d_rgb, d_rgba, d_variance, prev_camera=None,
                                          temporal=None, filter=None, tonemap="clamp", exposure=1.0, stream=None):
        """vrt_accum_resolve_hdr_temporal_device: DEVICE buffers (d_history_in None on the first frame; d_integrated and d_variance
        may be None; d_rgb, d_rgba: either may be None, not both), enqueued on `stream`"""
        self._temporal_accum_device("vrt_accum_resolve_hdr_temporal_device", self._temporal, d_history_in,
                                    (d_history_out, d_integrated, d_rgb, d_rgba, d_variance), prev_camera, temporal, filter, tonemap,
                                    exposure, stream)

    def temporal_hdr_mom(self, camera, rgb, guides, variance=None, history=None, prev_camera=None, temporal=None):
        """The temporal pass with measured variances and a 3 x 3 search through host arrays (vrt_temporal_hdr_mom_host):
        temporal_hdr's arguments, `variance` float32[H,W] -- this frame's measured variance of the mean, what accum_variance returns;
        None: unknown -- and temporal a dict with any of default_temporal_mom()'s keys -> (history float32[3,H,W,4], rgb
        float32[H,W,3], variance float32[H,W]): temporal_hdr's, the history with the integrated variance in plane 2's fourth float."""
        return self._temporal_frame("vrt_temporal_hdr_mom_host", self._temporal_mom, camera, rgb, guides, (variance,), history,
                                    prev_camera, temporal)

    def temporal_hdr_mom_device(self, width, height, camera, d_rgb, d_normal, d_depth, d_coverage, d_variance_in, d_history_in,
                                d_history_out, d_out_rgb, d_out_variance, prev_camera=None, temporal=None, stream=None):
        """vrt_temporal_hdr_mom: temporal_hdr_device's DEVICE buffers and d_variance_in (W*H floats, may be None), enqueued on
        `stream`"""
        self._temporal_frame_device("vrt_temporal_hdr_mom", self._temporal_mom, width, height, camera,
                                    (d_rgb, d_normal, d_depth, d_coverage, d_variance_in), d_history_in,
                                    (d_history_out, d_out_rgb, d_out_variance), prev_camera, temporal, stream)

    def accum_resolve_hdr_temporal_mom(self, history=None, prev_camera=None, temporal=None, filter=None, tonemap="clamp", exposure=1.0):
        """accum_resolve_hdr_temporal with the measured-variance pass (vrt_accum_resolve_hdr_temporal_mom): the variance input is the
        accumulation's own measured variance where it keeps moments (accum_keep_moments), unknown where it does not; temporal a dict
        with any of default_temporal_mom()'s keys -> the same five arrays."""
        return self._temporal_accum("vrt_accum_resolve_hdr_temporal_mom", self._temporal_mom, history, prev_camera, temporal, filter,
                                    tonemap, exposure)

    def accum_resolve_hdr_temporal_mom_device(self, d_history_in, d_history_out, d_integrated, d_rgb, d_rgba, d_variance, prev_camera=None,
                                              temporal=None, filter=None, tonemap="clamp", exposure=1.0, stream=None):
        """vrt_accum_resolve_hdr_temporal_mom_device: accum_resolve_hdr_temporal_device's DEVICE buffers, enqueued on `stream`"""
        self._temporal_accum_device("vrt_accum_resolve_hdr_temporal_mom_device", self._temporal_mom, d_history_in,
                                    (d_history_out, d_integrated, d_rgb, d_rgba, d_variance), prev_camera, temporal, filter, tonemap,
                                    exposure, stream)

    # Guided upsampling (include/vrt.h vrt_guide_frame, vrt_upsample_hdr, vrt_accum_resolve_hdr_upsampled), as upsample_frame /
    # upsample_host / upsample_accum of csrc/vrt_upsample.cpp: the struct from one builder, the planes through _planes
    @staticmethod
    def _frame_size(width, height):
        return (_check_int("width", width, "an integer >= 1", 1), _check_int("height", height, "an integer >= 1", 1))

    @staticmethod
    def _upsample(upsample):
        """None (the NULL vrt_upsample: vrt_upsample_default) or a dict with any of default_upsample()'s keys -> Upsample or None;
        ValueError for an unknown key, a factor outside 1..UPSAMPLE_MAX_FACTOR, a sigma that is not finite and > 0, a min_weight
        outside [0, 1) or an offset outside [0, 1]"""
        if upsample is None:
            return None
        d = default_upsample()
        unknown = set(upsample) - set(d)
        if unknown:
            raise ValueError(f"upsample: unknown keys {sorted(unknown)}")
        d.update(upsample)
        r = _check_int("factor", d["factor"], f"an integer in [1, {UPSAMPLE_MAX_FACTOR}]", 1, UPSAMPLE_MAX_FACTOR)
        sig = [_check_f32(k, d[k], _positive, "finite and > 0") for k in ("sigma_normal", "sigma_albedo", "sigma_depth")]
        mw = _check_f32("min_weight", d["min_weight"], lambda x: 0.0 <= x < 1.0, "in [0, 1)")
        off = [_check_f32(k, d[k], lambda x: 0.0 <= x <= 1.0, "in [0, 1]") for k in ("offset_lo_x", "offset_lo_y", "offset_hi_x", "offset_hi_y")]
        return Upsample(r, UPSAMPLE_DEMODULATE if d["demodulate"] else 0, *sig, mw, *off)

    def guide_frame(self, width, height):
        """The guide planes of a frame (vrt_guide_frame): one sample per pixel through the pixel's corner ray, from the context's
        current camera, uniforms and tree, with no accumulation involved -> accum_guides()'s dict at [height, width]."""
        w, h = self._frame_size(width, height)
        out = {k: np.zeros((h, w) + c, np.float32) for k, c in _GUIDE_PLANES.items()}
        self._chk(self._L.vrt_guide_frame(self._h, w, h, *(p.ctypes.data for p in out.values())))
        return out

    def guide_frame_device(self, width, height, d_normal, d_albedo, d_depth, d_coverage, stream=None):
        """vrt_guide_frame_device: DEVICE buffers (H*W x 3, x 4, x 1, x 1 floats; any may be None, not all), the resolve enqueued on
        `stream`"""
        w, h = self._frame_size(width, height)
        self._chk(self._L.vrt_guide_frame_device(self._h, w, h, d_normal, d_albedo, d_depth, d_coverage, stream))

    def upsample_hdr(self, rgb, guides, hi_guides, upsample=None, tonemap="clamp", exposure=1.0):
        """Guided upsampling through host arrays (vrt_upsample_hdr_host): the LOW image rgb[h,w,3] with its planes `guides` rebuilt
        at r times the size from the HIGH planes `hi_guides` ([r h, r w, ..]; both as accum_guides / guide_frame return them).
        upsample: None (vrt_upsample_default) or a dict with any of default_upsample()'s keys -> (rgb float32[H,W,3], rgba8
        uint8[H,W,4], unresolved uint8[H,W]: 1 where no tap counted and the nearest low pixel was taken)."""
        tm = self._tonemap_ref(tonemap, exposure)
        u = self._upsample(upsample)
        r = u.factor if u is not None else default_upsample()["factor"]
        rgb, planes, h, w = _planes(rgb, guides, tuple(_GUIDE_PLANES))
        hi = [np.ascontiguousarray(hi_guides[k], np.float32) for k in _GUIDE_PLANES]
        if any(p.shape != (r * h, r * w) + c for p, c in zip(hi, _GUIDE_PLANES.values())):
            raise ValueError(f"expected hi_guides at [{r * h}, {r * w}] for factor {r}; got {', '.join(str(p.shape) for p in hi)}")
        out, out8, mask = _zeros(r * h, r * w, "rgb", "rgba8", "mask")
        self._chk(self._L.vrt_upsample_hdr_host(self._h, w, h, rgb.ctypes.data, *(p.ctypes.data for p in planes), *(p.ctypes.data for p in hi),
                                                _ref(u), tm, out.ctypes.data, out8.ctypes.data, mask.ctypes.data))
        return out, out8, mask

    def upsample_hdr_device(self, width, height, d_rgb, d_normal, d_albedo, d_depth, d_coverage, d_hi_normal, d_hi_albedo, d_hi_depth,
                            d_hi_coverage, d_out_rgb, d_out_rgba, d_out_unresolved, upsample=None, tonemap="clamp", exposure=1.0,
                            stream=None):
        """vrt_upsample_hdr: DEVICE buffers (width, height: the LOW size; the high planes and the outputs at factor times it; d_out_rgb,
        d_out_rgba: either may be None, not both; d_out_unresolved may be None), enqueued on `stream`"""
        tm = self._tonemap_ref(tonemap, exposure)
        u = _ref(self._upsample(upsample))
        self._chk(self._L.vrt_upsample_hdr(self._h, width, height, d_rgb, d_normal, d_albedo, d_depth, d_coverage, d_hi_normal, d_hi_albedo,
                                           d_hi_depth, d_hi_coverage, u, tm, d_out_rgb, d_out_rgba, d_out_unresolved, stream))

    def accum_resolve_hdr_upsampled(self, upsample=None, tonemap="clamp", exposure=1.0):
        """Guided upsampling of an HDR accumulation (vrt_accum_resolve_hdr_upsampled): its float mean and its own planes are the LOW
        side, the guide planes of the frame `factor` times its size the HIGH side; the offsets are the accumulation's own -> (rgb
        float32[H,W,3], rgba8[H,W,4], unresolved uint8[H,W]) at the high size."""
        tm = self._tonemap_ref(tonemap, exposure)
        u = self._upsample(upsample)
        r = u.factor if u is not None else default_upsample()["factor"]
        h, w = self._accum_hw()
        rgb, rgba, mask = _zeros(r * h, r * w, "rgb", "rgba8", "mask")
        self._chk(self._L.vrt_accum_resolve_hdr_upsampled(self._h, _ref(u), tm, rgb.ctypes.data, rgba.ctypes.data, mask.ctypes.data))
        return rgb, rgba, mask

    def accum_resolve_hdr_upsampled_device(self, d_rgb, d_rgba, d_unresolved, upsample=None, tonemap="clamp", exposure=1.0, stream=None):
        """vrt_accum_resolve_hdr_upsampled_device: DEVICE buffers of the HIGH size (d_rgb, d_rgba: either may be None, not both;
        d_unresolved may be None), enqueued on `stream`"""
        tm = self._tonemap_ref(tonemap, exposure)
        u = _ref(self._upsample(upsample))
        self._chk(self._L.vrt_accum_resolve_hdr_upsampled_device(self._h, u, tm, d_rgb, d_rgba, d_unresolved, stream))

    # Auto-exposure (include/vrt.h vrt_meter_hdr, vrt_tonemap_hdr, vrt_accum_resolve_hdr_metered), as the entry points of
    # csrc/vrt_meter.cpp: the struct from one builder (_meter), the record as the dict meter_resolve returns
    def meter_hdr(self, rgb, meter=None, state=None):
        """Light metering through host arrays (vrt_meter_hdr_host): rgb[H,W,3]; meter: None (vrt_meter_default) or a dict with any of
        default_meter()'s keys; state: None (the first frame) or the record an earlier call returned -> (the new record as a dict,
        the histogram uint32[METER_BINS] of the metered rectangle)."""
        m = _meter(meter)
        e = _exposure(state)
        rgb = np.ascontiguousarray(rgb, np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"expected rgb[H,W,3], got {rgb.shape}")
        hist = np.zeros(METER_BINS, np.uint32)
        self._chk(self._L.vrt_meter_hdr_host(self._h, rgb.shape[1], rgb.shape[0], rgb.ctypes.data, _ref(m), hist.ctypes.data, C.byref(e)))
        return _exposure_dict(e), hist

    def meter_hdr_device(self, width, height, d_rgb, d_histogram, d_exposure, meter=None, stream=None):
        """vrt_meter_hdr: DEVICE buffers (d_rgb H*W x 3 floats; d_histogram METER_BINS uint32, zeroed by the call; d_exposure one
        vrt_exposure of 16 bytes, read and written), enqueued on `stream`"""
        w, h = self._frame_size(width, height)
        self._chk(self._L.vrt_meter_hdr(self._h, w, h, d_rgb, _ref(_meter(meter)), d_histogram, d_exposure, stream))

    def tonemap_hdr(self, rgb, tonemap="clamp", exposure=1.0, state=None):
        """The tone map by a record through host arrays (vrt_tonemap_hdr_host, E9): rgb[..., 3] float32; state: None (no record: the
        bytes of accum_resolve_hdr's tone map) or a record as meter_hdr returns it -> rgba8 uint8[..., 4]."""
        tm = self._tonemap_ref(tonemap, exposure)
        rgb = np.ascontiguousarray(rgb, np.float32)
        if rgb.ndim < 1 or rgb.shape[-1] != 3 or rgb.size == 0:
            raise ValueError(f"expected rgb[..., 3] with at least one pixel, got {rgb.shape}")
        out = np.zeros(rgb.shape[:-1] + (4,), np.uint8)
        e = None if state is None else _exposure(state)
        self._chk(self._L.vrt_tonemap_hdr_host(self._h, rgb.size // 3, rgb.ctypes.data, tm, _ref(e), out.ctypes.data))
        return out

    def tonemap_hdr_device(self, n, d_rgb, d_out_rgba, d_exposure=None, tonemap="clamp", exposure=1.0, stream=None):
        """vrt_tonemap_hdr: DEVICE buffers (d_rgb n x 3 floats, d_out_rgba n x 4 bytes; d_exposure: the record, or None), enqueued on
        `stream`"""
        tm = self._tonemap_ref(tonemap, exposure)
        n = _check_int("n", n, "an integer in [1, 2^30]", 1, 1 << 30)
        self._chk(self._L.vrt_tonemap_hdr(self._h, n, d_rgb, tm, d_exposure, d_out_rgba, stream))

    def accum_resolve_hdr_metered(self, meter=None, tonemap="clamp", exposure=1.0, state=None):
        """An HDR accumulation resolved, metered and tone mapped by the fresh record (vrt_accum_resolve_hdr_metered) -> (the new
        record as a dict, rgb float32[H,W,3], rgba8[H,W,4], the histogram uint32[METER_BINS])."""
        tm = self._tonemap_ref(tonemap, exposure)
        m = _meter(meter)
        e = _exposure(state)
        h, w = self._accum_hw()
        rgb, rgba = _zeros(h, w, "rgb", "rgba8")
        hist = np.zeros(METER_BINS, np.uint32)
        self._chk(self._L.vrt_accum_resolve_hdr_metered(self._h, _ref(m), tm, C.byref(e), rgb.ctypes.data, rgba.ctypes.data, hist.ctypes.data))
        return _exposure_dict(e), rgb, rgba, hist

    def accum_resolve_hdr_metered_device(self, d_exposure, d_histogram, d_rgb, d_rgba, meter=None, tonemap="clamp", exposure=1.0, stream=None):
        """vrt_accum_resolve_hdr_metered_device: DEVICE buffers (d_exposure: the record, required; d_histogram, d_rgb, d_rgba: each
        may be None), enqueued on `stream`"""
        tm = self._tonemap_ref(tonemap, exposure)
        self._chk(self._L.vrt_accum_resolve_hdr_metered_device(self._h, _ref(_meter(meter)), tm, d_exposure, d_histogram, d_rgb, d_rgba, stream))

    # Bloom (include/vrt.h vrt_bloom_hdr, vrt_accum_resolve_hdr_bloomed), as the entry points of csrc/vrt_bloom.cpp: the struct from
    # one builder (_bloom), the record as the dict meter_resolve returns
    def bloom_hdr(self, rgb, bloom=None, tonemap="clamp", exposure=1.0, state=None):
        """Bloom through host arrays (vrt_bloom_hdr_host): rgb[H,W,3]; bloom: None (vrt_bloom_default) or a dict with any of
        default_bloom()'s keys; state: None (no record) or a record as meter_hdr returns it -> (f float32[H,W,3], rgba8[H,W,4])."""
        b = _bloom(bloom)
        tm = self._tonemap_ref(tonemap, exposure)
        rgb = np.ascontiguousarray(rgb, np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"expected rgb[H,W,3], got {rgb.shape}")
        e = None if state is None else _exposure(state)
        out, rgba = _zeros(rgb.shape[0], rgb.shape[1], "rgb", "rgba8")
        self._chk(self._L.vrt_bloom_hdr_host(self._h, rgb.shape[1], rgb.shape[0], rgb.ctypes.data, _ref(b), tm, _ref(e), out.ctypes.data,
                                             rgba.ctypes.data))
        return out, rgba

    def bloom_hdr_device(self, width, height, d_rgb, d_workspace, d_out_rgb, d_out_rgba, d_exposure=None, bloom=None, tonemap="clamp",
                         exposure=1.0, stream=None):
        """vrt_bloom_hdr: DEVICE buffers (d_rgb H*W x 3 floats; d_workspace bloom_workspace_bytes() bytes, a multiple of 16, not
        initialised; d_out_rgb H*W x 3 floats and d_out_rgba H*W x 4 bytes: either may be None, not both; d_exposure: the record,
        or None), enqueued on `stream`"""
        w, h = self._frame_size(width, height)
        tm = self._tonemap_ref(tonemap, exposure)
        self._chk(self._L.vrt_bloom_hdr(self._h, w, h, d_rgb, _ref(_bloom(bloom)), tm, d_exposure, d_workspace, d_out_rgb, d_out_rgba, stream))

    def accum_resolve_hdr_bloomed(self, meter=None, bloom=None, tonemap="clamp", exposure=1.0, state=None, metering=True):
        """An HDR accumulation resolved, metered, bloomed and tone mapped by the fresh record (vrt_accum_resolve_hdr_bloomed) -> (the
        new record as a dict, f float32[H,W,3], rgba8[H,W,4]). metering False: no metering and no record (io == NULL); the record
        returned is None."""
        tm = self._tonemap_ref(tonemap, exposure)
        m, b = _meter(meter), _bloom(bloom)
        e = _exposure(state) if metering else None
        h, w = self._accum_hw()
        rgb, rgba = _zeros(h, w, "rgb", "rgba8")
        self._chk(self._L.vrt_accum_resolve_hdr_bloomed(self._h, _ref(m), _ref(b), tm, _ref(e), rgb.ctypes.data, rgba.ctypes.data))
        return (None if e is None else _exposure_dict(e)), rgb, rgba

    def accum_resolve_hdr_bloomed_device(self, d_exposure, d_rgb, d_rgba, meter=None, bloom=None, tonemap="clamp", exposure=1.0, stream=None):
        """vrt_accum_resolve_hdr_bloomed_device: DEVICE buffers (d_exposure: the record, None: no metering; d_rgb, d_rgba: either may
        be None, not both), enqueued on `stream`"""
        tm = self._tonemap_ref(tonemap, exposure)
        self._chk(self._L.vrt_accum_resolve_hdr_bloomed_device(self._h, _ref(_meter(meter)), _ref(_bloom(bloom)), tm, d_exposure, d_rgb, d_rgba,
                                                               stream))

    def denoise(self, rgba, id_dist):
        """quad.frag's ID-aware blur through host arrays -> rgba8[H,W,4]."""
        rgba = np.ascontiguousarray(rgba, np.uint8)
        idd = np.ascontiguousarray(id_dist, np.int32)
        h, w = rgba.shape[:2]
        out = np.zeros_like(rgba)
        self._chk(self._L.vrt_denoise_host(self._h, w, h, rgba.ctypes.data, idd.ctypes.data, out.ctypes.data))
        return out

    def patch_voxel(self, world, x, y, z, max_depth=15):
        """After `world` has been edited at voxel (x, y, z): replaces the smallest enclosing sub-tree on the device
        (vrt_patch_plan / vrth_world_path_records / vrt_patch_apply). Returns the depth of the node replaced, or None
        when the edit needs a full upload (nothing was changed on the device then)."""
        H = host_lib()
        plan = Patch()
        while max_depth >= 1:
            if self._L.vrt_patch_plan(self._h, x, y, z, max_depth, C.byref(plan)) != 0:
                return None
            if H.vrth_world_node_state(world._h, plan.path, plan.depth) == 2:
                p, n = C.c_void_p(), C.c_size_t(0)
                if H.vrth_world_path_records(world._h, plan.path, plan.depth, x, y, z, C.byref(p), C.byref(n)) != 0:
                    return None
                try:
                    self._chk(self._L.vrt_patch_apply(self._h, C.byref(plan), p, n.value))
                finally:
                    H.vrth_free(p)
                return plan.depth
            max_depth = plan.depth - 1
        return None

    def patch_box(self, world, lo, hi, max_depth=15):
        """After `world` has been edited anywhere inside the box of voxels [lo, hi] (inclusive): ONE patch for the whole box
        (vrt_patch_plan_box / vrth_world_box_records / vrt_patch_apply). Returns the depth of the node replaced, or None when the
        edit needs a full upload."""
        H = host_lib()
        lo3, hi3 = (C.c_int32 * 3)(*[int(v) for v in lo]), (C.c_int32 * 3)(*[int(v) for v in hi])
        plan = Patch()
        while max_depth >= 1:
            if self._L.vrt_patch_plan_box(self._h, lo3, hi3, max_depth, C.byref(plan)) != 0:
                return None
            if H.vrth_world_node_state(world._h, plan.path, plan.depth) == 2:
                p, n = C.c_void_p(), C.c_size_t(0)
                if H.vrth_world_box_records(world._h, plan.path, plan.depth, lo3, hi3, C.byref(p), C.byref(n)) != 0:
                    return None
                try:
                    self._chk(self._L.vrt_patch_apply(self._h, C.byref(plan), p, n.value))
                finally:
                    H.vrth_free(p)
                return plan.depth
            max_depth = plan.depth - 1
        return None

    def patch_begin(self):
        self._chk(self._L.vrt_patch_begin(self._h))

    def patch_end(self):
        self._chk(self._L.vrt_patch_end(self._h))

    def compact(self):
        self._chk(self._L.vrt_compact(self._h))

    def dispatch_views(self, width, height, tile_rows, shard, n_shards, mode, views, stream=None):
        """views: sequence of (inv_proj, inv_view, cam_pos, d_rgba8, d_id_dist) or a prepared (View * n) array;
        one launch renders them all (vrt_dispatch_views)."""
        if not isinstance(views, C.Array):
            views = make_views(views)
        self._chk(self._L.vrt_dispatch_views(self._h, width, height, tile_rows, shard, n_shards, mode, views, len(views),
                                             stream))

    def dispatch_frame(self, width, height, mode=MODE_FULL):
        """Dispatch + display pass with the intermediates kept on the device -> (shown, rgba8, id_dist) host arrays."""
        shown = np.zeros((height, width, 4), np.uint8)
        rgba = np.zeros((height, width, 4), np.uint8)
        idd = np.zeros((height, width, 2), np.int32)
        self._chk(self._L.vrt_dispatch_frame(self._h, width, height, mode, shown.ctypes.data, rgba.ctypes.data,
                                             idd.ctypes.data))
        return shown, rgba, idd

    def denoise_device(self, width, height, d_rgba, d_id, d_out, stream=None):
        self._chk(self._L.vrt_denoise(self._h, width, height, d_rgba, d_id, d_out, stream))

    def set_tile_scheduling(self, period):
        """Feedback scheduling of the tracing kernel's tiles (vrt_set_tile_scheduling): 0 = off, default 16."""
        self._chk(self._L.vrt_set_tile_scheduling(self._h, period))

    def sched_order(self, stream=None, cap=1 << 20):
        """The scheduler's current workgroup order for the shape last launched on `stream` (vrt_get_tile_order);
        empty until an order has been derived."""
        buf = np.zeros(cap, np.uint32)
        n = self._L.vrt_get_tile_order(self._h, stream, buf.ctypes.data, cap)
        if n < 0:
            self._chk(n)
        return buf[:min(n, cap)].copy()

    def sched_split_count(self, stream=None, cap=1 << 20):
        """How many groups at the head of the current order a VRT_MODE_FULL launch traces as part-tile waves (OPT_HEAVY_TILES)."""
        buf = np.zeros(cap, np.uint32)
        n = self._L.vrt_get_tile_order(self._h, stream, buf.ctypes.data, cap)
        if n < 0:
            self._chk(n)
        return int(buf[n]) if 0 < n < cap else 0

    def set_option(self, option, value):
        self._chk(self._L.vrt_set_option(self._h, option, value))

    def set_tile_order(self, enable, d_group_order=None, d_tile_cost=None):
        """caller-owned device buffers for the default kernel's group order / per-tile ticks (vrt_set_tile_order)"""
        self._chk(self._L.vrt_set_tile_order(self._h, 1 if enable else 0, d_group_order, d_tile_cost))

    def set_denoise_variant(self, v):
        """VRT_OPT_DISPLAY_KERNEL: 0 = each wave the cheaper of its two walks (default); 2 / 3 = one walk forced."""
        self.set_option(OPT_DISPLAY_KERNEL, v)

    def synchronize(self):
        self._chk(self._L.vrt_synchronize(self._h))

    @property
    def stream(self):
        return self._L.vrt_stream(self._h)

    def set_root0_only(self, on):
        """A/B: False = rays that leave wide root 0 always walk the records of the octants around it"""
        self.set_option(OPT_EMPTY_OCTANTS, int(on))   # True/1: on, 2: on without the tighter root, False/0: off

    def set_ray_tables(self, on):
        """A/B: False = every launch runs the shader's own ray-generation prologue (no per-projection tables)"""
        self.set_option(OPT_RAY_TABLES, 1 if on else 0)

    def debug_math(self, op, x, y):
        """device probe of the kernels' arithmetic (test support library, vrt_test_math) on this context's device"""
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y, np.float32)
        out = np.zeros_like(x)
        r = test_lib().vrt_test_math(self._L.vrt_device(self._h), op, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size)
        if r != 0:
            raise VrtError(f"vrt_test_math failed ({r})")
        return out


DELIVER_PEER_STORE, DELIVER_GATHER = 0, 1


class Multi:
    """vrt_multi: one context per device in this process, frames assembled on the first device (include/vrt.h)."""

    def __init__(self, devices):
        L = hip_lib()
        self._L = L
        ids = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        r = L.vrt_create_multi(len(devices), ids, C.byref(h))
        if r != 0:
            raise VrtError(f"vrt_create_multi failed ({r}): {L.vrt_multi_last_error(None).decode()}")
        self._h = h
        self.n = len(devices)

    def close(self):
        if self._h:
            self._L.vrt_destroy_multi(self._h)
            self._h = None

    def _chk(self, r):
        if r != 0:
            raise VrtError(f"vrt_multi error {r}: {self._L.vrt_multi_last_error(self._h).decode()}")

    def upload_octree(self, texels, tex_dim):
        t = np.ascontiguousarray(texels, dtype=np.uint8)
        self._chk(self._L.vrt_multi_upload_octree(self._h, t.ctypes.data if t.size else None, t.size, tex_dim))

    def set_camera(self, inv_proj, inv_view, cam_pos):
        ip, iv, cp = (np.ascontiguousarray(x, dtype=np.float32) for x in (inv_proj, inv_view, cam_pos))
        self._chk(self._L.vrt_multi_set_camera(self._h, _fptr(ip), _fptr(iv), _fptr(cp)))

    def frame_alloc(self, width, height):
        a, b = C.c_void_p(), C.c_void_p()
        self._chk(self._L.vrt_multi_frame_alloc(self._h, width, height, C.byref(a), C.byref(b)))
        return a.value, b.value

    def frame_free(self, d_rgba, d_id):
        self._chk(self._L.vrt_multi_frame_free(self._h, d_rgba, d_id))

    def dispatch(self, width, height, tile_rows, mode, delivery, d_rgba, d_id):
        self._chk(self._L.vrt_multi_dispatch(self._h, width, height, tile_rows, mode, delivery, d_rgba, d_id))

    def dispatch_frame(self, width, height, mode, d_shown):
        """vrt_multi_dispatch_frame: the displayed frame (trace + display pass in row bands with a halo) into d_shown on device 0"""
        r = self._L.vrt_multi_dispatch_frame(self._h, width, height, mode, C.c_void_p(d_shown))
        if r != 0:
            raise VrtError(f"vrt_multi_dispatch_frame failed ({r}): {self._L.vrt_multi_last_error(self._h).decode()}")

    def synchronize(self):
        self._chk(self._L.vrt_multi_synchronize(self._h))

    def stream(self):
        return self._L.vrt_multi_stream(self._h)

    def context(self, i):
        """the i-th device's context as a (borrowed) Context: do not close() it"""
        c = Context.__new__(Context)
        c._L = self._L
        c._h = C.c_void_p(self._L.vrt_multi_context(self._h, i))
        c.borrowed = True
        return c


def make_views(views):
    """(inv_proj, inv_view, cam_pos, d_rgba8, d_id_dist) tuples -> ctypes array of vrt_view"""
    arr = (View * len(views))()
    for v, (ip, iv, cp, p_rgba, p_id) in zip(arr, views):
        v.inv_projection[:] = [float(x) for x in ip]
        v.inv_view[:] = [float(x) for x in iv]
        v.camera_pos[:] = [float(x) for x in cp]
        v.d_rgba8, v.d_id_dist = p_rgba, p_id
    return arr


def shard_rows(height, tile_rows, shard, n_shards):
    return hip_lib().vrt_shard_rows(height, tile_rows, shard, n_shards)


def shard_row_indices(height, tile_rows, shard, n_shards):
    """Frame rows owned by a shard under the interleaved row-tile scheme, in compact order."""
    rows = []
    tiles = (height + tile_rows - 1) // tile_rows
    for t in range(shard, tiles, n_shards):
        rows.extend(range(t * tile_rows, min(height, (t + 1) * tile_rows)))
    return rows
