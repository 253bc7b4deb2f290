"""The HDR display pass restated in scalar C (tests/oracle_denoise_hdr.c) -- TEST INFRASTRUCTURE ONLY.

build(tmp_dir) compiles oracle_denoise_hdr.c as tests/oracle_hdr.py compiles its library: the same flags (no contraction), the same
three other oracle sources. The library holds everything oracle_hdr's holds (oracle_denoise_hdr.c includes oracle_hdr.c), so
oracle_hdr.render / Accum / tonemap take it too. denoise() is include/vrt.h vrt_denoise_hdr points 1-3; denoise64() the same sums
in float64 numpy, for the error bound; the two misreadings are planted mistakes the comparisons must catch."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_hdr

OPS = oracle_hdr.OPS


def build(tmp_dir):
    out = os.path.join(str(tmp_dir), "liboracle_denoise_hdr.so")
    srcs = [os.path.join(oracle_hdr.ROOT, "tests", "oracle_denoise_hdr.c")] + [os.path.join(oracle_hdr.ORACLE, f) for f in
                                                                              ("octree_oracle.c", "vox_oracle.c", "camera_oracle.c")]
    subprocess.run(["gcc", *oracle_hdr.CFLAGS, "-shared", "-o", out, *srcs, "-lm"], check=True)
    L = C.CDLL(out)
    L.o_denoise_hdr.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    L.o_denoise_hdr.restype = None
    # oracle_hdr.c's own, declared as oracle_hdr.build() declares them
    L.o_render_hdr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_float, C.c_float,
                               C.c_void_p]
    L.o_render_hdr.restype = None
    L.o_render_lens.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_float,
                                C.c_float, C.c_void_p, C.c_void_p]
    L.o_render_lens.restype = None
    L.o_hdr_unorm8.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.o_hdr_unorm8.restype = None
    L.o_hdr_value.argtypes = [C.c_float]
    L.o_hdr_value.restype = C.c_float
    L.o_hdr_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.o_hdr_add.restype = None
    L.o_hdr_mean.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.o_hdr_mean.restype = None
    L.o_hdr_tonemap.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_void_p]
    L.o_hdr_tonemap.restype = None
    return L


def denoise(L, rgb, id_dist, op="clamp", exposure=1.0):
    """rgb float32[H,W,3], id_dist int32[H,W,2] -> (filtered float32[H,W,3], tone-mapped rgba8[H,W,4]); op None: the NULL
    vrt_tonemap (clamp, exposure 1)"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    idd = np.ascontiguousarray(id_dist, np.int32)
    h, w = rgb.shape[:2]
    assert rgb.shape == (h, w, 3) and idd.shape == (h, w, 2)
    out = np.zeros_like(rgb)
    out8 = np.zeros((h, w, 4), np.uint8)
    if op is None:
        op, exposure = "clamp", 1.0
    L.o_denoise_hdr(rgb.ctypes.data, idd.ctypes.data, w, h, OPS[op], float(np.float32(exposure)), out.ctypes.data, out8.ctypes.data)
    return out, out8


def h_of(L, rgb):
    """h(c) of every float, through the checker's own function"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    return np.array([L.o_hdr_value(C.c_float(v.item())) for v in rgb.ravel()], np.float32).reshape(rgb.shape)


def radius(dist):
    """R = clamp(int(200.0f / sqrtf((float)max(1, dist))), 1, 20), in float32 as the contract states it"""
    d = np.maximum(np.asarray(dist, np.int64), 1).astype(np.float32)
    r = (np.float32(200.0) / np.sqrt(d, dtype=np.float32)).astype(np.int64)
    return np.clip(r, 1, 20)


def _windows(hc, id_dist, same_id=True):
    """for every pixel with a non-zero id: (y, x, the h(c) of its window's taps that count [n, 3] in y-outer, x-inner order)"""
    H, W = id_dist.shape[:2]
    ids, R = id_dist[..., 0], radius(id_dist[..., 1])
    for y in range(H):
        for x in range(W):
            if ids[y, x] == 0:
                continue
            r = int(R[y, x])
            y0, y1, x0, x1 = max(0, y - r), min(H, y + r + 1), max(0, x - r), min(W, x + r + 1)
            win = hc[y0:y1, x0:x1].reshape(-1, 3)
            if same_id:
                win = win[(ids[y0:y1, x0:x1] == ids[y, x]).ravel()]
            yield y, x, win


def denoise64(L, rgb, id_dist):
    """-> (float64[H,W,3]: the same sums and the division evaluated in float64; count int[H,W], 0 where the pixel passes through)"""
    hc = h_of(L, rgb).astype(np.float64)
    out = hc.copy()
    count = np.zeros(id_dist.shape[:2], np.int64)
    for y, x, win in _windows(hc, np.asarray(id_dist)):
        count[y, x] = len(win)
        out[y, x] = win.sum(axis=0) / max(len(win), 1)
    return out, count


def misread_across_ids(L, rgb, id_dist):
    """PLANTED MISTAKE: every in-image tap of the window counts, whatever its id -> float32[H,W,3] (sequential float32 sums)"""
    hc = h_of(L, rgb)
    out = hc.copy()
    for y, x, win in _windows(hc, np.asarray(id_dist), same_id=False):
        s = np.zeros(3, np.float32)
        for t in win:
            s = s + t
        out[y, x] = s / np.float32(len(win))
    return out


def misread_tonemap_first(L, O, rgb, id_dist, op, exposure):
    """PLANTED MISTAKE: tone map and quantise, then the byte pass (what vrt_accum_resolve_hdr's shown image is) -> rgba8[H,W,4]"""
    return O.denoise(oracle_hdr.tonemap(L, h_of(L, rgb), op, exposure), id_dist)
