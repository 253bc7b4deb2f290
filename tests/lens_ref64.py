"""The rays of a jittered or thin-lens sample of the progressive accumulation in float64, with bounds on how far their
float32 counterparts may lie from them (test helper, not a test).

Written from include/vrt.h ("VRT_ACCUM_JITTER" and "vrt_set_lens", points 1-6) and from the geometry; numpy and
shader_ref64 only, nothing under oracle/, none of the checkers and nothing of the product
(tests/test_shader_reference64.py enforces that). lens_rays() returns what shader_ref64.Trace.lens (modes 0 and 1) and
path_ref64.PathTrace.lens (mode 2) hand to the entries they share with the frame and ray-batch constructors.

Jitter. jx(k) = (bitreverse32(k) >> 8) * 2^-24 and jy(k) = (sobol2(k) >> 8) * 2^-24 in exact integer arithmetic. The
jittered position is DEFINED as one float32 addition rounded to nearest, float32(px) + float32(jx): it is done in
np.float32 (like rand()'s float conversion in path_ref64) and everything after it is shader_ref64.ray_dirs' float64
arithmetic. The frame's existing ~6u direction error (FRAME_DIR_ERR, which shader_ref64's step error already carries) then
applies unchanged; no term is added for jitter. At k = 2^32 - 1, jx = 1 - 2^-24: px + jx is px + 1 for px >= 2, a float32
tie that goes to the even 2 at px = 1, and exact at px = 0.

Lens sequence. Direction numbers v[i] = m[i] << (31 - i) for i < 3, then v[i] = v[i-3] ^ (v[i-3] >> 3) ^ v[i-1] (x^2 term)
^ v[i-2] (x term), over x^3+x+1 with m = 1,1,5 (lu) and x^3+x^2+1 with m = 1,3,1 (lv); the XOR over the set bits of k,
>> 8, the top bit flipped. Integers, exact.

Concentric map. a = 2 lu - 1 = (n_u - 2^23) * 2^-23 and b likewise are exact in float32, so a == b == 0 and |a| > |b| are
taken on the integers. (lx, ly) = (0, 0) only at a == b == 0: elsewhere r != 0 and cos, sin do not vanish together.
phi is computed from the float32 constants (they are part of the definition). Its float32 value is off by at most
4u: the quotient and the product round once each (<= 2u * pi/4) and, in the second branch, the difference once more
(<= u * 3pi/4). det_sincos adds E_SINCOS (its measured bound on [0, 2 pi); phi lies in [-pi/4, 3pi/4] and the routine
folds the sign first), and the product r * cos rounds once: |lx32 - lx| <= |r| (E_SINCOS + 4u) + u |lx|, the same for ly.

The ray (point 5), e = camera_pos.xyz, R, U, Z from the float32 inv_view, d the (jittered) pinhole direction:
  cosd = -((d.x Z.x + d.y Z.y) + d.z Z.z): e_cos = FRAME_DIR_ERR (|Z.x| + |Z.y| + |Z.z|) + 4u sum |d_i Z_i|.
  Pinhole cases: aperture == 0, the lens centre, !(cosd > 0): the pinhole ray (e, d) with the frame's bounds (origin
  exact, no extra direction term). A cosd within e_cos of 0 is undecided.
  1. Origin, per axis i: o_i = (e_i + sx R_i) + sy U_i with sx = aperture lx, sy = aperture ly.
     err_o_i = aperture (e_lx |R_i| + e_ly |U_i|)                  the lens point's error
             + u (|sx| |R_i| + |sy| |U_i|)                          sx and sy round
             + u (|sx R_i| + |sy U_i| + |e_i + sx R_i| + |o_i|)     the two multiply-adds, relative to ~|e_i|
     It enters as err3 / lo3 (times voxelScale, plus u |gro| for the float32 product o * voxelScale) on top of
     ray_start's rounding of this module's float64 o.
  2. Direction, absolute per component (one number per ray, the largest): t = focus / cosd has
     e_t = t (e_cos / (cosd - e_cos) + u); p_i = e_i + t d_i has err_p_i = |d_i| e_t + t FRAME_DIR_ERR + u |t d_i| + u |p_i|;
     v = p - o has err_v_i = err_p_i + err_o_i + u |v_i|; n = v / |v| moves by (I - n n^T) dv / |v|:
     dir_err = max_i min(err_v_i + |n_i| sum_j |n_j| err_v_j, |err_v|_2) / |v| (the projection does not lengthen a
     vector) + 2 * 4.5u for the normalize of point 5 and pathTrace's own (shader_ref64.GIVEN_DIR_ERR each). err_p grows like |e| / focus relative to |v|, so the bound is per ray.
  The start medium, distanceInMedium, dist and every other use of the origin come from o; the RNG is initRNG(pixel, k).
  The resolved id_dist is the unjittered pinhole frame's (point 6): the existing frame constructors are its reference.

Measured (tests/test_lens_reference64.py, every pixel of 32x24 frames on dragon, the room from inside and the terrain
window, k in (1, 2, 7, 255, 2^32 - 1), with and without jitter): the largest float32 error over its bound is 0.47 for
an origin coordinate (room), 0.084 for a direction component of a lens ray (its bound is a sum of worst cases, dominated
by the frame's 6u through t and cosd), 0.44 for a pinhole direction against the frame's 6u, and 0.40 for a lens point over
k in 0..4095 and the four indices around 2^31 and 2^32 (MEASURED_RATIOS; the test prints them, asserts each <= 1 and
that none exceeds what is recorded here). No ratio above 1 was met, so no rounding had to be added to the derivation.

flaws= plants one plausible misreading at a time (LENS_FLAWS), so the tests can show that the comparison catches it."""
import numpy as np

import shader_ref64 as R

U = R.U
E_SINCOS = 1.2e-7           # absolute, det_sinf / det_cosf (path_ref64.E_SINCOS; measured there)
FRAME_DIR_ERR = 6.0 * U     # each component of a frame's float32 ray direction (shader_ref64's step error carries it)
PHI_ERR = 4.0 * U
MEASURED_RATIOS = {"origin": 0.466, "direction": 0.084, "pinhole_direction": 0.439, "disc": 0.397}

LENS_FLAWS = ("jitter_axes_swapped", "jitter_pixel_centre", "jitter_exact_add", "lens_no_shift", "lens_polys_swapped",
              "lens_square", "lens_focus_along_ray", "lens_origin_only", "lens_medium_at_eye", "lens_dim_from_eye",
              "lens_rng_sample0")
_M32 = (1 << 32) - 1


# ---- the sequences, exact ---------------------------------------------------------------------------------------------------
def jitter24(k):
    """-> (jx, jy) of sample k as 24-bit integers"""
    k = int(k) & _M32
    x = 0
    for i in range(32):
        x |= ((k >> i) & 1) << (31 - i)
    y, v, i = 0, 1 << 31, k
    while i:
        if i & 1:
            y ^= v
        i >>= 1
        v ^= v >> 1
    return x >> 8, y >> 8


def jx(k):
    return jitter24(k)[0] * 2.0 ** -24


def jy(k):
    return jitter24(k)[1] * 2.0 ** -24


def _direction_numbers(x2, x1, m):
    v = [m[i] << (31 - i) for i in range(3)]
    for i in range(3, 32):
        n = v[i - 3] ^ (v[i - 3] >> 3)
        if x2:
            n ^= v[i - 1]
        if x1:
            n ^= v[i - 2]
        v.append(n & _M32)
    return v


def lens24(k, flaws=()):
    """-> (lu, lv) of sample k as 24-bit integers"""
    k = int(k) & _M32
    pu, pv = (0, 1), (1, 0)                                  # (x^2 term, x term) of x^3+x+1 and of x^3+x^2+1
    if "lens_polys_swapped" in flaws:
        pu, pv = pv, pu
    out = []
    for (x2, x1), m in ((pu, (1, 1, 5)), (pv, (1, 3, 1))):
        D = _direction_numbers(x2, x1, m)
        g = 0
        for i in range(32):
            if (k >> i) & 1:
                g ^= D[i]
        out.append((g >> 8) if "lens_no_shift" in flaws else (g >> 8) ^ 0x800000)
    return out[0], out[1]


def lu(k):
    return lens24(k)[0] * 2.0 ** -24


def lv(k):
    return lens24(k)[1] * 2.0 ** -24


def disc(k, flaws=()):
    """the concentric map of sample k's lens point -> (lx, ly, bound on |lx32 - lx|, on |ly32 - ly|, centre)"""
    nu, nv = lens24(k, flaws)
    A, B = nu - (1 << 23), nv - (1 << 23)
    if A == 0 and B == 0:
        return 0.0, 0.0, 0.0, 0.0, True
    a, b = A * 2.0 ** -23, B * 2.0 ** -23
    if "lens_square" in flaws:
        return a, b, 0.0, 0.0, False
    c4, c2 = R._f32(0.785398163), R._f32(1.57079633)
    if abs(A) > abs(B):
        r, phi = a, c4 * (b / a)
    else:
        r, phi = b, c2 - c4 * (a / b)
    x, y = r * np.cos(phi), r * np.sin(phi)
    e = abs(r) * (E_SINCOS + PHI_ERR)
    return float(x), float(y), e + U * abs(x), e + U * abs(y), False


def pixel_positions(xs, ys, k, jitter, flaws=()):
    """float(px) + jx(k), float(py) + jy(k): ONE float32 addition each, rounded to nearest -> float64 values of the sums"""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    if not jitter:
        return xs.astype(np.float64), ys.astype(np.float64)
    ox, oy = jx(k), jy(k)
    if "jitter_axes_swapped" in flaws:
        ox, oy = oy, ox
    if "jitter_pixel_centre" in flaws:
        ox, oy = ox - 0.5, oy - 0.5
    if "jitter_exact_add" in flaws:
        return xs + ox, ys + oy
    fx = xs.astype(np.float32) + np.float32(ox)
    fy = ys.astype(np.float32) + np.float32(oy)
    assert fx.dtype == np.float32 and fy.dtype == np.float32
    return fx.astype(np.float64), fy.astype(np.float64)


# ---- the rays ---------------------------------------------------------------------------------------------------------------
class Rays:
    """xs, ys, W, H: the pixels; o[n, 3], d[n, 3]: float64 origin (world units) and unit direction; err_o[n, 3]: bound on
    the float32 origin (world units); dir_err[n]: what the tracers add to the frame's own direction error (0 for a pinhole
    ray); dir_bound[n]: the whole bound on a float32 direction component; moved[n]: the lens moved the ray; amb[n]: which
    of the two is undecided; rng_sample: initRNG's sample index; medium_org / measure_org: planted misreadings only"""


def lens_rays(inv_proj, inv_view, cam_pos, width, height, xs=None, ys=None, sample=0, jitter=False, aperture=0.0, focus=1.0,
              flaws=()):
    """sample `sample` of the accumulation for pixels (xs, ys) (default: the whole frame) of the float32 camera block"""
    unknown = set(flaws) - set(LENS_FLAWS)
    assert not unknown, unknown
    ry = Rays()
    ry.W, ry.H = int(width), int(height)
    if xs is None:
        ys, xs = np.mgrid[0:ry.H, 0:ry.W]
    ry.xs, ry.ys = np.asarray(xs, np.int64).ravel(), np.asarray(ys, np.int64).ravel()
    n = ry.xs.size
    P = np.array(inv_proj, np.float32).astype(np.float64).reshape(4, 4).T
    iv = np.array(inv_view, np.float32).astype(np.float64).ravel()
    e = np.array(cam_pos, np.float32).astype(np.float64)[:3]
    ap, fo = R._f32(aperture), R._f32(focus)
    fx, fy = pixel_positions(ry.xs, ry.ys, sample, jitter, flaws)
    d = R.ray_dirs(P, iv.reshape(4, 4).T, fx, fy, ry.W, ry.H)
    ry.fx, ry.fy, ry.eye = fx, fy, e
    ry.rng_sample = 0 if "lens_rng_sample0" in flaws else int(sample) & _M32
    ry.medium_org = ry.measure_org = None
    ry.o = np.tile(e, (n, 1))
    ry.d = d.copy()
    ry.err_o = np.zeros((n, 3))
    ry.dir_err = np.zeros(n)
    ry.dir_bound = np.full(n, FRAME_DIR_ERR)
    ry.moved = np.zeros(n, bool)
    ry.amb = np.zeros(n, bool)
    lx, ly, e_lx, e_ly, centre = disc(sample, flaws)
    ry.lx, ry.ly, ry.e_lx, ry.e_ly = lx, ly, e_lx, e_ly
    if ap == 0.0 or centre:
        return ry
    Rv, Uv, Zv = iv[0:3], iv[4:7], iv[8:11]                  # column-major, as given
    cosd = -(d @ Zv)
    e_cos = FRAME_DIR_ERR * np.abs(Zv).sum() + 4 * U * np.abs(d * Zv).sum(1)
    ry.amb = np.abs(cosd) <= e_cos
    mv = cosd > 0
    ry.moved = mv
    c = np.where(mv, cosd, 1.0)
    t = np.full(n, fo) if "lens_focus_along_ray" in flaws else fo / c
    e_t = t * (e_cos / np.maximum(c - e_cos, 1e-300) + U)
    td = t[:, None] * d
    p = e + td
    e_p = np.abs(d) * e_t[:, None] + (t * FRAME_DIR_ERR)[:, None] + U * np.abs(td) + U * np.abs(p)
    sx, sy = ap * lx, ap * ly
    s1 = e + sx * Rv
    o = s1 + sy * Uv
    e_o = (ap * (e_lx * np.abs(Rv) + e_ly * np.abs(Uv)) + U * (abs(sx) * np.abs(Rv) + abs(sy) * np.abs(Uv))
           + U * (np.abs(sx * Rv) + np.abs(sy * Uv) + np.abs(s1) + np.abs(o)))
    v = p - o
    ln = np.linalg.norm(v, axis=1)
    nd = v / ln[:, None]
    e_v = e_p + e_o + U * np.abs(v)
    e_n = np.minimum(e_v + np.abs(nd) * (np.abs(nd) * e_v).sum(1)[:, None], np.linalg.norm(e_v, axis=1)[:, None]) / ln[:, None]
    de = e_n.max(1) + 2 * R.GIVEN_DIR_ERR
    ry.o[mv] = o
    ry.err_o[mv] = e_o
    if "lens_origin_only" not in flaws:
        ry.d[mv] = nd[mv]
    ry.dir_err[mv] = de[mv]
    ry.dir_bound[mv] = de[mv]
    if "lens_medium_at_eye" in flaws:
        ry.medium_org = e
    if "lens_dim_from_eye" in flaws:
        ry.measure_org = e
    return ry


def trace(world, inv_proj, inv_view, cam_pos, width, height, xs=None, ys=None, sample=0, jitter=False, aperture=0.0, focus=1.0,
          flaws=(), **uniforms):
    """modes 0 and 1 of the sample -> shader_ref64.Trace (mode 2: path_ref64.PathTrace.lens on lens_rays' result)"""
    return R.Trace.lens(world, lens_rays(inv_proj, inv_view, cam_pos, width, height, xs, ys, sample, jitter, aperture, focus,
                                         flaws), **uniforms)


def with_frame_ids(sample_frame, pinhole_frame):
    """point 6: the resolved image has the sample's colour and the unjittered pinhole frame's (voxel ID, dist) -> a Frame
    whose colour fields are sample_frame's and whose ID and dist fields are pinhole_frame's (same pixels, same order)"""
    assert np.array_equal(sample_frame.xs, pinhole_frame.xs) and np.array_equal(sample_frame.ys, pinhole_frame.ys)
    f = type(sample_frame)(sample_frame.xs, sample_frame.ys, sample_frame.mode)
    f.__dict__.update(sample_frame.__dict__)
    f.id, f.dist, f.dec_id, f.dec_dist = pinhole_frame.id, pinhole_frame.dist, pinhole_frame.dec_id, pinhole_frame.dec_dist
    return f
