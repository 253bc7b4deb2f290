"""A float64 restatement of one sample's guide, plain and past glass (test helper, not a test).

Written from include/vrt.h ("guide planes" and rule G0-G6 under "Guides past glass") and from the GLSL lines the header cites
(comp:497, 505-507, 518-520, 547-572). It imports numpy, shader_ref64 (the decoded grid, ray_start, given_dirs, the floor rule),
path_ref64 (march(), the node-to-node hitMarching with its per-axis error, and the error constants of the glass branch) and
lens_ref64 (the rays of a jittered or thin-lens sample) and nothing else: nothing under oracle/, none of the C checkers, nothing of
the product (tests/test_shader_reference64.py enforces that).

What is restated. A chain of segments per ray:
  G0  segment 0 is the sample's own ray: gro = float32(origin * voxelScale), the start medium from the leaf at floor(gro)
      (shader_ref64.ray_start), the unit direction. S = 0, L = 0.
  G1  march() on the segment. A miss on any segment makes the sample a miss (ending "miss", S the surfaces passed before it).
  G2  the normal -sign(d[axis]) on the crossed axis ((0, 1, 0) for a zero normal); the bytes b: the hit leaf's R, G, B, A, or the
      previous voxel's where the hit leaf's alpha is 0; at the highlighted cell 255 - byte and alpha 255. d_j = |p - o| in world
      units, p = hitPoint / voxelScale and o the segment's origin (later segments: the grid-space origin of G5 / voxelScale), both
      divided only when the scale is not 1. L += d_j; A0 = b's alpha at S == 0; S += 1.
  G3  alpha 255: ends "opaque".      G4  S == 8: ends "cap".
  G5  n2 = the hit leaf's refraction where its alpha > 0 and the property > 0, else 1; n1 the same of the previous voxel (comp:503-504
      leave an alpha-0 hit leaf with property 1 and an alpha-0 previous voxel with property 0 because the ray's IOF is > 0: both read
      as 1.0, whatever byte the leaf stores, and n1 never comes from the ray's own medium). cosi = dot(d, normal) < 0 at every hit of
      hitMarching, so the flip and the swap never run; they are restated all the same. eta = n1 / n2, GLSL refract, R0, Schlick's
      term with a true pow, TIR where k < 0 (refract returns 0: its length is < 0.001). Ends "tir", "reflect" (reflect_i <= 0.001)
      or "refract" (refract_i <= 0.001 without TIR); otherwise the next segment starts at hitPoint - normal * 1e-4 along the
      refracted direction in medium n2.
  G6  hit; the final surface's normal, R, G, B and cell; A = A0; depth h(L) = min(max(0, L), 65504).
The plain guide (glass=False) is the same code stopped after G2 of segment 0: ending "opaque" or "first".

Error model: path_ref64's undecided rule, carried from segment to segment.
  * A segment is marched by path_ref64.march with its origin's per-axis bound err3 / lo3, its direction bound dir_err and its
    medium. Segment 0 takes ray_start's rounding (+ a computed origin's own bound, lens_ref64's err_o in grid units); a caller's
    direction has R.GIVEN_DIR_ERR, a frame's 0 (shader_ref64's step error carries its ~6u), a lens ray lens_ref64's dir_err.
  * A continued segment starts at hitPoint - normal * 1e-4: the hit's per-axis bound (march's err3 at the hit) plus u |o| for
    that sum's rounding. Its direction bound is path_ref64._spawn_glass's: dir_err (eta + eta^2 |cos| / sqrt k) + 8u +
    4u (1 + eta^2) / sqrt k. The refracted direction is used "as given" by the rule; its float32 length is 1 within a few u,
    which the step error's 10u t holds.
  * Undecided, with the Fresnel error e_F of path_ref64._pass (R0's quotient terms, E_POW * pow, 5 (1 - cos)^4 (dir_err + 8u),
    3u): reflect_i and (without TIR) refract_i within e_F of 0.001; k within 6u (1 + eta^2) + 2 eta^2 |cos| (dir_err + 8u) of 0;
    |cosi| below dir_err + DIR_MARGIN; and whatever march() leaves undecided (floors, small components, the step cap).
  * The cell needs its own rule. R._floor_undecided asks whether a near-integer coordinate changes the NODE; inside a leaf larger
    than one voxel the cell differs while the node does not (materials_1 ray 384 lands at z = 12.99999987 in a 2 x 2 x 2 leaf: the
    float32 run floors 13, float64 floors 12). cell_near marks a hit whose point has any coordinate within DELTA_FLOOR +
    DELTA_SAFETY * err of an integer; the cell of such a ray is not compared, and the ray itself is undecided only where the
    highlighted voxel is one of the candidate cells but not all of them (the inversion then depends on the floor).
  * Depth. One segment's float32 length d_j differs from this module's by at most
        b_j = ((sqrt 3 + 1 / |d[ax]|) e + line) / |scale| + |e_o|_2 + 2 sqrt(3) u (|p|_max + |o|_max) + 4u d_j,
    e = DELTA_FLOOR + DELTA_SAFETY * (the largest per-axis bound of the hit point, not below the line's lo3): sqrt(3) e for the
    point's three coordinates and e / |d[ax]| for the last crossing, whose t = (plane - pos[ax]) / d[ax] carries pos[ax]'s error
    along the ray (tests/test_guides.py derives both for the plain guide); line = march's m.line, what the float32 run's own
    line has drifted across the ray; e_o the segment origin's bound in world units (0 for a caller's origin, lens_ref64's err_o
    for a lens ray, (err3 of the continued origin) / |scale| + u |o| for the division afterwards); the divisions of p and o by
    the scale and the subtraction round once per coordinate (2 sqrt(3) u of the larger coordinate), and the squares, the two
    sums and the square root stay within 4u of the length. The running sum L = L + d_j rounds once more: u L. So
        B = sum_j (b_j + u L_j)
    bounds |L32 - L|, and h is 1-Lipschitz. Nothing in B is fitted to a run; MEASURED_RATIOS records the largest observed
    error / B per input (tests/test_guides_reference64.py prints them and asserts each <= 1).

resolve() restates the header's resolve over n samples: float64 divisions and one rounding. Where all n samples of a pixel are
decided, normal, albedo and coverage are exact bits; the depth lies within the mean of the hit samples' bounds plus u |depth| for
the one float32 rounding. A pixel with any undecided sample is left out.

GUIDE_FLAWS plants one misreading at a time: ratio_inverted (n2 / n1), depth_straight (the straight distance from the sample's
origin to the final point), alpha_of_final (A from the final surface), nudge_outwards (+ normal * 1e-4), miss_is_glass (a miss
behind glass reported as the last glass surface), cap_9, grid_origin (later segments' origins left in grid units when the scale
is not 1), n1_ray_medium (n1 from the ray's medium where the previous voxel's alpha-0 rule gives 1)."""
import numpy as np

import lens_ref64 as LR
import path_ref64 as PR
import shader_ref64 as R

U = R.U
MAX_SURFACES = 8
HDR_MAX = R.HDR_MAX
ENDINGS = ("miss", "opaque", "cap", "tir", "reflect", "refract", "first")
MISS, OPAQUE, CAP, TIR, REFLECT, REFRACT, FIRST = range(7)
GUIDE_FLAWS = ("ratio_inverted", "depth_straight", "alpha_of_final", "nudge_outwards", "miss_is_glass", "cap_9", "grid_origin",
               "n1_ray_medium")
# the largest |float32 depth - L| / B over the decided hits of each input (tests/test_guides_reference64.py, the checker; the
# device gives the checker's bits): frames over the four sources at samples 5 and 12 and both sizes, batches with the setting on
MEASURED_RATIOS = {"room": 0.222, "lamp": 0.031, "outside": 0.376, "room_wall": 0.021, "panes_30": 0.001, "dragon_mix": 0.153,
                   "room_mix": 0.068, "materials_1": 0.061, "materials_0.5": 0.061, "materials_2": 0.061, "scale_3": 0.073,
                   "bounds_mix": 0.116, "near_index": 0.008, "alpha0": 0.004, "grazing": 0.058}


def fresnel_shares(n1, n2, cos_t):
    """comp:528-535 for an entering ray with cosTheta = cos_t >= 0 (the normal faces the ray): -> (reflect_i, refract_i, k, R0)
    in float64; k < 0 is TIR, where refract_i is 0"""
    n1, n2, c = (np.asarray(v, np.float64) for v in (n1, n2, cos_t))
    eta = n1 / n2
    k = 1.0 - eta * eta * (1.0 - c * c)
    R0 = (n1 - n2) / (n1 + n2) * (n1 - n2) / (n1 + n2)
    fres = np.clip(R0 + (1.0 - R0) * (1.0 - c) ** 5, 0.0, 1.0)
    return fres, np.where(k < 0.0, 0.0, 1.0 - fres), k, R0


class GuideTrace:
    """One sample's guide of every ray. Per ray: hit, cell[3], normal[3], rgb[3] (bytes), a0, a_final, S, end (ENDINGS),
    L (the bent path's length) and bound (B), straight; outside, amb, cell_near, first_hit, through (the segment-0 hit is decided
    and translucent), first_translucent (whatever is decided)."""

    def __init__(self, world, inv_proj, inv_view, cam_pos, width, height, xs=None, ys=None, voxel_scale=1.0,
                 highlighted=(-1, -1, -1), glass=True, flaws=()):
        """a frame's corner rays: one origin (cameraPos), ray_dirs' directions"""
        self._uniforms(world, voxel_scale, highlighted, glass, flaws)
        self.W, self.H = int(width), int(height)
        if xs is None:
            ys, xs = np.mgrid[0:self.H, 0:self.W]
        self.xs, self.ys = np.asarray(xs, np.int64).ravel(), np.asarray(ys, np.int64).ravel()
        cam = np.array(cam_pos, np.float32).astype(np.float64)[:3]
        P = np.array(inv_proj, np.float32).astype(np.float64).reshape(4, 4).T
        Vw = np.array(inv_view, np.float32).astype(np.float64).reshape(4, 4).T
        self._run(cam, R.ray_dirs(P, Vw, self.xs, self.ys, self.W, self.H), given=False)

    @classmethod
    def lens(cls, world, rays, voxel_scale=1.0, highlighted=(-1, -1, -1), glass=True, flaws=()):
        """a jittered and / or thin-lens sample: `rays` is lens_ref64.lens_rays' result (err_o, dir_err and amb enter as they do
        in PathTrace.lens)"""
        self = cls.__new__(cls)
        self._uniforms(world, voxel_scale, highlighted, glass, flaws)
        self.W, self.H, self.xs, self.ys = rays.W, rays.H, rays.xs, rays.ys
        self._run(rays.o, rays.d, given=False, err3=rays.err_o * abs(self.scale) + U * np.abs(rays.o * self.scale),
                  dir_err=rays.dir_err, amb=rays.amb, err_o=rays.err_o)
        return self

    @classmethod
    def sample(cls, world, inv_proj, inv_view, cam_pos, width, height, sample, jitter=False, aperture=0.0, focus=1.0, **kw):
        """sample `sample` of an accumulation: the corner rays, or lens_ref64's where the sample is jittered or has a lens"""
        if not jitter and float(aperture) == 0.0:
            return cls(world, inv_proj, inv_view, cam_pos, width, height, **kw)
        return cls.lens(world, LR.lens_rays(inv_proj, inv_view, cam_pos, width, height, None, None, sample, jitter, aperture, focus), **kw)

    @classmethod
    def rays(cls, world, origins, dirs, voxel_scale=1.0, highlighted=(-1, -1, -1), glass=True, flaws=()):
        """a caller's batch: origins float32 (n, 3) or (3,) shared, in world units; dirs float32 (n, 3) as given"""
        self = cls.__new__(cls)
        self._uniforms(world, voxel_scale, highlighted, glass, flaws)
        d, _ = R.given_dirs(dirs)
        self._run(np.array(origins, np.float32).astype(np.float64), d, given=True)
        return self

    def _uniforms(self, world, voxel_scale, highlighted, glass, flaws):
        unknown = set(flaws) - set(GUIDE_FLAWS)
        assert not unknown, unknown
        self.w, self.flaws, self.glass = world, frozenset(flaws), bool(glass)
        self.scale = float(np.float32(voxel_scale))
        self.hl = np.array(highlighted, np.int64)

    def _to_world(self, p):
        """each component divided by u_voxelScale only when the scale is not 1"""
        return p / self.scale if self.scale != 1.0 else p

    def _cell_rule(self, idx, pt, mp, perr):
        """-> near[k]: a coordinate of the hit point lies within the floor margin of an integer; rays for which the highlighted
        voxel is one candidate cell but not every one become undecided"""
        margin = R.DELTA_FLOOR + R.DELTA_SAFETY * perr
        near = np.abs(pt - np.rint(pt)) < margin
        rows = np.nonzero(near.any(1))[0]
        if rows.size and np.all(self.w.in_world(self.hl[None])):
            is_hl = np.all(mp[rows] == self.hl, 1)
            differs = np.zeros(rows.size, bool)
            for sub in R._SUBSETS:
                ok = np.all(near[rows][:, list(sub)], 1)
                alt = mp[rows].copy()
                for j in sub:
                    alt[:, j] += np.where(pt[rows, j] >= np.rint(pt[rows, j]), -1, 1)
                differs |= ok & (np.all(alt == self.hl, 1) != is_hl)
            self.amb[idx[rows[differs]]] = True
        return near.any(1)

    def _run(self, origins, d, given, err3=None, dir_err=None, amb=None, err_o=None):
        w, n, fl = self.w, d.shape[0], self.flaws
        scale = abs(self.scale)
        cap = MAX_SURFACES + 1 if "cap_9" in fl else MAX_SURFACES
        self.org = np.broadcast_to(origins.reshape(-1, 3), (n, 3)).copy()
        st = R.ray_start(w, self.org, self.scale, (), err3)
        self.outside = st.outside
        self.amb = st.amb | (R.dir_undecided(d, given) & ~st.outside)
        if amb is not None:
            self.amb = self.amb | amb
        org = np.where(st.outside[:, None], 0.0, st.gro)
        e3, lo3 = st.err.copy(), st.err.copy()
        dd = np.where(st.outside[:, None], 1.0, d)
        de = np.full(n, R.GIVEN_DIR_ERR) if given else (np.zeros(n) if dir_err is None else np.asarray(dir_err, np.float64).copy())
        iof = st.iof.copy()
        giv = np.full(n, 1 if given else 0, np.int64)
        ow = self.org.copy()
        eow = np.zeros((n, 3)) if err_o is None else np.asarray(err_o, np.float64).copy()
        self.hit = np.zeros(n, bool)
        self.cell = np.zeros((n, 3), np.int64)
        self.normal = np.zeros((n, 3), np.int64)
        self.rgb = np.zeros((n, 3), np.int64)
        self.a0 = np.zeros(n, np.int64)
        self.a_final = np.zeros(n, np.int64)
        self.S = np.zeros(n, np.int64)
        self.end = np.full(n, MISS, np.int64)
        self.L = np.zeros(n)
        self.bound = np.zeros(n)
        self.straight = np.zeros(n)
        self.cell_near = np.zeros(n, bool)
        self.first_hit = np.zeros(n, bool)
        self.first_translucent = np.zeros(n, bool)
        self.through = np.zeros(n, bool)
        alive = ~st.outside
        minus = np.full(n, -1, np.int64)
        for seg in range(cap + 1):
            act = np.nonzero(alive & ~self.amb)[0]
            if not act.size:
                break
            m = PR.march(w, org[act], e3[act], dd[act], de[act], iof[act], minus[act], minus[act], np.zeros(act.size), lo3[act], giv[act])
            self.amb[act] |= m.amb
            ok = ~m.amb
            mi = act[ok & ~m.hit]                                                 # G1
            alive[mi] = False
            if "miss_is_glass" in fl:
                self.hit[mi] = self.S[mi] > 0
            hi = np.nonzero(ok & m.hit)[0]
            if not hi.size:
                continue
            idx = act[hi]
            k = hi.size
            kr = np.arange(k)
            dv, ax, pt, mp, hv, lv, perr = dd[idx], m.ax[hi], m.pt[hi], m.mp[hi], m.hv[hi], m.lv[hi], m.err3[hi]
            # ---- G2 ----
            s = -np.sign(dv[kr, ax])
            normal = np.zeros((k, 3))
            normal[kr, ax] = s
            normal[s == 0] = (0.0, 1.0, 0.0)                                      # comp:497
            hva = w.a[hv] > 0
            rgb = np.where(hva[:, None], w.rgb[hv], w.rgb[lv])                    # comp:505-507
            al = np.where(hva, w.a[hv], w.a[lv])
            hl = np.all(mp == self.hl, 1)                                         # comp:518-520
            rgb = np.where(hl[:, None], 255 - rgb, rgb)
            al = np.where(hl, 255, al)
            near = self._cell_rule(idx, pt, mp, perr)
            hpw = self._to_world(pt)
            v = hpw - ow[idx]
            dj = np.sqrt((v * v).sum(1))
            e = R.DELTA_FLOOR + R.DELTA_SAFETY * np.maximum(perr, lo3[idx]).max(1)
            dax = np.maximum(np.abs(dv[kr, ax]), 1e-30)
            bj = ((np.sqrt(3.0) + 1.0 / dax) * e + m.line[hi]) / scale + np.linalg.norm(eow[idx], axis=1) \
                + 2.0 * np.sqrt(3.0) * U * (np.abs(hpw).max(1) + np.abs(ow[idx]).max(1)) + 4.0 * U * dj
            self.amb[idx] |= ~np.isfinite(bj)
            self.L[idx] += dj
            self.bound[idx] += np.where(np.isfinite(bj), bj, 0.0) + U * self.L[idx]
            self.straight[idx] = np.linalg.norm(hpw - self.org[idx], axis=1)
            first = self.S[idx] == 0
            self.a0[idx] = np.where(first, al, self.a0[idx])
            self.first_hit[idx[first]] = True
            self.first_translucent[idx[first]] = al[first] < 255
            self.through[idx[first]] = (al[first] < 255) & ~self.amb[idx[first]]
            self.S[idx] += 1
            self.cell[idx], self.normal[idx], self.rgb[idx], self.a_final[idx] = mp, normal.astype(np.int64), rgb, al
            self.cell_near[idx] = near
            # ---- G3, G4 (and the plain guide, which stops here) ----
            end = np.full(k, -1, np.int64)
            end[al == 255] = OPAQUE
            if not self.glass:
                end[end < 0] = FIRST
            end[(end < 0) & (self.S[idx] == cap)] = CAP
            # ---- G5 ----
            g = np.nonzero(end < 0)[0]
            if g.size:
                n2 = np.where(w.refractive[hv[g]], w.refr[hv[g]], 1.0)           # comp:503, 507
                n1 = np.where(w.refractive[lv[g]], w.refr[lv[g]], 1.0)           # comp:504, 508
                if "n1_ray_medium" in fl:
                    n1 = np.where(w.refractive[lv[g]], n1, iof[idx[g]])
                dg, ng = dv[g], normal[g].copy()
                cosi = np.einsum("ij,ij->i", dg, ng)                              # comp:522-526
                derr = de[idx[g]] + 8 * U
                und = np.abs(cosi) < de[idx[g]] + R.DIR_MARGIN
                flip = cosi > 0
                ng[flip] = -ng[flip]
                n1, n2 = np.where(flip, n2, n1), np.where(flip, n1, n2)
                eta = n2 / n1 if "ratio_inverted" in fl else n1 / n2
                c = np.einsum("ij,ij->i", ng, dg)
                kk = 1.0 - eta * eta * (1.0 - c * c)
                tir = kk < 0.0
                sq = np.sqrt(np.maximum(kk, 0.0))
                refr = eta[:, None] * dg - (eta * c + sq)[:, None] * ng
                cos_t = np.maximum(0.0, -c)
                refl_i, refr_i, _, R0 = fresnel_shares(n1, n2, cos_t)
                refr_i = np.where(tir, 0.0, 1.0 - refl_i)                         # has_tir follows refract's k, whichever ratio it took
                pw = (1.0 - cos_t) ** 5
                e_f = (R0 * (8 * U + 4 * U * (n1 + n2) / np.where(n1 != n2, np.abs(n1 - n2), 1.0)) + PR.E_POW * pw + PR.E_POW_ABS
                       + 5.0 * (1.0 - cos_t) ** 4 * derr + 3 * U)
                und |= (np.abs(refl_i - 0.001) <= e_f) | (~tir & (np.abs(refr_i - 0.001) <= e_f))
                und |= np.abs(kk) <= 6 * U * (1 + eta ** 2) + 2 * eta ** 2 * np.abs(c) * derr
                self.amb[idx[g]] |= und
                eg = np.where(tir, TIR, np.where(refl_i <= 0.001, REFLECT, np.where(refr_i <= 0.001, REFRACT, -1)))
                end[g] = eg
                q = g[eg < 0]                                                     # the chain goes on
                if q.size:
                    qg = np.nonzero(eg < 0)[0]
                    j = idx[q]
                    sign = 1.0 if "nudge_outwards" in fl else -1.0
                    o = pt[q] + sign * ng[qg] * 1e-4
                    org[j] = o
                    e3[j] = lo3[j] = perr[q] + U * np.abs(o)
                    dd[j] = refr[qg] / np.linalg.norm(refr[qg], axis=1, keepdims=True)
                    de[j] = de[j] * (eta[qg] + eta[qg] ** 2 * np.abs(c[qg]) / sq[qg]) + 8 * U + 4 * U * (1 + eta[qg] ** 2) / sq[qg]
                    iof[j] = n2[qg]
                    giv[j] = 0
                    ow[j] = o if "grid_origin" in fl else self._to_world(o)
                    eow[j] = e3[j] / scale + U * np.abs(ow[j])
            done = end >= 0
            j = idx[done]
            self.end[j] = end[done]
            self.hit[j] = True
            alive[j] = False
        assert not (alive & ~self.amb).any()

    # ---- what a comparison reads ----------------------------------------------------------------------------------------------
    @property
    def decided(self):
        return ~self.amb & ~self.outside

    def alpha(self):
        return self.a_final if "alpha_of_final" in self.flaws else self.a0

    def depth(self):
        """-> (h(L) float64[n] (0 on a miss), bound[n])"""
        L = self.straight if "depth_straight" in self.flaws else self.L
        return np.where(self.hit, np.clip(L, 0.0, HDR_MAX), 0.0), self.bound

    def bytes4(self):
        """-> the four albedo bytes int64[n, 4], zeros on a miss"""
        return np.where(self.hit[:, None], np.concatenate([self.rgb, self.alpha()[:, None]], 1), 0)

    def normals(self):
        return np.where(self.hit[:, None], self.normal, 0)

    def planes(self):
        """a batch's planes of n = 1 -> dict: normal float32[n, 3], albedo float32[n, 4] = float32(byte / 255.0), hit bool[n],
        depth float64[n] with depth_bound[n] (B as it is: the plane is the float32 h(L) itself, no further rounding), decided[n]"""
        depth, bound = self.depth()
        return {"normal": self.normals().astype(np.float32), "albedo": (self.bytes4() / 255.0).astype(np.float32), "hit": self.hit.copy(),
                "depth": depth, "depth_bound": bound, "decided": self.decided}

    def endings(self, mask=None):
        """-> {ending: count} over the decided rays (of mask)"""
        sel = self.decided if mask is None else self.decided & mask
        return {name: int((self.end[sel] == i).sum()) for i, name in enumerate(ENDINGS)}

    def left_out(self):
        """-> (share of the in-world rays that are undecided, share of the rays whose segment-0 hit is decided and translucent)"""
        inw = ~self.outside
        a = float(self.amb[inw].mean()) if inw.any() else 0.0
        b = float(self.amb[self.through].mean()) if self.through.any() else 0.0
        return a, b


def resolve(samples):
    """the planes of n samples (GuideTrace objects of the same rays) by the header's resolve: float64 divisions, one rounding
    -> dict: normal float32[n, 3], albedo float32[n, 4], coverage float32[n] (exact bits where decided), depth float64[n] with
    depth_bound[n] (the mean of the hit samples' bounds + u |depth|), decided[n] (every sample decided)"""
    n = len(samples)
    nsum = sum(s.normals() for s in samples)
    asum = sum(s.bytes4() for s in samples)
    hits = sum(s.hit.astype(np.int64) for s in samples)
    dsum = sum(s.depth()[0] for s in samples)
    bsum = sum(np.where(s.hit, s.bound, 0.0) for s in samples)
    has = hits > 0
    depth = np.where(has, dsum / np.maximum(hits, 1), 0.0)
    return {"normal": (nsum / float(n)).astype(np.float32), "albedo": (asum / (255.0 * n)).astype(np.float32),
            "coverage": (hits / float(n)).astype(np.float32), "depth": depth,
            "depth_bound": np.where(has, bsum / np.maximum(hits, 1), 0.0) + U * np.abs(depth),
            "decided": np.all([s.decided for s in samples], axis=0)}
