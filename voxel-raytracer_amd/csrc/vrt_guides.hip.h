// vrt_guides.hip.h -- the guide planes (include/vrt.h vrt_accum_guides, vrt_guide_rays): per sample the first hit's normal, surface
// colour bytes and depth, taken from the depth-0 march of the sample's own ray and from nothing else. A kernel of its own beside
// the accumulation's: the ray is the one pixel_ray<JIT, LENS>() hands trace_pixel() -- the same three sources (vrt_accum.hip.h
// CornerSource, JitterSource, LensSource), or a caller's ray through rays::RaySource (vrt_rays.hip.h) -- the march is TRAV::march()
// with the start medium of that ray, and what follows the march is the few lines of trace_pixel() that name the surface
// (comp:497, 505-507, the highlighted voxel), restated on bytes: no shading, no shadow ray, no random number.
//
// One lane per pixel (or ray), 8 x 8 tiles, no LDS, no barrier, no atomics. Over a frame a lane reads its pixel's ten state words
// (vrt_guides.h State) once, adds the launch's samples and writes them back once. The jitter and lens sources loop the samples in the
// lane and re-read the arguments per trip (accum::loop_args() / loop_view()); the corner source's ray is the same for every sample,
// so it marches once and adds the guide n times over: the integer sums take n * value, the float64 depth sum (double)h(d) * n, which
// equals the n sequential adds bit for bit -- every partial sum m * h(d), m <= 2^24, is exact in a double (24 x 24 bits), as in
// accum::add_hdr_repeat().
#pragma once
#include "vrt_accum.hip.h"
#include "vrt_guides.h"
#include "vrt_rays.hip.h"

namespace vrt {
namespace guides {

// One sample's guide. bytes: the surface colour's R | G<<8 | B<<16 | A<<24.
struct Guide {
    bool hit;
    int axis;        // the normal: sign on this axis
    int sign;        // +1 or -1
    uint32_t bytes;
    float depth;     // h(distance from the ray's origin), world units
};

// The caller's rays as a source of guide_kernel: the mapping of rays::ray_of_lane() needs n, width and tiles_x only
struct RaySource {
    static constexpr bool kJitter = false, kLens = false;
};
template <class SRC> struct is_rays { static constexpr bool value = false; };
template <> struct is_rays<RaySource> { static constexpr bool value = true; };
template <class SRC> using ArgsFor = typename std::conditional<is_rays<SRC>::value, RayArgs, Args>::type;

// The depth-0 march of `pr` as trace_pixel() makes it, and the surface it names
template <class TRAV>
VRT_DEV Guide guide_of_ray(const KArgs &a, const View &vw, const typename TRAV::Ctx &tc_, const LensRay &pr) {
    const F3 gro = scale3(pr.o, a.voxel_scale);
    // medium at the origin (comp:445-449), as trace_pixel() reads it from the leaf words
    const float r0 = unorm_of((float)(pr.eye1 & 0xffu)) * 3.0f;
    const float start_iof = (r0 > 0.0f && r0 < 3.0f) ? r0 : 1.0f;
    const uint32_t eye_b = pr.eye1 & 0xffu;
    const uint32_t iof_byte = (eye_b >= 1u && eye_b <= 254u) ? eye_b : 85u;
    Hit h;
    Guide g;
    g.hit = TRAV::march(a, tc_, gro, pr.dir, start_iof, iof_byte, h, &vw);
    g.axis = 1; g.sign = 1; g.bytes = 0u; g.depth = 0.0f;
    if (g.hit) {
        // normal = length(hitNormal) > 0 ? hitNormal : (0,1,0)  (comp:497)
        if (__builtin_fabsf(h.n) > 0.0f) { g.axis = h.axis; g.sign = h.n > 0.0f ? 1 : -1; }
        const LateArgs la = late_args();   // read after the march: not live across it
        const float scale = la->voxel_scale;
        F3 hpw = h.point;
        if (scale != 1.0f) hpw = F3{h.point.x / scale, h.point.y / scale, h.point.z / scale};
        g.depth = accum::hdr_value(len3(sub3(hpw, pr.o)));
        // surfaceColor = hitVoxel.color.a > 0 ? hitVoxel.color : lastVoxel.color (comp:505-507), all four bytes
        g.bytes = (h.h0 >> 24) != 0u ? h.h0 : h.p0;
        if (h.map.x == la->highlighted[0] && h.map.y == la->highlighted[1] && h.map.z == la->highlighted[2])
            g.bytes = (~g.bytes & 0x00ffffffu) | 0xff000000u;   // 1 - c per channel is 255 - byte; alpha 1
    }
    return g;
}

// Guides past glass (include/vrt.h vrt_set_guide_glass, rule G0-G6): the chain of `pr` through translucent surfaces along the
// refracted ray, up to kMaxSurfaces of them, and the surface it ends on. Every segment takes the traversal's general march -- a
// continuation starts inside a medium, so v4's one-loop form (every lane in refraction 1.0) is not for it, and one march in the loop
// keeps one set of its registers; the general march gives segment 0 the hit the one-loop form gives it. What follows a translucent
// hit is comp:547-572 as trace_pixel() has it (vrt_full.hip.h), without its ray stack: the alpha-0 rules, n1 and n2, the flip, the
// refracted direction, Fresnel's two shares and the shader's "spawns nothing" test. The trips of the loop are wave-uniform (the
// lanes of a wave are all on segment S); lanes whose chain has ended wait for the longest of their wave.
constexpr int kMaxSurfaces = VRT_GUIDE_MAX_SURFACES;
template <class TRAV> struct general_of { using type = TRAV; };
template <> struct general_of<v4::Trav> { using type = v4::TravAny; };

template <class TRAV>
VRT_DEV Guide guide_past_glass(const KArgs &a, const View &vw, const typename TRAV::Ctx &tc_, const LensRay &pr) {
    using T = typename general_of<TRAV>::type;
    // G0: segment 0 is the sample's own ray, its medium the leaf's at the origin (comp:445-449)
    const float r0 = unorm_of((float)(pr.eye1 & 0xffu)) * 3.0f;
    float iof = (r0 > 0.0f && r0 < 3.0f) ? r0 : 1.0f;
    const uint32_t eye_b = pr.eye1 & 0xffu;
    uint32_t iof_byte = (eye_b >= 1u && eye_b <= 254u) ? eye_b : 85u;
    F3 gro = scale3(pr.o, a.voxel_scale);   // the segment's origin in grid units
    F3 ow = pr.o;                           // ... and in world units
    F3 dir = pr.dir;
    float total = 0.0f;                     // L
    uint32_t a0 = 0u;
    Guide g;
    g.hit = false; g.axis = 1; g.sign = 1; g.bytes = 0u; g.depth = 0.0f;
    for (int s = 0; s < kMaxSurfaces; ++s) {
        Hit h;
        // G1: a miss on any segment is a miss of the sample
        if (!T::march(a, tc_, gro, dir, iof, iof_byte, h, s == 0 ? &vw : nullptr)) return g;
        // G2: the surface, as guide_of_ray() names it
        const LateArgs la = late_args();   // read after the march: not live across it
        const float scale = la->voxel_scale;
        F3 hpw = h.point;
        if (scale != 1.0f) hpw = F3{h.point.x / scale, h.point.y / scale, h.point.z / scale};
        total = total + len3(sub3(hpw, ow));
        uint32_t b = (h.h0 >> 24) != 0u ? h.h0 : h.p0;
        if (h.map.x == la->highlighted[0] && h.map.y == la->highlighted[1] && h.map.z == la->highlighted[2])
            b = (~b & 0x00ffffffu) | 0xff000000u;
        if (s == 0) a0 = b >> 24;
        F3 normal{0.0f, 1.0f, 0.0f};
        int axis = 1;
        if (__builtin_fabsf(h.n) > 0.0f) {
            axis = h.axis;
            normal = F3{h.axis == 0 ? h.n : 0.0f, h.axis == 1 ? h.n : 0.0f, h.axis == 2 ? h.n : 0.0f};
        }
        // G3, G4: an opaque surface, or the last surface the chain may take, ends it
        bool last_surface = (b >> 24) == 255u || s == kMaxSurfaces - 1;
        F3 refr_dir{0.0f, 0.0f, 0.0f};
        float n2 = 1.0f;
        F3 flipped = normal;
        if (!last_surface) {   // G5 (comp:547-572)
            float hv_r = unorm_of((float)(h.h1 & 0xffu)) * 3.0f, last_r = unorm_of((float)(h.p1 & 0xffu)) * 3.0f;
            if ((h.h0 >> 24) == 0u) hv_r = 1.0f;
            if ((h.p0 >> 24) == 0u) last_r = iof > 0.0f ? 0.0f : 1.0f;
            n2 = hv_r > 0.0f ? hv_r : 1.0f;
            float n1 = last_r > 0.0f ? last_r : 1.0f;
            if (dot3(dir, normal) > 0.0f) { flipped = F3{-normal.x, -normal.y, -normal.z}; const float t = n1; n1 = n2; n2 = t; }
            refr_dir = full::refract3(dir, flipped, n1 / n2);
            const float R0 = (n1 - n2) / (n1 + n2) * (n1 - n2) / (n1 + n2);
            const F3 ninc{-dir.x, -dir.y, -dir.z};
            const float cos_t = fmax_c(0.0f, dot3(ninc, flipped));
            float fres = R0 + (1.0f - R0) * full::det_powf(1.0f - cos_t, 5.0f);
            fres = fmin_c(fmax_c(fres, 0.0f), 1.0f);
            const bool has_tir = len3(refr_dir) < 0.001f;
            const float reflect_i = fres;
            const float refract_i = has_tir ? 0.0f : (1.0f - fres);
            last_surface = reflect_i <= 0.001f || refract_i <= 0.001f;   // the shader shades this surface and spawns nothing
        }
        if (last_surface) {   // G6
            g.hit = true;
            g.axis = axis; g.sign = comp(normal, axis) > 0.0f ? 1 : -1;
            g.bytes = (b & 0x00ffffffu) | (a0 << 24);
            g.depth = accum::hdr_value(total);
            return g;
        }
        gro = sub3(h.point, scale3(flipped, 1e-4f));
        ow = gro;
        if (scale != 1.0f) ow = F3{gro.x / scale, gro.y / scale, gro.z / scale};
        dir = refr_dir;
        iof = n2;
        iof_byte = full::iof_to_byte(n2);
    }
    return g;   // not reached: the trip of s == kMaxSurfaces - 1 returns
}

// SRC: accum::CornerSource / JitterSource / LensSource over a frame (q: Args; L...: the Lens, as primary_accum_kernel takes it), or
// RaySource over a caller's batch (q: RayArgs; one march, the planes of one sample stored by the lane). GLASS: the guide of every
// sample is guide_past_glass()'s.
template <bool GLASS, class TRAV>
VRT_DEV Guide guide_of(const KArgs &a, const View &vw, const typename TRAV::Ctx &tc_, const LensRay &pr) {
    if constexpr (GLASS) return guide_past_glass<TRAV>(a, vw, tc_, pr);
    else return guide_of_ray<TRAV>(a, vw, tc_, pr);
}

template <class SRC, class TRAV, int BLOCK, int WPE, bool GLASS, class... L>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(WPE))) void guide_kernel(const KArgs a, const ViewSet vs, const ArgsFor<SRC> q, const L... lens) {
    typename TRAV::Ctx tc_;
    TRAV::block_init(a, tc_);
    if constexpr (is_rays<SRC>::value) {
        rays::Args m{};   // what ray_of_lane() and RaySource::load() read
        m.origins = q.origins; m.dirs = q.dirs; m.n = q.n; m.origin_stride = q.origin_stride; m.width = q.width; m.tiles_x = q.tiles_x;
        uint32_t i;
        int px, py;
        if (!rays::ray_of_lane(m, i, px, py)) return;
        const LensRay lr = rays::RaySource::load(a, m, i);
        const Guide g = guide_of<GLASS, TRAV>(a, vs.v[0], tc_, lr);
        if (q.out_hit) q.out_hit[i] = g.hit ? 1 : 0;
        if (q.out_normal) {
            const float s = g.hit ? (float)g.sign : 0.0f;
            float *p = q.out_normal + (size_t)i * 3u;
            p[0] = g.axis == 0 ? s : 0.0f; p[1] = g.axis == 1 ? s : 0.0f; p[2] = g.axis == 2 ? s : 0.0f;
        }
        if (q.out_albedo) {
            float *p = q.out_albedo + (size_t)i * 4u;
#pragma unroll
            for (int k = 0; k < 4; ++k) p[k] = (float)((double)((g.bytes >> (8 * k)) & 0xffu) / 255.0);
        }
        if (q.out_depth) q.out_depth[i] = g.depth;
    } else {
        const SRC src{lens...};
        int px, py;
        if (!accum::frame_pixel<BLOCK>(a, px, py)) return;
        const size_t o = accum::pixel_offset(a, px, py);
        uint4 as = q.st.albedo[o];
        int4 ns = q.st.normal[o];
        double ds = q.st.depth[o];
        constexpr bool kLoop = SRC::kJitter || SRC::kLens;   // the corner's ray does not depend on the sample
        const uint32_t trips = kLoop ? q.n : 1u;
        for (uint32_t k = 0; k < trips; ++k) {
            Guide g;
            uint32_t times = 1u;
            if constexpr (kLoop) {
                const KArgs ak = accum::loop_args(a);
                const View vk = accum::loop_view(vs);
                if constexpr (SRC::kLens) {
                    const LensRay lr = accum::lens_sample(ak, vk, src.L, px, py, q.first + k);
                    g = guide_of<GLASS, TRAV>(ak, vk, tc_, pixel_ray<false, true>(ak, vk, px, py, q.first + k, &lr));
                } else {
                    g = guide_of<GLASS, TRAV>(ak, vk, tc_, pixel_ray<true, false>(ak, vk, px, py, q.first + k, nullptr));
                }
            } else {
                g = guide_of<GLASS, TRAV>(a, vs.v[0], tc_, pixel_ray<false, false>(a, vs.v[0], px, py, q.first, nullptr));
                times = q.n;
            }
            if (g.hit) {
                as.x += (g.bytes & 0xffu) * times; as.y += ((g.bytes >> 8) & 0xffu) * times;
                as.z += ((g.bytes >> 16) & 0xffu) * times; as.w += (g.bytes >> 24) * times;
                const int d = g.sign * (int)times;
                ns.x += g.axis == 0 ? d : 0; ns.y += g.axis == 1 ? d : 0; ns.z += g.axis == 2 ? d : 0;
                ns.w += (int)times;
                ds = ds + (double)g.depth * (double)times;
            }
        }
        q.st.albedo[o] = as;
        q.st.normal[o] = ns;
        q.st.depth[o] = ds;
    }
}

// The state of q.n samples -> the four planes: every division in float64, one rounding to float32
__global__ __launch_bounds__(256) void guide_resolve_kernel(const Resolve q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= q.pixels) return;
    const double n = (double)q.n;
    const int4 ns = q.st.normal[i];
    const uint32_t hits = (uint32_t)ns.w;
    if (q.normal) {
        float *p = q.normal + (size_t)i * 3u;
        p[0] = (float)((double)ns.x / n); p[1] = (float)((double)ns.y / n); p[2] = (float)((double)ns.z / n);
    }
    if (q.albedo) {
        const uint4 as = q.st.albedo[i];
        const double d = 255.0 * n;
        float *p = q.albedo + (size_t)i * 4u;   // a caller's plane: no alignment beyond a float's is assumed
        p[0] = (float)((double)as.x / d); p[1] = (float)((double)as.y / d); p[2] = (float)((double)as.z / d); p[3] = (float)((double)as.w / d);
    }
    if (q.coverage) q.coverage[i] = (float)((double)hits / n);
    if (q.depth) q.depth[i] = hits ? (float)(q.st.depth[i] / (double)hits) : 0.0f;
}

}  // namespace guides
}  // namespace vrt
