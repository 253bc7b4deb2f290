// vrt_emitters.cpp -- emitter sampling's host side (include/vrt.h vrt_set_emitter_sampling, vrt_set_emitter_importance,
// vrt_set_emitter_mis): the flag, the mode, the MIS flag, and the context's emitter list with its table of thresholds and their Wtot.
// The list is a function of the tree and the world bounds (vrt_emitters.h emitter_list()); it is made lazily -- by vrt_emitters, and by
// the first VRT_MODE_FULL add or ray batch with sampling on -- and made again when vrt_ctx::tree_gen (uploads, patches, batch ends,
// compactions) or the bounds (vrt_set_params) have moved since. No device code.
#include "vrt_internal.h"

#include <cstring>

namespace vrt_internal {

int ensure_emitters(vrt_ctx *c, const char *what, bool sampling) {
    if (!c->have_scene) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": no octree uploaded (call vrt_upload_octree first)");
    if (c->batch.open) return vrt_fail(c, VRT_E_STATE, std::string(what) + ": a patch batch is open (call vrt_patch_end first)");
    vrt_ctx::Emitters &em = c->emitters;
    const bool same = em.built && em.tree_gen == c->tree_gen && std::memcmp(em.wmin, c->params.world_min, sizeof em.wmin) == 0 &&
                      std::memcmp(em.wmax, c->params.world_max, sizeof em.wmax) == 0;
    if (!same) {
        em.built = false;
        std::vector<uint32_t> words;
        std::vector<uint64_t> weights;
        em.n = emitter_walk(c->host_records, c->params.world_min, c->params.world_max, VRT_MAX_EMITTERS, em.list, &words);
        emitter_weights(em.list, words, weights);
        emitter_cdf(weights, em.cdf, &em.wtot);
        if (!em.list.empty()) {
            VRT_HIP(c, hipSetDevice(c->device));
            // launches of any stream (ray batches take the caller's) may still read the list
            VRT_HIP(c, hipDeviceSynchronize());
            VRT_HIP(c, em.d_list.reserve(em.list.size() * sizeof(int32_t)));
            VRT_HIP(c, hipMemcpy(em.d_list, em.list.data(), em.list.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            VRT_HIP(c, em.d_cdf.reserve(em.cdf.size() * sizeof(uint32_t)));
            VRT_HIP(c, hipMemcpy(em.d_cdf, em.cdf.data(), em.cdf.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        em.tree_gen = c->tree_gen;
        std::memcpy(em.wmin, c->params.world_min, sizeof em.wmin);
        std::memcpy(em.wmax, c->params.world_max, sizeof em.wmax);
        em.built = true;
    }
    if (sampling && em.n > VRT_MAX_EMITTERS)
        return vrt_fail(c, VRT_E_STATE, std::string(what) + ": emitter sampling is on and the tree has more than VRT_MAX_EMITTERS emitters");
    return VRT_OK;
}

}  // namespace vrt_internal

extern "C" {

int vrt_set_emitter_sampling(vrt_ctx *c, int enable) {
    if (!c) return VRT_E_INVALID;
    if (enable != 0 && enable != 1) return vrt_fail(c, VRT_E_INVALID, "vrt_set_emitter_sampling: enable must be 0 or 1");
    c->emitter_sampling = enable != 0;
    return VRT_OK;
}

int vrt_set_emitter_importance(vrt_ctx *c, int mode) {
    if (!c) return VRT_E_INVALID;
    if (mode != VRT_EMIT_UNIFORM && mode != VRT_EMIT_POWER)
        return vrt_fail(c, VRT_E_INVALID, "vrt_set_emitter_importance: mode must be VRT_EMIT_UNIFORM or VRT_EMIT_POWER");
    c->emitter_importance = mode;
    return VRT_OK;
}

int vrt_set_emitter_mis(vrt_ctx *c, int enable) {
    if (!c) return VRT_E_INVALID;
    if (enable != 0 && enable != 1) return vrt_fail(c, VRT_E_INVALID, "vrt_set_emitter_mis: enable must be 0 or 1");
    c->emitter_mis = enable != 0;
    return VRT_OK;
}

long vrt_emitter_cdf(vrt_ctx *c, uint32_t *out, size_t cap) {
    if (!c) return VRT_E_INVALID;
    if (cap && !out) return vrt_fail(c, VRT_E_INVALID, "vrt_emitter_cdf: out is NULL");
    const int r = vrt_internal::ensure_emitters(c, "vrt_emitter_cdf", false);
    if (r) return r;
    const vrt_ctx::Emitters &em = c->emitters;
    const size_t held = em.cdf.size();   // none above VRT_MAX_EMITTERS
    const size_t take = held < cap ? held : cap;
    if (take) std::memcpy(out, em.cdf.data(), take * sizeof(uint32_t));
    return (long)em.n;
}

long vrt_emitters(vrt_ctx *c, int32_t *out, size_t cap) {
    if (!c) return VRT_E_INVALID;
    if (cap && !out) return vrt_fail(c, VRT_E_INVALID, "vrt_emitters: out is NULL");
    const int r = vrt_internal::ensure_emitters(c, "vrt_emitters", false);
    if (r) return r;
    const vrt_ctx::Emitters &em = c->emitters;
    const size_t held = em.list.size() / 4;   // none above VRT_MAX_EMITTERS
    const size_t take = held < cap ? held : cap;
    if (take) std::memcpy(out, em.list.data(), take * 4 * sizeof(int32_t));
    return (long)em.n;
}

}  // extern "C"
