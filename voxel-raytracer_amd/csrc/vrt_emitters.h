// vrt_emitters.h -- the emitter list of a tree (include/vrt.h vrt_set_emitter_sampling, "The emitter list"), made by the host from the
// record array and the world bounds, and the table of thresholds by which VRT_EMIT_POWER picks from it (vrt_set_emitter_importance,
// "Weights"): a header of its own, plain C++, so that the test library (test/vrt_test.hip vrt_test_emitter_list,
// vrt_test_emitter_cdf) runs the product's functions on a caller's records.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "vrt_layout.h"

// Every leaf with alpha byte > 0 and illumination byte > 0, as {lo.x, lo.y, lo.z, size}: its box under the world bounds, split as the
// shader splits (mid = min + (max - min) / 2, child bit 2 - k the upper half of axis k), ascending by (lo.x, lo.y, lo.z). A leaf whose
// box is no cube -- only a merged volume in a world whose bounds are no power of two -- is listed as its unit cells; a box that holds
// no cell is not listed. Returns N. Above max_entries nothing is kept (`out` comes back empty): the count alone is the answer. A
// malformed array (a child index past the end, deeper than 32 levels) ends the walk of that branch.
// emitter_walk() is the walk itself: with `words` it also hands out each entry's record words (w0, w1), two per entry in the list's
// order -- a unit cell of a non-cube leaf takes that leaf's record.
inline uint64_t emitter_walk(const std::vector<vrt::Record> &records, const int wmin[3], const int wmax[3], uint64_t max_entries,
                             std::vector<int32_t> &out, std::vector<uint32_t> *words) {
    out.clear();
    if (words) words->clear();
    if (records.empty()) return 0;
    struct Item { uint32_t rec; int mn[3], mx[3]; int depth; };
    struct Found { int32_t e[4]; uint32_t rec; };
    std::vector<Item> todo;
    std::vector<Found> found;
    uint64_t n = 0;
    Item root{0u, {wmin[0], wmin[1], wmin[2]}, {wmax[0], wmax[1], wmax[2]}, 0};
    todo.push_back(root);
    while (!todo.empty()) {
        const Item it = todo.back();
        todo.pop_back();
        const uint32_t mask = records[it.rec].w0 & 0xffu, leaf_mask = (records[it.rec].w0 >> 8) & 0xffu;
        uint32_t child = records[it.rec].w1;
        for (uint32_t ci = 0; ci < 8; ++ci) {
            if (!((mask >> ci) & 1u)) continue;
            const uint32_t idx = child++;
            if ((size_t)idx >= records.size()) break;
            Item cb{idx, {0, 0, 0}, {0, 0, 0}, it.depth + 1};
            for (int k = 0; k < 3; ++k) {
                const int mid = it.mn[k] + ((it.mx[k] - it.mn[k]) >> 1);
                const bool hi = (ci >> (2 - k)) & 1u;
                cb.mn[k] = hi ? mid : it.mn[k];
                cb.mx[k] = hi ? it.mx[k] : mid;
            }
            if (!((leaf_mask >> ci) & 1u)) {
                if (cb.depth < 32) todo.push_back(cb);
                continue;
            }
            if ((records[idx].w0 >> 24) == 0u || ((records[idx].w1 >> 8) & 0xffu) == 0u) continue;
            const int64_t dx = (int64_t)cb.mx[0] - cb.mn[0], dy = (int64_t)cb.mx[1] - cb.mn[1], dz = (int64_t)cb.mx[2] - cb.mn[2];
            if (dx <= 0 || dy <= 0 || dz <= 0) continue;
            if (dx == dy && dy == dz) {
                if (++n <= max_entries) found.push_back({{cb.mn[0], cb.mn[1], cb.mn[2], (int32_t)dx}, idx});
                continue;
            }
            const uint64_t cells = (uint64_t)dx * (uint64_t)dy * (uint64_t)dz;
            if (n + cells <= max_entries)
                for (int x = cb.mn[0]; x < cb.mx[0]; ++x)
                    for (int y = cb.mn[1]; y < cb.mx[1]; ++y)
                        for (int z = cb.mn[2]; z < cb.mx[2]; ++z) found.push_back({{x, y, z, 1}, idx});
            n += cells;
        }
    }
    if (n > max_entries) return n;
    std::sort(found.begin(), found.end(), [](const Found &p, const Found &q) {
        return p.e[0] != q.e[0] ? p.e[0] < q.e[0] : (p.e[1] != q.e[1] ? p.e[1] < q.e[1] : p.e[2] < q.e[2]);
    });
    out.reserve(found.size() * 4);
    if (words) words->reserve(found.size() * 2);
    for (const Found &f : found) {
        out.insert(out.end(), f.e, f.e + 4);
        if (words) {
            words->push_back(records[f.rec].w0);
            words->push_back(records[f.rec].w1);
        }
    }
    return n;
}

inline uint64_t emitter_list(const std::vector<vrt::Record> &records, const int wmin[3], const int wmax[3], uint64_t max_entries,
                             std::vector<int32_t> &out) {
    return emitter_walk(records, wmin, wmax, max_entries, out, nullptr);
}

// The power of entry j of a list (four int32 each) with the record words emitter_walk() handed out (two each), an integer:
// W_j = size^2 * illum * (R + G + B), illum = (w1 >> 8) & 0xff, R, G, B the low three bytes of w0, as decode_leaf reads them. At most
// 2^22 * 255 * 765 < 2^40, so that the sum over VRT_MAX_EMITTERS entries stays below 2^60.
inline void emitter_weights(const std::vector<int32_t> &list, const std::vector<uint32_t> &words, std::vector<uint64_t> &weights) {
    const size_t n = list.size() / 4;
    weights.resize(n);
    for (size_t j = 0; j < n; ++j) {
        const uint32_t w0 = words[2 * j], w1 = words[2 * j + 1];
        const uint64_t size = (uint64_t)(uint32_t)list[4 * j + 3];
        weights[j] = size * size * (uint64_t)((w1 >> 8) & 0xffu) * (uint64_t)((w0 & 0xffu) + ((w0 >> 8) & 0xffu) + ((w0 >> 16) & 0xffu));
    }
}

// The thresholds of VRT_EMIT_POWER (include/vrt.h vrt_set_emitter_importance, "Weights"), in exact integers: with C_j the inclusive
// prefix sum of the N weights and Wtot = C_{N-1},
//   Wtot > 0:  T_j = (j + 1) + floor(C_j * (2^24 - N) / Wtot)       Wtot == 0:  T_j = floor((j + 1) * 2^24 / N)
// so that T is strictly increasing, every emitter holds at least one of the 2^24 ticks and T_{N-1} = 2^24. N is at most 2^20
// (VRT_MAX_EMITTERS) and Wtot below 2^63: the product passes 64 bits.
// With `wtot` it also hands out Wtot, which vrt_set_emitter_mis turns into the launch's inv_power (emitter_inv_power()).
inline void emitter_cdf(const std::vector<uint64_t> &weights, std::vector<uint32_t> &out, uint64_t *wtot = nullptr) {
    const uint64_t n = weights.size();
    out.resize(n);
    uint64_t total = 0;
    for (uint64_t w : weights) total += w;
    if (wtot) *wtot = total;
    uint64_t c = 0;
    for (uint64_t j = 0; j < n; ++j) {
        c += weights[j];
        if (total > 0) out[j] = (uint32_t)((j + 1) + (uint64_t)((unsigned __int128)c * ((1u << 24) - n) / total));
        else out[j] = (uint32_t)(((j + 1) << 24) / n);
    }
}

// inv_power of include/vrt.h vrt_set_emitter_mis, "Per launch": 1 / Wtot in float32, rounded once from the float64 quotient; 0 for a
// list without power.
inline float emitter_inv_power(uint64_t wtot) { return wtot > 0 ? (float)(1.0 / (double)wtot) : 0.0f; }
