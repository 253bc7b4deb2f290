// vrt_emitters.h -- the emitter list of a tree (include/vrt.h vrt_set_emitter_sampling, "The emitter list"), made by the host from the
// record array and the world bounds: a header of its own, plain C++, so that the test library (test/vrt_test.hip
// vrt_test_emitter_list) runs the product's function on a caller's records.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <vector>

#include "vrt_layout.h"

// Every leaf with alpha byte > 0 and illumination byte > 0, as {lo.x, lo.y, lo.z, size}: its box under the world bounds, split as the
// shader splits (mid = min + (max - min) / 2, child bit 2 - k the upper half of axis k), ascending by (lo.x, lo.y, lo.z). A leaf whose
// box is no cube -- only a merged volume in a world whose bounds are no power of two -- is listed as its unit cells; a box that holds
// no cell is not listed. Returns N. Above max_entries nothing is kept (`out` comes back empty): the count alone is the answer. A
// malformed array (a child index past the end, deeper than 32 levels) ends the walk of that branch.
inline uint64_t emitter_list(const std::vector<vrt::Record> &records, const int wmin[3], const int wmax[3], uint64_t max_entries,
                             std::vector<int32_t> &out) {
    out.clear();
    if (records.empty()) return 0;
    struct Item { uint32_t rec; int mn[3], mx[3]; int depth; };
    std::vector<Item> todo;
    std::vector<std::array<int32_t, 4>> found;
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
                if (++n <= max_entries) found.push_back({cb.mn[0], cb.mn[1], cb.mn[2], (int32_t)dx});
                continue;
            }
            const uint64_t cells = (uint64_t)dx * (uint64_t)dy * (uint64_t)dz;
            if (n + cells <= max_entries)
                for (int x = cb.mn[0]; x < cb.mx[0]; ++x)
                    for (int y = cb.mn[1]; y < cb.mx[1]; ++y)
                        for (int z = cb.mn[2]; z < cb.mx[2]; ++z) found.push_back({x, y, z, 1});
            n += cells;
        }
    }
    if (n > max_entries) return n;
    std::sort(found.begin(), found.end(), [](const std::array<int32_t, 4> &p, const std::array<int32_t, 4> &q) {
        return p[0] != q[0] ? p[0] < q[0] : (p[1] != q[1] ? p[1] < q[1] : p[2] < q[2]);
    });
    out.reserve(found.size() * 4);
    for (const auto &e : found) out.insert(out.end(), e.begin(), e.end());
    return n;
}
