// tests/emit_cdf_main.cpp -- TEST INFRASTRUCTURE ONLY: the host's table code (csrc/vrt_emitters.h emitter_walk(), emitter_weights(),
// emitter_cdf()) as a stand-alone program, for a run under the host sanitizers (tests/test_emit_power.py compiles it with
// -fsanitize=address,undefined and runs it; it is never loaded into Python). Cases: a list of 2^20 leaves of size 1024 whose weights
// sum into the 2^57 range -- every fourth one black -- and a small tree walked from its records. Prints, per case, N, the total
// weight, a few thresholds and an FNV-1a hash of the whole table; exits non-zero where the table is not strictly increasing or does
// not end at 2^24.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vrt_emitters.h"

static int report(const char *name, const std::vector<uint64_t> &weights, const std::vector<uint32_t> &cdf) {
    unsigned long long total = 0;
    for (uint64_t w : weights) total += w;
    uint64_t h = 1469598103934665603ull;
    uint32_t before = 0;
    for (size_t j = 0; j < cdf.size(); ++j) {
        if (cdf[j] <= before) { std::printf("%s: not increasing at %zu\n", name, j); return 1; }
        before = cdf[j];
        for (int b = 0; b < 4; ++b) { h ^= (cdf[j] >> (8 * b)) & 0xffu; h *= 1099511628211ull; }
    }
    if (cdf.empty() || cdf.back() != (1u << 24)) { std::printf("%s: the last threshold is not 2^24\n", name); return 1; }
    std::printf("%s %zu %llu %u %u %u %llu\n", name, cdf.size(), total, cdf[0], cdf[cdf.size() / 2], cdf[cdf.size() - 1], (unsigned long long)h);
    return 0;
}

int main() {
    int bad = 0;
    {   // 2^20 leaves of size 1024: W_j = 2^20 * 255 * 765 (every fourth one: 0), the sum in the 2^57 range
        const size_t n = (size_t)1 << 20;
        std::vector<int32_t> list(4 * n);
        std::vector<uint32_t> words(2 * n);
        for (size_t j = 0; j < n; ++j) {
            list[4 * j] = (int32_t)j; list[4 * j + 1] = 0; list[4 * j + 2] = 0; list[4 * j + 3] = 1024;
            words[2 * j] = j % 4 == 3 ? 0xff000000u : 0xffffffffu;
            words[2 * j + 1] = 0x0000ffffu;
        }
        std::vector<uint64_t> weights;
        std::vector<uint32_t> cdf;
        emitter_weights(list, words, weights);
        emitter_cdf(weights, cdf);
        bad |= report("big", weights, cdf);
        for (auto &w : words) w &= 0xff000000u;   // all black, no illumination: the equal split
        emitter_weights(list, words, weights);
        emitter_cdf(weights, cdf);
        bad |= report("black", weights, cdf);
    }
    {   // a tree of one internal root with three leaf children, two of them emitters, under bounds 0 .. 2
        std::vector<vrt::Record> recs(4);
        recs[0] = vrt::Record{0x00000007u | (0x07u << 8), 1u};
        recs[1] = vrt::Record{0xff102030u, 0x000020ffu};
        recs[2] = vrt::Record{0xffffffffu, 0x000000ffu};   // no illumination: not an emitter
        recs[3] = vrt::Record{0xff0000ffu, 0x0000ffffu};
        const int mn[3] = {0, 0, 0}, mx[3] = {2, 2, 2};
        std::vector<int32_t> list;
        std::vector<uint32_t> words, cdf;
        std::vector<uint64_t> weights;
        const uint64_t n = emitter_walk(recs, mn, mx, 1u << 20, list, &words);
        if (n != 2 || list.size() != 8 || words.size() != 4) { std::printf("walk: %llu entries\n", (unsigned long long)n); return 1; }
        emitter_weights(list, words, weights);
        emitter_cdf(weights, cdf);
        bad |= report("walk", weights, cdf);
        std::vector<int32_t> plain;
        if (emitter_list(recs, mn, mx, 1u << 20, plain) != n || plain != list) { std::printf("emitter_list differs from the walk\n"); return 1; }
        if (emitter_walk(recs, mn, mx, 1, list, &words) != 2 || !list.empty() || !words.empty()) { std::printf("above max_entries something was kept\n"); return 1; }
    }
    return bad;
}
