// tests/bloom_layout_main.cpp -- TEST INFRASTRUCTURE ONLY: the pyramid's layout (csrc/vrt_bloom.h pyramid(): B0 of include/vrt.h
// vrt_bloom_hdr and the offsets of the levels in the workspace, the text vrt_bloom_workspace_bytes and the launches evaluate) as a
// stand-alone program, for a run under the host sanitizers (tests/test_bloom.py compiles it with -fsanitize=address,undefined and runs
// it; it is never loaded into Python).
// argv[1]: a file of cases, each three int32: width, height, levels. Prints per case "refused", or "ok bytes" followed by
// " w h offset" for each level 1..levels. Where the workspace is at most 64 MiB the program allocates exactly `bytes`, fills every
// level's pixels where the layout puts them, each level with its own number, and reads them back: a level that overlapped another or
// left the block would be seen by the check or by the sanitizer.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vrt_bloom.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int cases = 0;
    int32_t in[3];
    while (std::fread(in, sizeof(int32_t), 3, f) == 3) {
        ++cases;
        vrt::bloom::Pyramid p;
        if (!vrt::bloom::pyramid(in[0], in[1], in[2], p)) {
            std::printf("refused\n");
            continue;
        }
        std::printf("ok %zu", p.bytes);
        for (int l = 1; l <= p.levels; ++l) std::printf(" %d %d %zu", p.w[l], p.h[l], p.offset[l]);
        std::printf("\n");
        if (p.bytes > (64u << 20)) continue;
        std::vector<unsigned char> block(p.bytes, 0);
        for (int l = 1; l <= p.levels; ++l) {
            if (p.offset[l] % vrt::bloom::kLevelAlign != 0) { std::fclose(f); return 5; }
            const size_t n = (size_t)p.w[l] * (size_t)p.h[l] * vrt::bloom::kPixelBytes;
            for (size_t i = 0; i < n; ++i) {
                if (block[p.offset[l] + i] != 0) { std::fclose(f); return 6; }   // another level's
                block[p.offset[l] + i] = (unsigned char)l;
            }
        }
        for (int l = 1; l <= p.levels; ++l) {
            const size_t n = (size_t)p.w[l] * (size_t)p.h[l] * vrt::bloom::kPixelBytes;
            for (size_t i = 0; i < n; ++i)
                if (block[p.offset[l] + i] != (unsigned char)l) { std::fclose(f); return 7; }
        }
    }
    std::fclose(f);
    return cases ? 0 : 4;
}
