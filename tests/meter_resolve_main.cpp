// tests/meter_resolve_main.cpp -- TEST INFRASTRUCTURE ONLY: the metering rule (csrc/vrt_meter.h resolve(): E4-E8 of include/vrt.h
// vrt_meter_hdr, the text the finishing kernel and vrt_meter_resolve evaluate) as a stand-alone program, for a run under the host
// sanitizers (tests/test_meter.py compiles it with -fsanitize=address,undefined and runs it; it is never loaded into Python).
// argv[1]: a file of cases, each VRT_METER_BINS uint32 counts, a vrt_meter and a vrt_exposure, in that order with no padding.
// Prints per case "ok exposure-bits metered-bits window frames", or "refused" where the counts sum to more than 2^30.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vrt_meter.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint32_t> hist(VRT_METER_BINS);
    int cases = 0;
    for (;;) {
        vrt_meter m;
        vrt_exposure io;
        if (std::fread(hist.data(), sizeof(uint32_t), hist.size(), f) != hist.size()) break;
        if (std::fread(&m, sizeof m, 1, f) != 1 || std::fread(&io, sizeof io, 1, f) != 1) { std::fclose(f); return 3; }
        if (!vrt::meter::resolve(hist.data(), m, io)) {
            std::printf("refused\n");
        } else {
            uint32_t e, y;
            std::memcpy(&e, &io.exposure, 4);
            std::memcpy(&y, &io.metered, 4);
            std::printf("ok %u %u %u %u\n", e, y, io.window, io.frames);
        }
        ++cases;
    }
    std::fclose(f);
    return cases ? 0 : 4;
}
