// vrt_meter.h -- light metering (include/vrt.h vrt_meter_hdr, points E1-E9): the rule that turns a luminance histogram into an
// exposure record, as host/device inline functions, and the arguments of the three kernels (vrt_meter.hip.h). One text of E2 and
// E4-E8 serves the finishing step on the device, vrt_meter_resolve on the host and tests/meter_resolve_main.cpp, which compiles this
// header alone under the host sanitizers: it needs include/vrt.h and the C headers below, nothing of HIP. Every translation unit that
// includes it is compiled without contraction; E7 and E8 are float32, one rounding per operation; everything else is integers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vrt.h"

#if defined(__HIPCC__)
#define VRT_METER_FN __host__ __device__ inline
#else
#define VRT_METER_FN inline
#endif

namespace vrt {
namespace meter {

constexpr uint32_t kBins = VRT_METER_BINS;
constexpr uint32_t kBinBase = 888u;           // (exponent field of 2^-16 = 111) * 8: E2 counts eighths of an octave from 2^-16
constexpr uint64_t kMaxPixels = 1ull << 30;   // the frame-size rule's bound on N (E3): no count wraps, S << 20 stays below 2^58

VRT_METER_FN uint32_t float_bits(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}
VRT_METER_FN float float_from_bits(uint32_t b) {
    float v;
    memcpy(&v, &b, 4);
    return v;
}
// min and max in the conventions of the unorm8 store (include/vrt.h vrt_accum_keep_hdr point 1)
VRT_METER_FN float min_c(float a, float b) { return b < a ? b : a; }
VRT_METER_FN float max_c(float a, float b) { return a < b ? b : a; }

// E2: the bin of a luminance Y that is finite, >= +0 and below 2^16
VRT_METER_FN uint32_t bin_of(float y) {
    const int k = (int)(float_bits(y) >> 20) - (int)kBinBase;
    return (uint32_t)(k < 0 ? 0 : k);
}

// E4: the rank window [a, b) of N pixels
struct Window { uint64_t a, b; };
VRT_METER_FN Window window_of(uint64_t n, const vrt_meter &m) {
    return Window{n * (uint64_t)m.low_permille / 1000u, n * (uint64_t)m.high_permille / 1000u};
}
// ... and n_k: how many of the ranks [cum_before, cum) of bin k lie in it
VRT_METER_FN uint64_t overlap(uint64_t cum_before, uint64_t cum, const Window &w) {
    const uint64_t lo = cum_before > w.a ? cum_before : w.a, hi = cum < w.b ? cum : w.b;
    return hi > lo ? hi - lo : 0u;
}

// E6-E8: the sums M and S of E5 -> the record. m: checked (vrt_meter.cpp check_params)
VRT_METER_FN void finish(uint64_t big_m, uint64_t big_s, const vrt_meter &m, vrt_exposure &io) {
    float metered = 0.0f, target;
    if (big_m != 0u) {
        const uint64_t t = (big_s << 20) / big_m;                                   // E6: the mean pseudo-logarithm, 20 fraction bits
        metered = float_from_bits((kBinBase << 20) + (uint32_t)t + (1u << 19));     // ... at the bins' centres
        target = min_c(max_c(m.key / metered, m.min_exposure), m.max_exposure);     // E7
    } else {
        target = io.frames > 0u ? io.exposure : min_c(max_c(1.0f, m.min_exposure), m.max_exposure);
    }
    float e = target;                                                               // E8
    if (!(m.adapt == 1.0f || io.frames == 0u || big_m == 0u)) {
        const float prev = io.exposure;
        e = prev + m.adapt * (target - prev);
    }
    io.exposure = e;
    io.metered = metered;
    io.window = (uint32_t)big_m;
    io.frames = io.frames == 0xffffffffu ? io.frames : io.frames + 1u;
}

// E3-E8 over a whole histogram, one bin after the other (the host's form; the device's finishing step takes the same window_of,
// overlap and finish with the prefix sum spread over a workgroup). false: the counts sum to more than kMaxPixels.
VRT_METER_FN bool resolve(const uint32_t *histogram, const vrt_meter &m, vrt_exposure &io) {
    uint64_t n = 0;
    for (uint32_t k = 0; k < kBins; ++k) n += histogram[k];
    if (n > kMaxPixels) return false;
    const Window w = window_of(n, m);
    uint64_t cum = 0, big_m = 0, big_s = 0;
    for (uint32_t k = 0; k < kBins; ++k) {
        const uint64_t before = cum;
        cum += histogram[k];
        if (k == 0u) continue;   // E5: black occupies ranks and enters no sum
        const uint64_t nk = overlap(before, cum, w);
        big_m += nk;
        big_s += nk * k;
    }
    finish(big_m, big_s, m, io);
    return true;
}

// ---- the kernels' arguments ----

// The histogram pass over the rectangle's rows: row r is the `len` pixels from pixel first + r * stride of the image. A rectangle as
// wide as the frame is ONE row of all its pixels (the host folds it).
struct HistArgs {
    const float *rgb;      // 3 floats per pixel, 4-byte aligned
    uint32_t *histogram;   // kBins counts, zeroed before the launch
    uint32_t first, stride, len, rows;   // in pixels; first + (rows - 1) * stride + len <= 2^30
    uint32_t phase;        // pixel p starts a 16-byte word of rgb exactly when (p + phase) % 4 == 0
};

// The finishing step: histogram -> *record
struct FinishArgs {
    const uint32_t *histogram;
    vrt_exposure *record;
    vrt_meter m;
};

// The tone-map pass (E9): n pixels of 3 floats -> n rgba8 words. record may be null.
struct ToneArgs {
    const float *rgb;
    const vrt_exposure *record;
    uint32_t *out_rgba;
    size_t n;
    int op;           // VRT_TONEMAP_*
    float exposure;   // tm->exposure
};

}  // namespace meter
}  // namespace vrt
