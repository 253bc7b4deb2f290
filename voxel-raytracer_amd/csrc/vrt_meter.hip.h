// vrt_meter.hip.h -- light metering on the device (include/vrt.h vrt_meter_hdr, vrt_tonemap_hdr, points E1-E9): the luminance
// histogram of a float image, the finishing step that turns it into the exposure record, and the tone map that reads the record.
//
// histogram_kernel: a capped grid (launch file) with a grid-stride loop over QUADS, four pixels whose 48 bytes are three aligned
// 16-byte words; one lane takes one quad as three 16-byte loads. Where a row of the metered rectangle starts or ends inside a quad,
// the lane loads the pixels that belong to the row one float at a time: the scalar head and tail. Every wave counts into a
// sub-histogram of its own in LDS with integer atomics; at the end the workgroup adds its four and flushes with one global integer
// atomic add per non-zero bin. Integer adds commute: the counts do not depend on the order of arrival. Two forms of the LDS add,
// by the template parameter MERGE: one atomic per lane and pixel (false), or the lanes of a wave that hold the same bin found with
// ballots first and one lane adding their number per distinct bin (true). profiles/meter_ab.txt has both measured; the launch file
// instantiates the one that is kept (kMergeLanes).
// finish_kernel: one workgroup of 256 lanes, one per bin: an inclusive prefix sum in LDS, E4's overlap per bin, E5's sums with LDS
// atomics, and lane 0 writes the record by E6-E8 -- window_of(), overlap() and finish() of vrt_meter.h, the text vrt_meter_resolve
// evaluates on the host. A launch of its own behind the histogram pass: no workgroup waits for another, and the call keeps no counter.
// tonemap_kernel: E9. The record is read once, at an address every lane shares, before the loop; four pixels per lane as three
// 16-byte loads and one 16-byte store where both pointers are aligned (VEC), one pixel per lane otherwise.
// No inline assembly. The resources are in profiles/meter_resource_usage.txt.
#pragma once
#include "vrt_accum.hip.h"   // accum::mom_luminance: E1 is M1's luminance, one definition
#include "vrt_meter.h"

namespace vrt {
namespace meter {

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr uint32_t kMaxBlocks = 512;   // the capped grid of the two streaming passes: two workgroups per CU; one pass of the histogram's covers kMaxBlocks * kBlock * 4 = 524,288 pixels
#ifndef VRT_METER_MERGE
#define VRT_METER_MERGE 0   // the form the library is built with (profiles/meter_ab.txt)
#endif
constexpr bool kMergeLanes = VRT_METER_MERGE != 0;

// E1, E2 of one pixel
VRT_DEV uint32_t pixel_bin(float r, float g, float b) {
    const float c[3] = {r, g, b};
    const uint32_t k = bin_of(accum::mom_luminance(c));
    return k < kBins - 1u ? k : kBins - 1u;   // never binds (E2: the largest Y lands in bin 255); the index stays inside the sub-histogram whatever
}

// one count into the wave's sub-histogram per lane that holds a pixel
template <bool MERGE>
VRT_DEV void count(uint32_t *mine, uint32_t k, bool valid, uint32_t lane) {
    if (!MERGE) {
        if (valid) atomicAdd(&mine[k], 1u);
        return;
    }
    // every lane of the wave is here (the caller's loops are wave-uniform): the first lane still to be counted names a bin, the lanes
    // that hold it drop out together and that lane adds how many they were
    unsigned long long todo = __ballot(valid);
    while (todo != 0ull) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t kl = (uint32_t)__shfl((int)k, leader);
        const unsigned long long same = __ballot(valid && k == kl);
        if ((int)lane == leader) atomicAdd(&mine[kl], (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

template <bool MERGE>
__global__ __launch_bounds__(kBlock) void histogram_kernel(const HistArgs q) {
    __shared__ uint32_t s_hist[kWaves * kBins];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t i = tid; i < kWaves * kBins; i += kBlock) s_hist[i] = 0u;
    __syncthreads();
    uint32_t *mine = s_hist + wave * kBins;
    for (uint32_t row = blockIdx.y; row < q.rows; row += gridDim.y) {
        // the row's pixels [s, e) and its quads [q0, q1], both counted from the aligned origin: pixel p is pp = p + phase there
        const uint32_t sp = q.first + row * q.stride + q.phase, ep = sp + q.len;
        const uint32_t q0 = sp >> 2, q1 = (ep - 1u) >> 2;
        for (uint32_t base = q0 + (blockIdx.x * kWaves + wave) * 64u; base <= q1; base += gridDim.x * kBlock) {   // the same trips in every lane of a wave
            const uint32_t quad = base + lane, pp = quad * 4u;
            uint32_t k[4] = {0u, 0u, 0u, 0u};
            bool valid[4] = {false, false, false, false};
            if (quad <= q1) {
                if (pp >= sp && pp + 4u <= ep) {   // a whole quad: pp >= phase, and the address is a multiple of 16
                    const float4 *v = reinterpret_cast<const float4 *>(q.rgb + (size_t)(pp - q.phase) * 3u);
                    const float4 a = v[0], b = v[1], c = v[2];
                    k[0] = pixel_bin(a.x, a.y, a.z);
                    k[1] = pixel_bin(a.w, b.x, b.y);
                    k[2] = pixel_bin(b.z, b.w, c.x);
                    k[3] = pixel_bin(c.y, c.z, c.w);
                    valid[0] = valid[1] = valid[2] = valid[3] = true;
                } else {   // the row's head or tail: the pixels of the quad that belong to the row
#pragma unroll
                    for (uint32_t j = 0; j < 4u; ++j) {
                        if (pp + j < sp || pp + j >= ep) continue;
                        const float *f = q.rgb + (size_t)(pp + j - q.phase) * 3u;
                        k[j] = pixel_bin(f[0], f[1], f[2]);
                        valid[j] = true;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) count<MERGE>(mine, k[j], valid[j], lane);
        }
    }
    __syncthreads();
    // kBlock == kBins: a lane per bin
    uint32_t total = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += s_hist[w * kBins + tid];
    if (total != 0u) atomicAdd(&q.histogram[tid], total);
}
static_assert(kBlock == (int)kBins, "the flush and the finishing step give every bin a lane");

__global__ __launch_bounds__(kBlock) void finish_kernel(const FinishArgs q) {
    __shared__ uint32_t s_cum[kBins];             // N <= 2^30: a prefix sum fits 32 bits
    __shared__ unsigned long long s_sum[2];       // M, S
    const uint32_t k = threadIdx.x;
    const uint32_t own = q.histogram[k];
    s_cum[k] = own;
    if (k < 2u) s_sum[k] = 0ull;
    __syncthreads();
    for (uint32_t d = 1u; d < kBins; d <<= 1) {   // inclusive, Hillis-Steele
        const uint32_t add = k >= d ? s_cum[k - d] : 0u;
        __syncthreads();
        s_cum[k] += add;
        __syncthreads();
    }
    const uint64_t cum = s_cum[k], n = s_cum[kBins - 1u];
    const uint64_t nk = k == 0u ? 0u : overlap(cum - own, cum, window_of(n, q.m));   // E5: black enters no sum
    if (nk != 0u) {
        atomicAdd(&s_sum[0], (unsigned long long)nk);
        atomicAdd(&s_sum[1], (unsigned long long)(nk * k));
    }
    __syncthreads();
    if (k == 0u) {
        vrt_exposure io = *q.record;
        finish(s_sum[0], s_sum[1], q.m, io);
        *q.record = io;
    }
}

// E9's exposure: the record's with the caller's
VRT_DEV float tone_exposure(const ToneArgs &q) {
    if (!q.record) return q.exposure;
    return min_c(q.exposure * q.record->exposure, 3.402823466e38f);
}
VRT_DEV uint32_t tone_pixel(float r, float g, float b, int op, float e) {
    return unorm8(accum::tone_map(r, op, e)) | (unorm8(accum::tone_map(g, op, e)) << 8) | (unorm8(accum::tone_map(b, op, e)) << 16) | (255u << 24);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void tonemap_kernel(const ToneArgs q) {
    const float e = tone_exposure(q);   // one address for every lane: read once per wave
    const size_t step = (size_t)gridDim.x * kBlock, first = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (VEC) {
        const size_t quads = q.n >> 2;
        for (size_t i = first; i < quads; i += step) {
            const float4 *v = reinterpret_cast<const float4 *>(q.rgb) + i * 3u;
            const float4 a = v[0], b = v[1], c = v[2];
            reinterpret_cast<uint4 *>(q.out_rgba)[i] = make_uint4(tone_pixel(a.x, a.y, a.z, q.op, e), tone_pixel(a.w, b.x, b.y, q.op, e),
                                                                  tone_pixel(b.z, b.w, c.x, q.op, e), tone_pixel(c.y, c.z, c.w, q.op, e));
        }
        const size_t p = quads * 4u + first;   // the tail: at most three pixels
        if (p < q.n) q.out_rgba[p] = tone_pixel(q.rgb[p * 3u], q.rgb[p * 3u + 1u], q.rgb[p * 3u + 2u], q.op, e);
    } else {
        for (size_t p = first; p < q.n; p += step) q.out_rgba[p] = tone_pixel(q.rgb[p * 3u], q.rgb[p * 3u + 1u], q.rgb[p * 3u + 2u], q.op, e);
    }
}

}  // namespace meter
}  // namespace vrt
