// vrt_test.hip -- TEST SUPPORT, not product: libvrt_hip_test.so. What the parity suite needs to look INSIDE the dispatch layer
// without the product library exporting hooks for it:
//   * device probes of the arithmetic the kernels rely on (correctly rounded / and sqrt, no contraction, the in-range 1/x, sqrt and
//     x/PI forms, the polynomial exp / sin / cos / pow conventions): the same inline functions the kernels call, compiled from the
//     same headers with the same flags;
//   * host-only views of the layouts the uploader builds (record array, wide cells), of the edit patches, of the per-projection
//     ray tables and of the dispatcher's "world is empty outside wide root 0" analysis: the same sources (vrt_layout.cpp,
//     vrt_raygen.cpp) linked a second time.
//   * the adaptive accumulation's stopping rule (vrt_accum.h adaptive_active), on the host and on the device.
//   * the guided filter's launch geometry (vrt_filter.hip.h): the tile constants the coverage model of tests/filter_geometry.py needs.
// libvrt_hip.so exports none of this (tests/test_abi.py checks that).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/vrt.h"
#include "../vrt_common.hip.h"
#include "../vrt_accum.h"
#include "../vrt_full.hip.h"
#include "../vrt_kernels_v4.hip.h"
#include "../vrt_layout.h"
#include "../vrt_miss.h"
#include "../vrt_sched.hip.h"
#include "../vrt_sun.h"
#include "../vrt_emitters.h"
#include "../vrt_filter.hip.h"

namespace vrt {
// the adaptive stopping rule on the device: out[i] = adaptive_active(n[i], s[i], q[i], min, max, tol)
__global__ void adaptive_probe_kernel(const uint32_t *n, const uint64_t *s, const uint64_t *q, uint32_t min, uint32_t max,
                                      uint32_t tol, uint32_t *out, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[i] = accum::adaptive_active(n[i], s[i], q[i], min, max, tol) ? 1u : 0u;
}

// exactness probe for the arithmetic contract: out[i] = op(x[i], y[i])
__global__ void math_probe_kernel(int op, const float *x, const float *y, float *out, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a = x[i], b = y[i], r = 0.0f;
    switch (op) {
        case 0: r = a / b; break;
        case 1: r = __builtin_sqrtf(a); break;
        case 2: r = 1.0f / __builtin_sqrtf(a); break;
        case 3: r = __builtin_floorf(a); break;
        case 4: r = __builtin_rintf(a); break;
        case 5: r = a * b + 1.0f; break;          // must NOT be fused
        case 6: r = det_expf(a); break;
        case 7: r = (float)(int)a; break;
        case 8: r = a + b; break;
        case 9: r = a * b; break;
        case 30: r = rcp_inrange(a); break;
        case 31: r = sqrt_inrange(a); break;
        case 32: r = div_pi_inrange(a); break;
        default: break;
    }
    out[i] = r;
}

namespace full {
// exactness probe for the conventions above (ops 10..): out[i] = op(x[i], y[i])
__global__ void math_probe_full_kernel(int op, const float *x, const float *y, float *out, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a = x[i], b = y[i], r = 0.0f, s, c;
    switch (op) {
        case 10: det_sincos(a, s, c); r = s; break;
        case 11: det_sincos(a, s, c); r = c; break;
        case 12: r = det_powf(a, b); break;
        case 13: { int q; asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(q) : "v"(a)); r = (float)q; } break;
        case 14: r = (float)__float_as_uint(a) / 4294967296.0f; break;  // rand(): uint -> float, RNE
        case 15: r = unorm_of(a); break;                                // must equal a / 255.0f for the 256 byte values
        default: break;
    }
    out[i] = r;
}

}  // namespace full

// The march step of v4 (dda_step + axis_of, the node planes of find()) against the arithmetic it replaced, written out in
// plain C: the position after the step, its floor as integers, the exit axis and the planes of a node of side 2^t there.
// in: 16 words per case = rp[3], plane[3], dir[3], inv[3], push[3] (floats), t (uint); dpos[3] (ints) separately.
// out: 20 words per case = the step's rp[3], mp[3], axis, planes[3]; then the same from the old arithmetic.
__global__ void march_step_probe_kernel(const float *in, const int *dpos, uint32_t *out, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *q = in + 16 * i;
    const F3 plane{q[3], q[4], q[5]}, dir{q[6], q[7], q[8]}, inv{q[9], q[10], q[11]}, push{q[12], q[13], q[14]};
    const uint32_t t = __float_as_uint(q[15]);
    const I3 dp{dpos[3 * i], dpos[3 * i + 1], dpos[3 * i + 2]};
    uint32_t *o = out + 20 * i;
    {   // the kernel's step
        F3 rp{q[0], q[1], q[2]};
        I3 mp;
        const v4::Trav::Step st = v4::Trav::dda_step(rp, mp, dir, inv, push, plane);
        const F3 pl = v4::Trav::planes(mp, dp, t);
        o[0] = __float_as_uint(rp.x); o[1] = __float_as_uint(rp.y); o[2] = __float_as_uint(rp.z);
        o[3] = (uint32_t)mp.x; o[4] = (uint32_t)mp.y; o[5] = (uint32_t)mp.z;
        o[6] = (uint32_t)v4::Trav::axis_of(st);
        o[7] = __float_as_uint(pl.x); o[8] = __float_as_uint(pl.y); o[9] = __float_as_uint(pl.z);
    }
    {   // the arithmetic it replaced: selects, two floors, float planes
        F3 rp{q[0], q[1], q[2]};
        const float tx = (plane.x - rp.x) * inv.x, ty = (plane.y - rp.y) * inv.y, tz = (plane.z - rp.z) * inv.z;
        const bool ax = tx < (ty < tz ? ty : tz), ayz = ty < tz;
        const float ts = ax ? tx : (ayz ? ty : tz);
        rp.x = rp.x + dir.x * ts; rp.y = rp.y + dir.y * ts; rp.z = rp.z + dir.z * ts;
        const int axis = ax ? 0 : (ayz ? 1 : 2);
        if (axis == 0) rp.x = push.x + rp.x;
        if (axis == 1) rp.y = push.y + rp.y;
        if (axis == 2) rp.z = push.z + rp.z;
        const F3 pf{__builtin_floorf(rp.x), __builtin_floorf(rp.y), __builtin_floorf(rp.z)};
        const float side = __uint_as_float((127u + t) << 23), inv_side = __uint_as_float((127u - t) << 23);
        const F3 dposf{dp.x ? 1.0f : 0.0f, dp.y ? 1.0f : 0.0f, dp.z ? 1.0f : 0.0f};
        o[10] = __float_as_uint(rp.x); o[11] = __float_as_uint(rp.y); o[12] = __float_as_uint(rp.z);
        o[13] = (uint32_t)(int)pf.x; o[14] = (uint32_t)(int)pf.y; o[15] = (uint32_t)(int)pf.z;
        o[16] = (uint32_t)axis;
        o[17] = __float_as_uint((__builtin_floorf(pf.x * inv_side) + dposf.x) * side);
        o[18] = __float_as_uint((__builtin_floorf(pf.y * inv_side) + dposf.y) * side);
        o[19] = __float_as_uint((__builtin_floorf(pf.z * inv_side) + dposf.z) * side);
    }
}

// the selection of VRT_EMIT_POWER on the device: the kernels' own emit_pick() (vrt_common.hip.h) on a caller's table, with the rule's
// conversion of the draw: out[2 * i] = j, out[2 * i + 1] = ticks for u0[i]
__global__ void emit_pick_probe_kernel(const uint32_t *cdf, uint32_t n, const float *u0, uint32_t *out, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t t = (uint32_t)(u0[i] * 16777216.0f);
    t = t < 16777215u ? t : 16777215u;
    uint32_t ticks;
    out[2 * i] = emit_pick(cdf, n, t, ticks);
    out[2 * i + 1] = ticks;
}

// the densities of vrt_set_emitter_mis on the device: the kernels' own emit_mis_density() (vrt_common.hip.h) on a caller's cases. Per
// case fin[8] = x, dir, cs, inv_power and fin[8..10] = the hit point, iin[6] = axis, cell, w0, w1; out[2 * i] = pl, out[2 * i + 1] = pb
__global__ void emit_mis_probe_kernel(const float *fin, const int32_t *iin, float *out, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float *f = fin + (size_t)i * 11u;
    const int32_t *q = iin + (size_t)i * 6u;
    Hit h{};
    h.point = F3{f[8], f[9], f[10]};
    h.axis = q[0];
    h.map = I3{q[1], q[2], q[3]};
    h.h0 = (uint32_t)q[4];
    h.h1 = (uint32_t)q[5];
    float pl, pb;
    emit_mis_density(F3{f[0], f[1], f[2]}, F3{f[3], f[4], f[5]}, f[6], h, f[7], pl, pb);
    out[2 * i] = pl;
    out[2 * i + 1] = pb;
}
}  // namespace vrt

namespace vrt_internal {
bool build_ray_table(const float *m, int W, int H, std::vector<float> &tab, float &z_out);
bool view_matrix_in_range(const float *m);
bool miss_table_fit(const float *tab, float z, int W, int H, vrt::miss::TableFit &f);
bool miss_view_params(const float *inv_view, const float gro[3], const vrt::miss::TableFit &f, vrt::miss::ViewParams &v);
}
using vrt_internal::build_ray_table;
using vrt_internal::view_matrix_in_range;

#define VRT_HIP(c, call)                       \
    do {                                       \
        if ((call) != hipSuccess) return VRT_E_HIP; \
    } while (0)

extern "C" {

// host only: the guided filter's launch geometry as this build has it (vrt_filter.hip.h) -> out[7] = kBlockX, kBlockY, kVarX, kVarY,
// kLatX, kLatY, kLatticeMaxStep
void vrt_test_filter_geometry(int32_t *out) {
    namespace f = vrt::filter;
    const int32_t g[7] = {f::kBlockX, f::kBlockY, f::kVarX, f::kVarY, f::kLatX, f::kLatY, f::kLatticeMaxStep};
    for (int i = 0; i < 7; ++i) out[i] = g[i];
}

// host only: the sun disc's block as the dispatcher makes it (vrt_sun.h sun_block()) -> out[11] = tan_radius, ll, Ln, T, B
void vrt_test_sun_block(const float *light_dir, float tan_radius, float *out) {
    const vrt::Sun s = sun_block(light_dir, tan_radius);
    out[0] = s.tan_radius; out[1] = s.ll;
    for (int i = 0; i < 3; ++i) { out[2 + i] = s.Ln[i]; out[5 + i] = s.T[i]; out[8 + i] = s.B[i]; }
}


// host only: the emitter list as the context makes it (vrt_emitters.h emitter_list()) of a caller's record array (n_records x 2
// words) and world bounds -> N, and the first min(N, cap) entries of four int32 in out (none where N exceeds max_entries)
long vrt_test_emitter_list(const uint32_t *records, size_t n_records, const int *wmin, const int *wmax, uint64_t max_entries, int32_t *out, size_t cap) {
    if (!records || !wmin || !wmax || (cap && !out)) return VRT_E_INVALID;
    std::vector<vrt::Record> recs(n_records);
    for (size_t i = 0; i < n_records; ++i) recs[i] = vrt::Record{records[2 * i], records[2 * i + 1]};
    std::vector<int32_t> list;
    const uint64_t n = emitter_list(recs, wmin, wmax, max_entries, list);
    const size_t take = list.size() / 4 < cap ? list.size() / 4 : cap;
    for (size_t i = 0; i < take * 4; ++i) out[i] = list[i];
    return (long)n;
}

// host only: the weights and thresholds of VRT_EMIT_POWER as the context makes them (vrt_emitters.h emitter_walk(), emitter_weights(),
// emitter_cdf()) of a caller's record array and world bounds -> N, and the first min(N, cap) weights and thresholds (none where N
// exceeds max_entries)
long vrt_test_emitter_cdf(const uint32_t *records, size_t n_records, const int *wmin, const int *wmax, uint64_t max_entries, uint64_t *weights_out,
                          uint32_t *cdf_out, size_t cap) {
    if (!records || !wmin || !wmax || (cap && (!weights_out || !cdf_out))) return VRT_E_INVALID;
    std::vector<vrt::Record> recs(n_records);
    for (size_t i = 0; i < n_records; ++i) recs[i] = vrt::Record{records[2 * i], records[2 * i + 1]};
    std::vector<int32_t> list;
    std::vector<uint32_t> words, cdf;
    std::vector<uint64_t> weights;
    const uint64_t n = emitter_walk(recs, wmin, wmax, max_entries, list, &words);
    emitter_weights(list, words, weights);
    emitter_cdf(weights, cdf);
    const size_t take = cdf.size() < cap ? cdf.size() : cap;
    for (size_t i = 0; i < take; ++i) { weights_out[i] = weights[i]; cdf_out[i] = cdf[i]; }
    return (long)n;
}

// ... and of a caller's list (n entries of four int32) with its record words (two per entry), for lists no tree of a test's size gives
long vrt_test_emitter_cdf_list(const int32_t *list, const uint32_t *words, size_t n, uint64_t *weights_out, uint32_t *cdf_out) {
    if (n && (!list || !words || !weights_out || !cdf_out)) return VRT_E_INVALID;
    const std::vector<int32_t> l(list, list + 4 * n);
    const std::vector<uint32_t> w(words, words + 2 * n);
    std::vector<uint32_t> cdf;
    std::vector<uint64_t> weights;
    emitter_weights(l, w, weights);
    emitter_cdf(weights, cdf);
    for (size_t i = 0; i < n; ++i) { weights_out[i] = weights[i]; cdf_out[i] = cdf[i]; }
    return (long)n;
}

// Device probe of the selection (emit_pick_probe_kernel): a table of n thresholds and `count` draws, host arrays, synchronous.
// out: 2 * count words = j, ticks. The table must be strictly increasing and end at 2^24, as emitter_cdf() makes it.
int vrt_test_emit_pick(int device, const uint32_t *cdf, uint32_t n, const float *u0, uint32_t *out, int count) {
    if (!cdf || !u0 || !out || n < 1 || n > VRT_MAX_EMITTERS || count < 1 || cdf[n - 1] != (1u << 24)) return VRT_E_INVALID;
    VRT_HIP(c, hipSetDevice(device));
    uint32_t *d_cdf = nullptr, *d_out = nullptr;
    float *d_u = nullptr;
    struct Free { uint32_t *&a, *&o; float *&u; ~Free() { (void)hipFree(a); (void)hipFree(o); (void)hipFree(u); } } free_on_exit{d_cdf, d_out, d_u};
    VRT_HIP(c, hipMalloc((void **)&d_cdf, (size_t)n * sizeof(uint32_t)));
    VRT_HIP(c, hipMalloc((void **)&d_u, (size_t)count * sizeof(float)));
    VRT_HIP(c, hipMalloc((void **)&d_out, (size_t)count * 2 * sizeof(uint32_t)));
    VRT_HIP(c, hipMemcpy(d_cdf, cdf, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    VRT_HIP(c, hipMemcpy(d_u, u0, (size_t)count * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(vrt::emit_pick_probe_kernel, dim3((count + 255) / 256), dim3(256), 0, nullptr, d_cdf, n, d_u, d_out, count);
    VRT_HIP(c, hipGetLastError());
    VRT_HIP(c, hipDeviceSynchronize());
    VRT_HIP(c, hipMemcpy(out, d_out, (size_t)count * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return VRT_OK;
}

// Device probe of vrt_set_emitter_mis's densities (emit_mis_probe_kernel): `count` cases of 11 floats and 6 int32 each, host arrays,
// synchronous. out: 2 * count floats = pl, pb. The axis must be 0, 1 or 2.
int vrt_test_emit_mis_density(int device, const float *fin, const int32_t *iin, float *out, int count) {
    if (!fin || !iin || !out || count < 1) return VRT_E_INVALID;
    for (int i = 0; i < count; ++i)
        if (iin[6 * (size_t)i] < 0 || iin[6 * (size_t)i] > 2) return VRT_E_INVALID;
    VRT_HIP(c, hipSetDevice(device));
    float *d_f = nullptr, *d_out = nullptr;
    int32_t *d_i = nullptr;
    struct Free { float *&f, *&o; int32_t *&i; ~Free() { (void)hipFree(f); (void)hipFree(o); (void)hipFree(i); } } free_on_exit{d_f, d_out, d_i};
    VRT_HIP(c, hipMalloc((void **)&d_f, (size_t)count * 11 * sizeof(float)));
    VRT_HIP(c, hipMalloc((void **)&d_i, (size_t)count * 6 * sizeof(int32_t)));
    VRT_HIP(c, hipMalloc((void **)&d_out, (size_t)count * 2 * sizeof(float)));
    VRT_HIP(c, hipMemcpy(d_f, fin, (size_t)count * 11 * sizeof(float), hipMemcpyHostToDevice));
    VRT_HIP(c, hipMemcpy(d_i, iin, (size_t)count * 6 * sizeof(int32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(vrt::emit_mis_probe_kernel, dim3((count + 255) / 256), dim3(256), 0, nullptr, d_f, d_i, d_out, count);
    VRT_HIP(c, hipGetLastError());
    VRT_HIP(c, hipDeviceSynchronize());
    VRT_HIP(c, hipMemcpy(out, d_out, (size_t)count * 2 * sizeof(float), hipMemcpyDeviceToHost));
    return VRT_OK;
}

// host only: Wtot and inv_power of vrt_set_emitter_mis as the context makes them (vrt_emitters.h emitter_cdf(), emitter_inv_power()) of a
// caller's list with its record words
long vrt_test_emitter_inv_power(const int32_t *list, const uint32_t *words, size_t n, uint64_t *wtot_out, float *inv_out) {
    if ((n && (!list || !words)) || !wtot_out || !inv_out) return VRT_E_INVALID;
    const std::vector<int32_t> l(list, list + 4 * n);
    const std::vector<uint32_t> w(words, words + 2 * n);
    std::vector<uint32_t> cdf;
    std::vector<uint64_t> weights;
    emitter_weights(l, w, weights);
    emitter_cdf(weights, cdf, wtot_out);
    *inv_out = emitter_inv_power(*wtot_out);
    return (long)n;
}

// Arithmetic-contract probe (math_probe_kernel / math_probe_full_kernel): out[i] = op(x[i], y[i]) on `device`; host arrays, synchronous.
int vrt_test_math(int device, int op, const float *x, const float *y, float *out, int n) {
    if (!x || !y || !out || n < 1) return VRT_E_INVALID;
    VRT_HIP(c, hipSetDevice(device));
    void *c = nullptr; (void)c;
    hipStream_t stream = nullptr;
    float *dx = nullptr, *dy = nullptr, *dout = nullptr;
    const size_t bytes = (size_t)n * sizeof(float);
    struct Free { float *&a, *&b, *&o; ~Free() { (void)hipFree(a); (void)hipFree(b); (void)hipFree(o); } } free_on_exit{dx, dy, dout};
    VRT_HIP(c, hipMalloc((void **)&dx, bytes));
    VRT_HIP(c, hipMalloc((void **)&dy, bytes));
    VRT_HIP(c, hipMalloc((void **)&dout, bytes));
    VRT_HIP(c, hipMemcpyAsync(dx, x, bytes, hipMemcpyHostToDevice, stream));
    VRT_HIP(c, hipMemcpyAsync(dy, y, bytes, hipMemcpyHostToDevice, stream));
    if (op >= 10 && op < 30)
        hipLaunchKernelGGL(vrt::full::math_probe_full_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, op, dx, dy, dout, n);
    else
        hipLaunchKernelGGL(vrt::math_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, op, dx, dy, dout, n);
    VRT_HIP(c, hipGetLastError());
    VRT_HIP(c, hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, stream));
    VRT_HIP(c, hipStreamSynchronize(stream));
    return VRT_OK;
}

// Device probe of the v4 march step (march_step_probe_kernel): n cases, host arrays, synchronous.
int vrt_test_march_step(int device, const float *in, const int32_t *dpos, uint32_t *out, int n) {
    if (!in || !dpos || !out || n < 1) return VRT_E_INVALID;
    VRT_HIP(c, hipSetDevice(device));
    float *din = nullptr;
    int *ddp = nullptr;
    uint32_t *dout = nullptr;
    struct Free { float *&a; int *&b; uint32_t *&o; ~Free() { (void)hipFree(a); (void)hipFree(b); (void)hipFree(o); } } free_on_exit{din, ddp, dout};
    VRT_HIP(c, hipMalloc((void **)&din, (size_t)n * 16 * sizeof(float)));
    VRT_HIP(c, hipMalloc((void **)&ddp, (size_t)n * 3 * sizeof(int)));
    VRT_HIP(c, hipMalloc((void **)&dout, (size_t)n * 20 * sizeof(uint32_t)));
    VRT_HIP(c, hipMemcpy(din, in, (size_t)n * 16 * sizeof(float), hipMemcpyHostToDevice));
    VRT_HIP(c, hipMemcpy(ddp, dpos, (size_t)n * 3 * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(vrt::march_step_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, din, ddp, dout, n);
    VRT_HIP(c, hipGetLastError());
    VRT_HIP(c, hipMemcpy(out, dout, (size_t)n * 20 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    VRT_HIP(c, hipDeviceSynchronize());
    return VRT_OK;
}

// Host-only (tests): the ray-generation table the dispatcher would build for this inverse projection and frame shape.
// Returns 1 and fills out_x[width], out_y[height], out_z when the projection has a table, 0 when it has none.
int vrt_test_ray_table(const float inv_projection[16], int width, int height, float *out_x, float *out_y, float *out_z) {
    if (!inv_projection || width < 1 || height < 1 || !out_x || !out_y || !out_z) return VRT_E_INVALID;
    std::vector<float> tab;
    float z = 0.0f;
    if (!build_ray_table(inv_projection, width, height, tab, z)) return 0;
    std::memcpy(out_x, tab.data(), (size_t)width * sizeof(float));
    std::memcpy(out_y, tab.data() + width, (size_t)height * sizeof(float));
    *out_z = z;
    return 1;
}
// ... and whether an inverse view matrix keeps the second normalisation in range (view_matrix_in_range())
int vrt_test_view_in_range(const float inv_view[16]) { return inv_view ? (view_matrix_in_range(inv_view) ? 1 : 0) : VRT_E_INVALID; }

// Host-only (tests): what the dispatcher would tell the kernels about wide root 0 for this tree, these world bounds and
// this eye: out[0] = root0_only, out[1] = log2 of the chosen root's side, out[2..4] = its minimum corner, out[5] = log2 of
// the side of build_wide()'s root. Returns 0, VRT_E_MALFORMED, or VRT_E_STATE when the scene has no wide form.
int vrt_test_root0(const uint8_t *texels, size_t used_bytes, const int32_t wmin[3], const int32_t wmax[3], const int32_t eye[3],
                    int32_t out[6]) {
    if (!wmin || !wmax || !eye || !out) return VRT_E_INVALID;
    vrt::Layout lay;
    std::string err;
    if (!vrt::build_layout(texels, used_bytes, lay, err)) return VRT_E_MALFORMED;
    vrt::WideTree wt;
    if (vrt::has_unit_internal_node(lay.records, wmin, wmax) || !vrt::build_wide(lay.records, wmin, wmax, wt, err) || wt.roots.empty())
        return VRT_E_STATE;
    uint32_t node = wt.roots[0].node;
    int shift = wt.roots[0].shift, mn[3] = {wt.roots[0].origin[0], wt.roots[0].origin[1], wt.roots[0].origin[2]};
    out[5] = shift;
    out[0] = vrt::content_only_in_root0(lay.records, wt) ? 1 : 0;
    const int eyes[1][3] = {{eye[0], eye[1], eye[2]}};
    if (out[0]) vrt::tighten_root0(wt, eyes, 1, vrt::v3::kAnchorShift, node, shift, mn);
    out[1] = shift; out[2] = mn[0]; out[3] = mn[1]; out[4] = mn[2];
    return VRT_OK;
}

// Host-only (tests): which side of each one-eye shortcut an accumulation with this thin lens takes (vrt_layout.h lens_select(),
// what enqueue() in vrt_dispatch.cpp consults). out: [0] the box of origins is finite, [1] one eye lookup for every origin,
// [2] one first lookup of the wide kernels, [3] no origin in a medium (the v4 primary kernels), [4] every origin in empty
// space (the opaque chain, given an opaque tree), [5..7] / [8..10] the box's lowest / highest cell, [11] log2 of the side of
// the wide root 0 the launch uses (tightened to the box where root0_only holds; -1: no wide layout).
// Returns 0 or VRT_E_MALFORMED.
int vrt_test_lens_select(const uint8_t *texels, size_t used_bytes, const int32_t wmin[3], const int32_t wmax[3], float voxel_scale,
                         const float cam_pos[4], const float inv_view[16], float aperture, int32_t out[12]) {
    if (!wmin || !wmax || !cam_pos || !inv_view || !out) return VRT_E_INVALID;
    vrt::Layout lay;
    std::string err;
    if (!vrt::build_layout(texels, used_bytes, lay, err)) return VRT_E_MALFORMED;
    vrt::WideTree wt;
    const bool wide_ok = !vrt::has_unit_internal_node(lay.records, wmin, wmax) && vrt::build_wide(lay.records, wmin, wmax, wt, err) &&
                         !wt.roots.empty();
    vrt::LensSel ls;
    vrt::lens_select(lay.records, wide_ok ? &wt : nullptr, wmin, wmax, voxel_scale, cam_pos, inv_view, aperture, ls);
    out[0] = ls.box_valid; out[1] = ls.eye_shared; out[2] = ls.first_shared; out[3] = ls.no_medium; out[4] = ls.empty;
    for (int k = 0; k < 3; ++k) { out[5 + k] = ls.lo[k]; out[8 + k] = ls.hi[k]; }
    out[11] = -1;
    if (wide_ok) {
        uint32_t node = wt.roots[0].node;
        int shift = wt.roots[0].shift, mn[3] = {wt.roots[0].origin[0], wt.roots[0].origin[1], wt.roots[0].origin[2]};
        const int corners[2][3] = {{ls.lo[0], ls.lo[1], ls.lo[2]}, {ls.hi[0], ls.hi[1], ls.hi[2]}};
        if (wt.roots.size() == 1 && ls.box_valid && vrt::content_only_in_root0(lay.records, wt))
            vrt::tighten_root0(wt, corners, 2, vrt::v3::kAnchorShift, node, shift, mn);
        out[11] = shift;
    }
    return VRT_OK;
}

// Host-only (tests without a GPU): the miss mask the dispatcher would give this view of this tree (VRT_OPT_MISS_TILES) -- the same
// occupancy boxes (vrt_layout.cpp), view parameters (vrt_raygen.cpp) and per-box marking (vrt_miss.h mark_box, the function
// miss_mask_kernel runs per box). mask_out: ((W + 7) / 8) * ((H + 7) / 8) bytes, 1 = traced, 0 = every forward-pointing ray of the
// tile misses. stats (optional): [0] boxes, [1] 1 when some box needed the whole view. Returns 1 with a mask, 0 when the view gets
// none (no ray tables, view matrix out of range, view parameters refused, too many boxes), VRT_E_MALFORMED / VRT_E_INVALID.
int vrt_test_miss_mask(const uint8_t *texels, size_t used_bytes, const int32_t wmin[3], const int32_t wmax[3], float voxel_scale,
                       const float inv_proj[16], const float inv_view[16], const float cam_pos[4], int width, int height,
                       uint8_t *mask_out, int32_t stats[2]) {
    if (!wmin || !wmax || !inv_proj || !inv_view || !cam_pos || !mask_out || width < 1 || height < 1) return VRT_E_INVALID;
    vrt::Layout lay;
    std::string err;
    if (!vrt::build_layout(texels, used_bytes, lay, err)) return VRT_E_MALFORMED;
    for (int k = 0; k < 3; ++k)
        if (wmin[k] < -vrt::miss::kMaxWorld || wmax[k] > vrt::miss::kMaxWorld) return 0;
    if (!view_matrix_in_range(inv_view)) return 0;
    std::vector<float> tab;
    float z = 0.0f;
    if (!build_ray_table(inv_proj, width, height, tab, z)) return 0;
    const float gro[3] = {cam_pos[0] * voxel_scale, cam_pos[1] * voxel_scale, cam_pos[2] * voxel_scale};
    if (!vrt::miss::eye_in_world(gro, wmin, wmax)) return 0;
    vrt::miss::ViewParams vp;
    vrt::miss::TableFit fit;
    if (!vrt_internal::miss_table_fit(tab.data(), z, width, height, fit) || !vrt_internal::miss_view_params(inv_view, gro, fit, vp)) return 0;
    std::vector<int> boxes;
    if (!vrt::occupancy_boxes(lay.records, wmin, wmax, (size_t)vrt::miss::kMaxBoxes, boxes)) return 0;
    const size_t tiles = (size_t)vp.tiles_x * (size_t)vp.tiles_y;
    std::memset(mask_out, 0, tiles);
    bool all = false;
    for (size_t i = 0; i + 6 <= boxes.size(); i += 6) {
        const vrt::miss::Box b{{boxes[i], boxes[i + 1], boxes[i + 2]}, {boxes[i + 3], boxes[i + 4], boxes[i + 5]}};
        all = vrt::miss::mark_box(vp, b, mask_out, 1u) || all;
    }
    if (all) std::memset(mask_out, 1, tiles);
    if (stats) { stats[0] = (int32_t)(boxes.size() / 6); stats[1] = all ? 1 : 0; }
    return 1;
}

// Host-only check of the wide layout (tests without a GPU): builds it for the texel stream and world
// bounds and answers n point queries through it. out: n * 8 words = w0, w1, mn[3], mx[3].
// stats (optional): wide nodes, roots. Returns 0, VRT_E_MALFORMED, or VRT_E_STATE when the scene has no wide form.
int vrt_test_wide_find(const uint8_t *texels, size_t used_bytes, const int32_t wmin[3], const int32_t wmax[3],
                        const int32_t *points, size_t n, uint32_t *out, uint32_t *stats) {
    vrt::Layout lay;
    std::string err;
    if (!vrt::build_layout(texels, used_bytes, lay, err)) return VRT_E_MALFORMED;
    vrt::WideTree wt;
    if (!vrt::build_wide(lay.records, wmin, wmax, wt, err)) return VRT_E_STATE;
    if (stats) { stats[0] = wt.n_nodes; stats[1] = (uint32_t)wt.roots.size(); }
    for (size_t i = 0; i < n; ++i) {
        uint32_t w0, w1;
        int mn[3], mx[3];
        (void)vrt::wide_find_host(lay.records, wt, wmin, wmax, points + 3 * i, w0, w1, mn, mx);
        uint32_t *o = out + 8 * i;
        o[0] = w0; o[1] = w1;
        for (int k = 0; k < 3; ++k) { o[2 + k] = (uint32_t)mn[k]; o[5 + k] = (uint32_t)mx[k]; }
    }
    return VRT_OK;
}

// Host-only check of the edit patch (no device): lays out the tree before and after an edit of voxel (x, y, z) from
// their texel streams, patches the "before" structures with the sub-tree taken from the "after" ones, and counts the
// query points whose lookup (leaf words + node box), through the wide layout and through the records alone, differs
// between the patched and the freshly built structures. info: [0] depth of the node replaced (0: no patchable
// ancestor, nothing compared), [1] records appended, [2] wide cells appended, [3] 1 when the stream's texel count
// tracked by the patch equals the "after" stream's. sparse: the sub-tree carries only the nodes that contain the
// voxel, everything else as kKeep records. Returns the number of differing points or a negative code.
long vrt_test_patch_check(const uint8_t *before, size_t before_bytes, const uint8_t *after, size_t after_bytes,
                           const int32_t wmin[3], const int32_t wmax[3], int x, int y, int z, const int32_t *points, size_t n,
                           uint32_t *info, int sparse) {
    vrt::Layout lb, la;
    std::string err;
    if (!vrt::build_layout(before, before_bytes, lb, err) || !vrt::build_layout(after, after_bytes, la, err)) return VRT_E_MALFORMED;
    vrt::WideTree wb, wa;
    const bool wide_b = !vrt::has_unit_internal_node(lb.records, wmin, wmax) && vrt::build_wide(lb.records, wmin, wmax, wb, err);
    const bool wide_a = !vrt::has_unit_internal_node(la.records, wmin, wmax) && vrt::build_wide(la.records, wmin, wmax, wa, err);
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    const int p[3] = {x, y, z};
    vrt::PatchSite site;
    std::vector<vrt::Record> sub;
    int max_depth = 15;
    bool have = false;
    while (max_depth >= 1 && vrt::plan_patch(lb.records, wb, wide_b, wmin, wmax, p, max_depth, site)) {
        if (vrt::extract_subtree(la.records, site.path, site.depth, sub, sparse ? p : nullptr, wmin, wmax)) { have = true; break; }
        max_depth = site.depth - 1;
    }
    if (!have) return 0;
    const size_t n_rec = lb.records.size(), n_cells = wb.cells.size();
    vrt::PatchRanges rg;
    if (!vrt::apply_patch(lb.records, wb, wide_b, site, sub.data(), sub.size(), rg, err)) return VRT_E_MALFORMED;
    bool wide_p = wide_b;
    if (wide_b && rg.wide_invalid) wide_p = !vrt::has_unit_internal_node(lb.records, wmin, wmax) && vrt::build_wide(lb.records, wmin, wmax, wb, err);
    if (info) {
        info[0] = (uint32_t)site.depth;
        info[1] = (uint32_t)(lb.records.size() - n_rec);
        info[2] = (uint32_t)(wb.cells.size() > n_cells ? wb.cells.size() - n_cells : 0);
        info[3] = ((long)(before_bytes / 4) + rg.texel_delta == (long)(after_bytes / 4)) ? 1u : 0u;
    }
    if (wide_p != wide_a) return VRT_E_STATE;
    const vrt::WideTree none;
    long bad = 0;
    for (size_t i = 0; i < n; ++i) {
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 0 && !wide_p) continue;
            uint32_t a0, a1, b0, b1;
            int amn[3], amx[3], bmn[3], bmx[3];
            const int ka = vrt::wide_find_host(lb.records, pass == 0 ? wb : none, wmin, wmax, points + 3 * i, a0, a1, amn, amx);
            const int kb = vrt::wide_find_host(la.records, pass == 0 ? wa : none, wmin, wmax, points + 3 * i, b0, b1, bmn, bmx);
            bool same = ka == kb && a0 == b0 && a1 == b1;
            for (int k = 0; k < 3; ++k) same = same && amn[k] == bmn[k] && amx[k] == bmx[k];
            if (!same) { ++bad; break; }
        }
    }
    return bad;
}

// Host-only check of a CHAIN of edits (no device): vrt_test_patch_check lays both trees out afresh at every step; a session lays the
// first stream out once and then takes every patch, batch and compaction on the SAME records and wide layout, by the rules of
// vrt_patch.cpp restated on host structures alone (patch_host(), patch_device()'s bookkeeping, vrt_patch_plan_box() with its own
// compaction, vrt_compact(), ensure_analysis()). The sub-trees come from the caller (vrth_world_path_records / vrth_world_box_records).
struct PatchSession {
    std::vector<vrt::Record> records;
    vrt::WideTree wide;
    int wmin[3], wmax[3];
    bool analysis_valid = false, wide_ok = false;
    size_t uploaded_records = 0, stream_texels = 0;
    uint32_t tex_dim = 1;
    bool dim_from_texels = false;
    bool open = false, dirty = false, wide_invalid = false;   // the batch
    long texel_delta = 0;
    uint32_t compactions = 0;                                 // all of them, vrt_patch_plan_box's own included
    size_t peak_records = 0;
    // the one cell (last_cell >= 0) or root table entry (last_root >= 0) the last patch re-pointed, with the value it had before:
    // what a device copy that was never made would leave (vrt_test_patch_session_check's `stale`); void once the layout is rebuilt
    long last_cell = -1, last_root = -1;
    vrt::WideCell old_cell{0u, 0u};
    uint32_t old_root = 0;
};

static uint32_t session_dim_of_texels(size_t texels) {   // vrt_scene.cpp dim_of_texels(): ceil(cbrt()), at least 1
    const size_t d = (size_t)ceil(cbrt((double)texels));
    return (uint32_t)(d == 0 ? 1 : d);
}

static void session_ensure(PatchSession *s) {   // ensure_analysis()
    if (s->analysis_valid) return;
    std::string why;
    s->wide_ok = !vrt::has_unit_internal_node(s->records, s->wmin, s->wmax) && vrt::build_wide(s->records, s->wmin, s->wmax, s->wide, why);
    s->last_cell = s->last_root = -1;
    s->analysis_valid = true;
}

static void session_compact(PatchSession *s) {   // vrt_compact()
    vrt::compact_records(s->records);
    s->uploaded_records = s->records.size();
    s->analysis_valid = false;
    ++s->compactions;
}

static void session_end(PatchSession *s) {   // patch_device(): what it keeps in the context beside the copies
    const bool was_dirty = s->dirty, invalid = s->wide_invalid;
    const long delta = s->texel_delta;
    s->open = s->dirty = s->wide_invalid = false;
    s->texel_delta = 0;
    if (!was_dirty) return;
    s->stream_texels = (size_t)((long)s->stream_texels + delta);
    if (s->dim_from_texels) s->tex_dim = session_dim_of_texels(s->stream_texels);
    if (s->wide_ok && invalid) s->analysis_valid = false;
}

// Host-only: the sub-tree under the node reached by `depth` child indices in a fresh layout of a stream, as vrt_patch_apply takes it
// (vrt::extract_subtree): hand-written streams hold what the host library never emits. -> the record count (the first min(count,
// cap) records in out), or a negative code.
long vrt_test_extract_subtree(const uint8_t *texels, size_t used_bytes, const uint8_t *path, int depth, uint32_t *out, size_t cap) {
    if (!path || depth < 1 || depth > 15 || (cap && !out)) return VRT_E_INVALID;
    vrt::Layout lay;
    std::string err;
    if (!vrt::build_layout(texels, used_bytes, lay, err)) return VRT_E_MALFORMED;
    std::vector<vrt::Record> sub;
    if (!vrt::extract_subtree(lay.records, path, depth, sub)) return VRT_E_STATE;
    for (size_t i = 0; i < sub.size() && i < cap; ++i) { out[2 * i] = sub[i].w0; out[2 * i + 1] = sub[i].w1; }
    return (long)sub.size();
}

// (re)starts the session from a full upload of this stream (vrt_upload_octree); h = NULL: a new session. NULL when malformed.
void *vrt_test_patch_session_upload(void *h, const uint8_t *texels, size_t used_bytes, uint32_t tex_dim, const int32_t wmin[3],
                                    const int32_t wmax[3]) {
    if (!wmin || !wmax) return nullptr;
    PatchSession *s = static_cast<PatchSession *>(h);
    if (s && s->open) return nullptr;
    vrt::Layout lay;
    std::string err;
    if (!vrt::build_layout(texels, used_bytes, lay, err)) return nullptr;
    if (!s) s = new PatchSession();
    for (int k = 0; k < 3; ++k) { s->wmin[k] = wmin[k]; s->wmax[k] = wmax[k]; }
    s->records.swap(lay.records);
    s->uploaded_records = s->records.size();
    s->stream_texels = used_bytes / 4;
    s->tex_dim = tex_dim ? tex_dim : 1;
    s->dim_from_texels = s->tex_dim == session_dim_of_texels(s->stream_texels);
    s->analysis_valid = false;
    if (s->records.size() > s->peak_records) s->peak_records = s->records.size();
    return s;
}

void vrt_test_patch_session_close(void *h) { delete static_cast<PatchSession *>(h); }

// vrt_patch_plan_box(): 0 and the plan, or VRT_E_STATE when the edit needs a full upload
int vrt_test_patch_session_plan(void *h, const int32_t lo[3], const int32_t hi[3], int max_depth, int32_t *depth_out, uint8_t path_out[16]) {
    PatchSession *s = static_cast<PatchSession *>(h);
    if (!s || !lo || !hi || !depth_out || !path_out || lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]) return VRT_E_INVALID;
    session_ensure(s);
    if (!s->open && s->records.size() > 2 * s->uploaded_records + (1u << 12)) {
        session_compact(s);
        session_ensure(s);
    }
    const int p[3] = {lo[0], lo[1], lo[2]};
    int md = max_depth > 15 ? 15 : max_depth;
    while (md >= 1) {
        vrt::PatchSite site;
        if (!vrt::plan_patch(s->records, s->wide, s->wide_ok && !s->wide_invalid, s->wmin, s->wmax, p, md, site)) break;
        int mn[3], mx[3];
        for (int k = 0; k < 3; ++k) { mn[k] = s->wmin[k]; mx[k] = s->wmax[k]; }
        for (int d = 0; d < site.depth; ++d)
            for (int k = 0; k < 3; ++k) {
                const int mid = mn[k] + ((mx[k] - mn[k]) >> 1);
                if ((site.path[d] >> (2 - k)) & 1u) mn[k] = mid; else mx[k] = mid;
            }
        if (hi[0] < mx[0] && hi[1] < mx[1] && hi[2] < mx[2] && hi[0] >= mn[0] && hi[1] >= mn[1] && hi[2] >= mn[2]) {
            *depth_out = site.depth;
            std::memcpy(path_out, site.path, 16);
            return VRT_OK;
        }
        md = site.depth - 1;
    }
    return VRT_E_STATE;
}

int vrt_test_patch_session_begin(void *h) {
    PatchSession *s = static_cast<PatchSession *>(h);
    if (!s || s->open) return VRT_E_STATE;
    session_ensure(s);
    s->open = true;
    s->dirty = s->wide_invalid = false;
    s->texel_delta = 0;
    return VRT_OK;
}

int vrt_test_patch_session_end(void *h) {
    PatchSession *s = static_cast<PatchSession *>(h);
    if (!s || !s->open) return VRT_E_STATE;
    session_end(s);
    return VRT_OK;
}

// vrt_patch_apply() with patch_host()'s batch rule. info (optional): [0] the patch voided the wide layout, [1] a cell was re-pointed,
// [2] a root changed.
int vrt_test_patch_session_apply(void *h, int depth, const uint8_t path[16], const uint32_t *sub, size_t n_sub, uint32_t info[3]) {
    PatchSession *s = static_cast<PatchSession *>(h);
    if (!s || !path || !sub || depth < 1 || depth > 15) return VRT_E_INVALID;
    const bool single = !s->open;
    if (single) { const int r = vrt_test_patch_session_begin(h); if (r) return r; }
    int lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = s->wmin[k]; hi[k] = s->wmax[k]; }
    for (int d = 0; d < depth; ++d) {
        if (path[d] > 7) { if (single) s->open = false; return VRT_E_INVALID; }
        for (int k = 0; k < 3; ++k) {
            const int mid = lo[k] + ((hi[k] - lo[k]) >> 1);
            if ((path[d] >> (2 - k)) & 1u) lo[k] = mid; else hi[k] = mid;
        }
    }
    const bool wide_now = s->wide_ok && !s->wide_invalid;
    vrt::PatchSite site;
    vrt::PatchRanges rg;
    std::string why;
    if (!vrt::plan_patch(s->records, s->wide, wide_now, s->wmin, s->wmax, lo, depth, site) || site.depth != depth ||
        std::memcmp(site.path, path, (size_t)depth) != 0) { if (single) s->open = false; return VRT_E_STATE; }
    vrt::WideCell old_cell{0u, 0u};
    uint32_t old_root = 0;
    const size_t at = (size_t)site.parent_node * 64 + site.parent_cell;
    if (wide_now && site.root_index >= 0) old_root = s->wide.roots[(size_t)site.root_index].node;
    else if (wide_now && at < s->wide.cells.size()) old_cell = s->wide.cells[at];
    if (!vrt::apply_patch(s->records, s->wide, wide_now, site, reinterpret_cast<const vrt::Record *>(sub), n_sub, rg, why)) {
        if (single) s->open = false;
        return VRT_E_MALFORMED;
    }
    s->dirty = true;
    s->texel_delta += rg.texel_delta;
    if (info) { info[0] = rg.wide_invalid ? 1u : 0u; info[1] = rg.cell_repointed ? 1u : 0u; info[2] = (wide_now && site.root_index >= 0) ? 1u : 0u; }
    if (wide_now) {
        s->wide_invalid = s->wide_invalid || rg.wide_invalid;
        if (!rg.wide_invalid && site.root_index >= 0 && s->wide.roots[(size_t)site.root_index].node != old_root) {
            s->last_root = site.root_index; s->last_cell = -1; s->old_root = old_root;
        } else if (!rg.wide_invalid && rg.cell_repointed) {
            s->last_cell = (long)at; s->last_root = -1; s->old_cell = old_cell;
        }
    }
    if (s->records.size() > s->peak_records) s->peak_records = s->records.size();
    if (single) session_end(s);
    return VRT_OK;
}

int vrt_test_patch_session_compact(void *h) {
    PatchSession *s = static_cast<PatchSession *>(h);
    if (!s || s->open) return VRT_E_STATE;
    session_compact(s);
    return VRT_OK;
}

// counters: [0] records now, [1] compactions so far, [2] the largest record count so far, [3] wide cells now
void vrt_test_patch_session_counts(void *h, uint64_t out[4]) {
    PatchSession *s = static_cast<PatchSession *>(h);
    out[0] = s->records.size(); out[1] = s->compactions; out[2] = s->peak_records; out[3] = s->wide.cells.size();
}

// The patched structures, as the next dispatch would find them, against a fresh layout of `after`, on n points and for an eye cell:
// out[0] points that differ through the cells (0xffffffff: one side has a wide layout and the other none), [1] through the records
// alone, [2] / [3] tree_is_opaque patched / fresh, [4] 1 when emitter list and thresholds are equal, [5] / [6] their lengths,
// [7] 1 when both have a wide form, [8..13] / [14..19] vrt_test_root0's six findings patched / fresh, [20] / [21] tracked and actual
// texel count, [22] / [23] tracked u_texDim and after_dim, [24] live records, [25] all records, [26] the fresh layout's, [27] 1 when
// the last patch re-pointed a cell or a root and the layout has not been rebuilt since. With list_out / cdf_out (cap entries): the
// patched array's emitter list and thresholds. stale = 1: the comparison is made with that cell or root at its value from before the
// patch -- the sensitivity check of out[0].
int vrt_test_patch_session_check(void *h, const uint8_t *after, size_t after_bytes, uint32_t after_dim, const int32_t *points, size_t n,
                                 const int32_t eye[3], int stale, uint32_t out[28], int32_t *list_out, uint32_t *cdf_out, size_t cap) {
    PatchSession *s = static_cast<PatchSession *>(h);
    if (!s || !eye || !out || (n && !points) || s->open) return VRT_E_INVALID;
    vrt::Layout la;
    std::string err;
    if (!vrt::build_layout(after, after_bytes, la, err)) return VRT_E_MALFORMED;
    session_ensure(s);
    out[27] = (s->wide_ok && (s->last_cell >= 0 || s->last_root >= 0)) ? 1u : 0u;
    struct Swap {   // the stale value in for the length of the check
        PatchSession *s; bool on;
        void flip() {
            if (!on) return;
            if (s->last_cell >= 0) std::swap(s->wide.cells[(size_t)s->last_cell], s->old_cell);
            else std::swap(s->wide.roots[(size_t)s->last_root].node, s->old_root);
        }
        ~Swap() { flip(); }
    } swap{s, stale && out[27]};
    swap.flip();
    vrt::WideTree wa;
    const bool wide_a = !vrt::has_unit_internal_node(la.records, s->wmin, s->wmax) && vrt::build_wide(la.records, s->wmin, s->wmax, wa, err);
    const vrt::WideTree none;
    uint32_t bad_cells = 0, bad_records = 0;
    for (size_t i = 0; i < n; ++i)
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 0 && !(s->wide_ok && wide_a)) continue;
            uint32_t a0, a1, b0, b1;
            int amn[3], amx[3], bmn[3], bmx[3];
            const int ka = vrt::wide_find_host(s->records, pass == 0 ? s->wide : none, s->wmin, s->wmax, points + 3 * i, a0, a1, amn, amx);
            const int kb = vrt::wide_find_host(la.records, pass == 0 ? wa : none, s->wmin, s->wmax, points + 3 * i, b0, b1, bmn, bmx);
            bool same = ka == kb && a0 == b0 && a1 == b1;
            for (int k = 0; k < 3; ++k) same = same && amn[k] == bmn[k] && amx[k] == bmx[k];
            if (!same) ++(pass == 0 ? bad_cells : bad_records);
        }
    out[0] = s->wide_ok == wide_a ? bad_cells : 0xffffffffu;
    out[1] = bad_records;
    out[2] = vrt::tree_is_opaque(s->records) ? 1u : 0u;
    out[3] = vrt::tree_is_opaque(la.records) ? 1u : 0u;
    std::vector<int32_t> lp, lf;
    std::vector<uint32_t> wp, wf, cp, cf;
    std::vector<uint64_t> weights;
    emitter_walk(s->records, s->wmin, s->wmax, 1u << 20, lp, &wp);
    emitter_weights(lp, wp, weights);
    emitter_cdf(weights, cp);
    emitter_walk(la.records, s->wmin, s->wmax, 1u << 20, lf, &wf);
    emitter_weights(lf, wf, weights);
    emitter_cdf(weights, cf);
    out[4] = (lp == lf && cp == cf) ? 1u : 0u;
    out[5] = (uint32_t)cp.size();
    out[6] = (uint32_t)cf.size();
    for (size_t i = 0; i < cp.size() && i < cap; ++i) {
        if (list_out) std::memcpy(list_out + 4 * i, lp.data() + 4 * i, 4 * sizeof(int32_t));
        if (cdf_out) cdf_out[i] = cp[i];
    }
    const bool both = s->wide_ok && wide_a && !s->wide.roots.empty() && !wa.roots.empty();
    out[7] = both ? 1u : 0u;
    for (int side = 0; side < 2; ++side) {
        uint32_t *o = out + 8 + 6 * side;
        for (int k = 0; k < 6; ++k) o[k] = 0;
        if (!both) continue;
        const vrt::WideTree &wt = side ? wa : s->wide;
        const std::vector<vrt::Record> &recs = side ? la.records : s->records;
        uint32_t node = wt.roots[0].node;
        int shift = wt.roots[0].shift, mn[3] = {wt.roots[0].origin[0], wt.roots[0].origin[1], wt.roots[0].origin[2]};
        o[5] = (uint32_t)shift;
        o[0] = vrt::content_only_in_root0(recs, wt) ? 1u : 0u;
        const int eyes[1][3] = {{eye[0], eye[1], eye[2]}};
        if (o[0]) vrt::tighten_root0(wt, eyes, 1, vrt::v3::kAnchorShift, node, shift, mn);
        o[1] = (uint32_t)shift; o[2] = (uint32_t)mn[0]; o[3] = (uint32_t)mn[1]; o[4] = (uint32_t)mn[2];
    }
    out[20] = (uint32_t)s->stream_texels;
    out[21] = (uint32_t)(after_bytes / 4);
    out[22] = s->tex_dim;
    out[23] = after_dim;
    std::vector<vrt::Record> live(s->records);
    vrt::compact_records(live);
    out[24] = (uint32_t)live.size();
    out[25] = (uint32_t)s->records.size();
    out[26] = (uint32_t)la.records.size();
    return VRT_OK;
}

// Host-only: what the dispatcher concludes about a tree before it runs VRT_MODE_FULL without a ray stack (vrt::tree_is_opaque):
// 1 / 0, or VRT_E_MALFORMED.
int vrt_test_tree_is_opaque(const uint8_t *texels, size_t used_bytes) {
    vrt::Layout lay;
    std::string err;
    if (!vrt::build_layout(texels, used_bytes, lay, err)) return VRT_E_MALFORMED;
    return vrt::tree_is_opaque(lay.records) ? 1 : 0;
}

// Host-only view of the device layout for tests that run without a GPU:
// writes up to cap records (8 bytes each) and returns the record count, or <0.
long vrt_test_build_layout(const uint8_t *texels, size_t used_bytes, uint32_t *records_out, size_t cap_records,
                            vrt_scene_info *info) {
    vrt::Layout lay;
    std::string err;
    if (!vrt::build_layout(texels, used_bytes, lay, err)) return VRT_E_MALFORMED;
    if (records_out)
        for (size_t i = 0; i < lay.records.size() && i < cap_records; ++i) {
            records_out[2 * i] = lay.records[i].w0;
            records_out[2 * i + 1] = lay.records[i].w1;
        }
    if (info) {
        std::memset(info, 0, sizeof *info);
        info->n_texels = (uint32_t)(used_bytes / 4);
        info->n_records = (uint32_t)lay.records.size();
        info->n_internal = lay.n_internal;
        info->n_leaves = lay.n_leaves;
        info->max_depth = lay.max_depth;
    }
    return (long)lay.records.size();
}

// The feedback scheduler's order kernel on a synthetic frame: tile_ticks[n_groups * 4] -> order[n_groups] and the split count the
// kernel leaves behind it (KArgs::split_count). Host arrays, synchronous.
int vrt_test_tile_order(int device, const uint32_t *tile_ticks, uint32_t n_groups, uint32_t wave_slots, uint32_t *order_out, uint32_t *split_out) {
    if (!tile_ticks || !order_out || !split_out || n_groups < 1 || n_groups > 36864) return VRT_E_INVALID;
    void *c = nullptr; (void)c;
    VRT_HIP(c, hipSetDevice(device));
    uint32_t *d_cost = nullptr, *d_order = nullptr;
    VRT_HIP(c, hipMalloc((void **)&d_cost, (size_t)n_groups * 4 * sizeof(uint32_t)));
    VRT_HIP(c, hipMalloc((void **)&d_order, ((size_t)n_groups + 1) * sizeof(uint32_t)));
    VRT_HIP(c, hipMemcpy(d_cost, tile_ticks, (size_t)n_groups * 4 * sizeof(uint32_t), hipMemcpyHostToDevice));
    const size_t lds = (size_t)n_groups * sizeof(uint32_t);
    if (lds > 48 * 1024) VRT_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&vrt::tile_order_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 36864 * 4));
    hipLaunchKernelGGL(vrt::tile_order_kernel, dim3(1), dim3(1024), lds, 0, (const uint4 *)d_cost, n_groups, d_order, wave_slots);
    VRT_HIP(c, hipGetLastError());
    VRT_HIP(c, hipDeviceSynchronize());
    VRT_HIP(c, hipMemcpy(order_out, d_order, (size_t)n_groups * sizeof(uint32_t), hipMemcpyDeviceToHost));
    VRT_HIP(c, hipMemcpy(split_out, d_order + n_groups, sizeof(uint32_t), hipMemcpyDeviceToHost));
    (void)hipFree(d_cost);
    (void)hipFree(d_order);
    return VRT_OK;
}

// The adaptive accumulation's stopping rule (include/vrt.h vrt_accum_begin_adaptive) as the kernels evaluate it: 1 active, 0 not
int vrt_test_adaptive_rule(uint32_t n, uint64_t s, uint64_t q, uint32_t min, uint32_t max, uint32_t tol) {
    return vrt::accum::adaptive_active(n, s, q, min, max, tol) ? 1 : 0;
}

// The same on the device, for `count` states: host arrays, synchronous
int vrt_test_adaptive_rule_device(int device, const uint32_t *n, const uint64_t *s, const uint64_t *q, uint32_t min, uint32_t max,
                                  uint32_t tol, uint32_t *out, int count) {
    if (!n || !s || !q || !out || count < 1 || count > (1 << 20)) return VRT_E_INVALID;
    void *c = nullptr; (void)c;
    VRT_HIP(c, hipSetDevice(device));
    uint32_t *d_n = nullptr, *d_out = nullptr;
    uint64_t *d_s = nullptr, *d_q = nullptr;
    VRT_HIP(c, hipMalloc((void **)&d_n, (size_t)count * 4));
    VRT_HIP(c, hipMalloc((void **)&d_out, (size_t)count * 4));
    VRT_HIP(c, hipMalloc((void **)&d_s, (size_t)count * 8));
    VRT_HIP(c, hipMalloc((void **)&d_q, (size_t)count * 8));
    VRT_HIP(c, hipMemcpy(d_n, n, (size_t)count * 4, hipMemcpyHostToDevice));
    VRT_HIP(c, hipMemcpy(d_s, s, (size_t)count * 8, hipMemcpyHostToDevice));
    VRT_HIP(c, hipMemcpy(d_q, q, (size_t)count * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(vrt::adaptive_probe_kernel, dim3((count + 255) / 256), dim3(256), 0, 0, d_n, d_s, d_q, min, max, tol, d_out, count);
    VRT_HIP(c, hipGetLastError());
    VRT_HIP(c, hipDeviceSynchronize());
    VRT_HIP(c, hipMemcpy(out, d_out, (size_t)count * 4, hipMemcpyDeviceToHost));
    (void)hipFree(d_n);
    (void)hipFree(d_out);
    (void)hipFree(d_s);
    (void)hipFree(d_q);
    return VRT_OK;
}

}  // extern "C"
