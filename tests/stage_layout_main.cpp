// stage_layout_main.cpp -- the layouts of csrc/vrt_stage.h against the offset arithmetic every host form wrote out by hand before
// there was a staging type. For every staging block of the library the program declares the planes the way the entry point does
// and compares each plane's offset and the block's total with the old formula, written out literally here; it also checks that
// no two planes with room overlap, that every plane lies inside the total and on the stage's alignment, and that an output the
// caller did not ask for is a null pointer for the launch. Prints one line per row; the first difference ends it with status 1.
// Built by tests/test_stage_layout.py with the host sanitizers; includes the layout part of the header only (no HIP).
#define VRT_STAGE_LAYOUT_ONLY
#include "vrt_stage.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using vrt_stage::Layout;

namespace {

char g_host;                                                                  // what a caller's non-null buffer points at
char *const kBase = reinterpret_cast<char *>(static_cast<uintptr_t>(1) << 40);   // a block's address: 256-aligned, never dereferenced
const size_t kRays[] = {1, 2, 63, 64, 65, 1000, (size_t)1 << 30};
const size_t kPixels[] = {1, 64, 72 * 40, 1920 * 1080, (size_t)7680 * 4320};
constexpr size_t kHistory = 48;
long g_cases = 0;

size_t align256(size_t b) { return (b + 255u) & ~(size_t)255u; }
size_t align16(size_t b) { return (b + 15u) & ~(size_t)15u; }
void *want(unsigned mask, int bit) { return (mask >> bit) & 1u ? &g_host : nullptr; }

[[noreturn]] void fail(const char *row, const std::string &cse, const std::string &what) {
    std::printf("%s [%s]: %s\n", row, cse.c_str(), what.c_str());
    std::exit(1);
}

// One expected plane: the old formula's offset, and whether the launch gets a pointer
struct Expect {
    size_t offset;
    bool present;
    size_t align;
};

void check(const char *row, const std::string &cse, Layout &st, const std::vector<Expect> &e, size_t total) {
    ++g_cases;
    st.base = kBase;
    if ((size_t)st.n != e.size()) fail(row, cse, "declares " + std::to_string(st.n) + " planes, expected " + std::to_string(e.size()));
    if (st.total != total) fail(row, cse, "total " + std::to_string(st.total) + ", the old formula gives " + std::to_string(total));
    for (int i = 0; i < st.n; ++i) {
        const vrt_stage::Plane &p = st.plane[i];
        const std::string name = "plane " + std::to_string(i);
        if (p.offset != e[i].offset) fail(row, cse, name + " at " + std::to_string(p.offset) + ", the old formula gives " + std::to_string(e[i].offset));
        if (p.offset % e[i].align) fail(row, cse, name + " at " + std::to_string(p.offset) + " is not on the alignment " + std::to_string(e[i].align));
        if (p.offset + p.bytes > st.total) fail(row, cse, name + " ends behind the total");
        for (int j = 0; j < i; ++j) {
            const vrt_stage::Plane &q = st.plane[j];
            if (p.bytes && q.bytes && p.offset < q.offset + q.bytes && q.offset < p.offset + p.bytes) fail(row, cse, name + " overlaps plane " + std::to_string(j));
        }
        char *const at = st.at<char>(i);
        if (e[i].present ? at != kBase + p.offset : at != nullptr) fail(row, cse, name + (e[i].present ? ": wrong pointer for the launch" : ": not null for the launch"));
    }
}

std::string batch_case(size_t n, int stride, unsigned mask) {
    return "n " + std::to_string(n) + ", stride " + std::to_string(stride) + ", outputs " + std::to_string(mask);
}
std::string frame_case(size_t px, unsigned mask) { return "px " + std::to_string(px) + ", outputs " + std::to_string(mask); }

void cast_rays() {
    for (size_t n : kRays)
        for (int stride : {0, 3}) {
            const size_t o_bytes = (stride ? n : 1) * 3 * sizeof(float), d_bytes = n * 3 * sizeof(float), out_bytes = n * 40;
            Layout st(256);
            st.in((stride ? n : 1) * 3 * sizeof(float), &g_host);
            st.in(n * 3 * sizeof(float), &g_host);
            st.out(n * 40, &g_host);
            check("vrt_cast_rays", batch_case(n, stride, 1), st, {{0, true, 256}, {align256(o_bytes), true, 256}, {align256(o_bytes) + align256(d_bytes), true, 256}},
                  align256(o_bytes) + align256(d_bytes) + out_bytes);
        }
}

void find_voxels() {
    for (size_t n : kRays) {
        const size_t bytes = n * 3 * sizeof(uint32_t);
        Layout st(256);
        st.in(n * 3 * sizeof(int32_t), &g_host);
        st.out(n * 3 * sizeof(uint32_t), &g_host);
        st.kept(0);
        check("vrt_find_voxels", batch_case(n, 3, 1), st, {{0, true, 256}, {align256(bytes), true, 256}, {2 * align256(bytes), true, 256}}, 2 * align256(bytes));
    }
}

void shade_rays() {
    for (size_t n : kRays)
        for (int stride : {0, 3})
            for (unsigned m = 0; m < 4; ++m) {
                void *out_rgba8 = want(m, 0), *out_id_dist = want(m, 1);
                const size_t o_bytes = (stride ? n : 1) * 3 * sizeof(float), d_bytes = n * 3 * sizeof(float);
                const size_t rgba_bytes = out_rgba8 ? n * 4 : 0, id_bytes = out_id_dist ? n * 8 : 0;
                Layout st(256);
                st.in((stride ? n : 1) * 3 * sizeof(float), &g_host);
                st.in(n * 3 * sizeof(float), &g_host);
                st.out(out_rgba8 ? n * 4 : 0, out_rgba8);
                st.out(out_id_dist ? n * 8 : 0, out_id_dist);
                check("vrt_shade_rays", batch_case(n, stride, m), st,
                      {{0, true, 256},
                       {align256(o_bytes), true, 256},
                       {align256(o_bytes) + align256(d_bytes), out_rgba8 != nullptr, 256},
                       {align256(o_bytes) + align256(d_bytes) + align256(rgba_bytes), out_id_dist != nullptr, 256}},
                      align256(o_bytes) + align256(d_bytes) + align256(rgba_bytes) + id_bytes);
            }
}

void shade_rays_hdr() {
    for (size_t n : kRays)
        for (int stride : {0, 3})
            for (unsigned m = 0; m < 8; ++m) {
                void *out_rgba8 = want(m, 0), *out_id_dist = want(m, 1), *out_rgb = want(m, 2);
                const size_t o_bytes = (stride ? n : 1) * 3 * sizeof(float), d_bytes = n * 3 * sizeof(float);
                const size_t rgba_bytes = out_rgba8 ? n * 4 : 0, id_bytes = out_id_dist ? n * 8 : 0, rgb_bytes = out_rgb ? n * 12 : 0;
                const size_t out = align256(o_bytes) + align256(d_bytes);
                Layout st(256);
                st.in((stride ? n : 1) * 3 * sizeof(float), &g_host);
                st.in(n * 3 * sizeof(float), &g_host);
                st.out(out_rgba8 ? n * 4 : 0, out_rgba8);
                st.out(out_id_dist ? n * 8 : 0, out_id_dist);
                st.out(out_rgb ? n * 12 : 0, out_rgb);
                check("vrt_shade_rays_hdr", batch_case(n, stride, m), st,
                      {{0, true, 256},
                       {align256(o_bytes), true, 256},
                       {out, out_rgba8 != nullptr, 256},
                       {out + align256(rgba_bytes), out_id_dist != nullptr, 256},
                       {out + align256(rgba_bytes) + align256(id_bytes), out_rgb != nullptr, 256}},
                      align256(o_bytes) + align256(d_bytes) + align256(rgba_bytes) + align256(id_bytes) + rgb_bytes);
            }
}

void guide_rays() {
    for (size_t n : kRays)
        for (int stride : {0, 3})
            for (unsigned m = 0; m < 16; ++m) {
                void *out_normal = want(m, 0), *out_albedo = want(m, 1), *out_depth = want(m, 2), *out_hit = want(m, 3);
                const size_t o_bytes = (stride ? n : 1) * 3 * sizeof(float), d_bytes = n * 3 * sizeof(float);
                const size_t nb = out_normal ? n * 12 : 0, ab = out_albedo ? n * 16 : 0, db = out_depth ? n * 4 : 0, hb = out_hit ? n : 0;
                const size_t out = align256(o_bytes) + align256(d_bytes);
                Layout st(256);
                st.in((stride ? n : 1) * 3 * sizeof(float), &g_host);
                st.in(n * 3 * sizeof(float), &g_host);
                st.out(out_normal ? n * 12 : 0, out_normal);
                st.out(out_albedo ? n * 16 : 0, out_albedo);
                st.out(out_depth ? n * 4 : 0, out_depth);
                st.out(out_hit ? n : 0, out_hit);
                check("vrt_guide_rays", batch_case(n, stride, m), st,
                      {{0, true, 256},
                       {align256(o_bytes), true, 256},
                       {out, out_normal != nullptr, 256},
                       {out + align256(nb), out_albedo != nullptr, 256},
                       {out + align256(nb) + align256(ab), out_depth != nullptr, 256},
                       {out + align256(nb) + align256(ab) + align256(db), out_hit != nullptr, 256}},
                      align256(o_bytes) + align256(d_bytes) + align256(nb) + align256(ab) + align256(db) + hb);
            }
}

void accum_guides() {
    for (size_t px : kPixels)
        for (unsigned m = 0; m < 16; ++m) {
            Layout st(4);
            st.out(px * 12, want(m, 0));
            st.out(px * 16, want(m, 1));
            st.out(px * 4, want(m, 2));
            st.out(px * 4, want(m, 3));
            check("vrt_accum_guides", frame_case(px, m), st,
                  {{0, want(m, 0) != nullptr, 4},
                   {px * 3 * sizeof(float), want(m, 1) != nullptr, 4},
                   {px * 7 * sizeof(float), want(m, 2) != nullptr, 4},
                   {px * 8 * sizeof(float), want(m, 3) != nullptr, 4}},
                  px * 9 * sizeof(float));
        }
}

// vrt_filter.cpp declare(); host: the five inputs are the caller's (else made on the device, the accumulation forms); m: variance in,
// out_rgb, out_rgba8, out_variance
void filter(bool var, bool host) {
    const char *row = var ? (host ? "vrt_filter_hdr_var_host" : "vrt_accum_resolve_hdr_filtered_var") : (host ? "vrt_filter_hdr_host" : "vrt_accum_resolve_hdr_filtered");
    for (size_t px : kPixels)
        for (unsigned m = 0; m < 16; ++m) {
            if ((!var && (m & 9u)) || (!host && (m & 1u))) continue;   // the guide-only forms have no variance plane, the accumulation no variance input
            const vrt_stage::Dir in = host ? vrt_stage::kIn : vrt_stage::kKept;
            void *const plane = host ? &g_host : nullptr;
            Layout st(4);
            st.add(in, px * 12, plane);
            st.add(in, px * 12, plane);
            st.add(in, px * 16, plane);
            st.add(in, px * 4, plane);
            st.add(in, px * 4, plane);
            st.out(px * 12, want(m, 1));
            st.out(px * 4, want(m, 2));
            st.in(var ? px * 4 : 0, want(m, 0));
            st.out(var ? px * 4 : 0, want(m, 3));
            const size_t f = sizeof(float);
            check(row, frame_case(px, m), st,
                  {{0, true, 4},
                   {px * 3 * f, true, 4},
                   {px * 6 * f, true, 4},
                   {px * 10 * f, true, 4},
                   {px * 11 * f, true, 4},
                   {px * 12 * f, want(m, 1) != nullptr, 4},
                   {px * 15 * f, want(m, 2) != nullptr, 4},
                   {px * 16 * f, want(m, 0) != nullptr, 4},
                   {var ? px * 17 * f : px * 16 * f, want(m, 3) != nullptr, 4}},
                  px * (var ? 72 : 64));
        }
}

void temporal_host() {   // m: history_in, out_rgb, out_variance
    for (size_t px : kPixels)
        for (unsigned m = 0; m < 8; ++m) {
            Layout st(4);
            st.in(px * kHistory, want(m, 0));
            st.out(px * kHistory, &g_host);
            st.in(px * 12, &g_host);
            st.in(px * 12, &g_host);
            st.in(px * 4, &g_host);
            st.in(px * 4, &g_host);
            st.out(px * 12, want(m, 1));
            st.out(px * 4, want(m, 2));
            const size_t rgb = 2 * px * kHistory, f = sizeof(float);
            check("vrt_temporal_hdr_host", frame_case(px, m), st,
                  {{0, want(m, 0) != nullptr, 16},
                   {px * kHistory, true, 16},
                   {rgb, true, 4},
                   {rgb + px * 3 * f, true, 4},
                   {rgb + px * 6 * f, true, 4},
                   {rgb + px * 7 * f, true, 4},
                   {rgb + px * 8 * f, want(m, 1) != nullptr, 4},
                   {rgb + px * 11 * f, want(m, 2) != nullptr, 4}},
                  px * (2 * kHistory + 12 + 12 + 4 + 4 + 12 + 4));
        }
}

void temporal_accum() {   // the host form; m: history_in, out_integrated, out_rgb, out_rgba8, out_variance
    for (size_t px : kPixels)
        for (unsigned m = 0; m < 32; ++m) {
            Layout st(4);
            for (size_t bytes : {12, 12, 16, 4, 4}) st.kept(px * bytes);
            st.kept(px * 12, want(m, 1));
            st.kept(px * 4);
            st.out(px * 12, want(m, 2));
            st.out(px * 4, want(m, 3));
            st.out(px * 4, want(m, 4));
            st.align = 16;
            st.in(px * kHistory, want(m, 0));
            st.out(px * kHistory, &g_host);
            const size_t f = sizeof(float), plane_bytes = px * 21 * f;
            check("vrt_accum_resolve_hdr_temporal", frame_case(px, m), st,
                  {{0, true, 4},
                   {px * 3 * f, true, 4},
                   {px * 6 * f, true, 4},
                   {px * 10 * f, true, 4},
                   {px * 11 * f, true, 4},
                   {px * 12 * f, true, 4},
                   {px * 15 * f, true, 4},
                   {px * 16 * f, want(m, 2) != nullptr, 4},
                   {px * 19 * f, want(m, 3) != nullptr, 4},
                   {px * 20 * f, want(m, 4) != nullptr, 4},
                   {align16(plane_bytes), want(m, 0) != nullptr, 16},
                   {align16(plane_bytes) + px * kHistory, true, 16}},
                  align16(plane_bytes) + 2 * px * kHistory);
        }
}

// The device form: the caller's pointers are device memory and reach the launch as they are, the block keeps the planes' room and
// none for the histories
void temporal_accum_device() {
    for (size_t px : kPixels) {
        char mine[4];
        Layout st(4, false);
        for (size_t bytes : {12, 12, 16, 4, 4}) st.kept(px * bytes);
        const int integrated = st.kept(px * 12, &mine[0]), variance = st.kept(px * 4);
        const int rgb = st.out(px * 12, &mine[1]), rgba = st.out(px * 4, nullptr);
        st.out(px * 4, nullptr);
        const int hin = st.in(0, nullptr), hout = st.out(0, &mine[2]);
        st.base = kBase;
        ++g_cases;
        const std::string cse = frame_case(px, 0);
        if (st.total != px * 21 * sizeof(float)) fail("vrt_accum_resolve_hdr_temporal_device", cse, "total " + std::to_string(st.total));
        if (st.at<char>(integrated) != &mine[0] || st.at<char>(rgb) != &mine[1] || st.at<char>(hout) != &mine[2])
            fail("vrt_accum_resolve_hdr_temporal_device", cse, "a caller's device pointer does not reach the launch");
        if (st.at(rgba) || st.at(hin)) fail("vrt_accum_resolve_hdr_temporal_device", cse, "a plane not asked for is not null");
        if (st.at<char>(variance) != kBase + px * 15 * sizeof(float)) fail("vrt_accum_resolve_hdr_temporal_device", cse, "the variance plane is not the block's");
    }
}

// device memory of the context's own (the separate images: c->d_rgba, Accum::d_hrgb, ...) takes no room in a block
void fixed_planes() {
    char image[2];
    Layout st(4);
    const int a = st.out(400, &g_host, &image[0]), b = st.out(800, nullptr, &image[1]);
    ++g_cases;
    if (st.total != 0) fail("separate images", "2 planes", "they take room");
    if (st.at<char>(a) != &image[0] || st.at(b)) fail("separate images", "2 planes", "wrong pointer for the launch");
}

}  // namespace

int main() {
    struct Row { const char *name; void (*run)(); };
    const Row rows[] = {{"cast_rays", cast_rays}, {"find_voxels", find_voxels}, {"shade_rays", shade_rays}, {"shade_rays_hdr", shade_rays_hdr},
                        {"guide_rays", guide_rays}, {"accum_guides", accum_guides},
                        {"filter_host", [] { filter(false, true); }}, {"filter_var_host", [] { filter(true, true); }},
                        {"filter_accum", [] { filter(false, false); }}, {"filter_var_accum", [] { filter(true, false); }},
                        {"temporal_host", temporal_host}, {"temporal_accum", temporal_accum}, {"temporal_accum_device", temporal_accum_device},
                        {"fixed_planes", fixed_planes}};
    for (const Row &r : rows) {
        const long before = g_cases;
        r.run();
        std::printf("%s %ld\n", r.name, g_cases - before);
    }
    return 0;
}
