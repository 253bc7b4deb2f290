// vrt_stage.h -- the staging of every entry point that takes host buffers: which planes a call keeps on the device, where each lies
// in the block it stages through, which of them come from the caller and which go back. A call declares its planes once, in the
// order they lie in; the size of the block, each plane's pointer and the copies all come from that one declaration.
//
// The first part is arithmetic on size_t and pointers and nothing else (tests/stage_layout_main.cpp compiles it alone, with
// VRT_STAGE_LAYOUT_ONLY defined); the second is the three operations on a stream: reserve, copy up, copy down and wait.
#pragma once
#include <cassert>
#include <cstddef>

namespace vrt_stage {

inline size_t align_up(size_t b, size_t a) { return (b + a - 1) & ~(a - 1); }   // a: a power of two

// A plane's direction. kIn comes from the caller before the launch, kOut goes back after it; both are null for the launch when the
// caller's pointer is. kKept is device-only -- the launch always has it -- and goes back too where the caller asks for it.
enum Dir { kIn, kOut, kKept };

struct Plane {
    size_t bytes, offset;   // what the copies move; where the plane starts in the block
    Dir dir;
    void *user;             // the caller's buffer, or null
    void *fixed;            // device memory of the context's own that the plane lies in instead of the block, or null
};

// Planes one after another, each starting at the next multiple of `align` (which a call may raise between two planes). A plane of
// zero bytes takes no room: the batch forms give an output that was not asked for zero bytes. The frame forms keep its room and
// only hand the launch a null pointer. With to_host false the caller's pointers are device memory: the launch gets them as they
// are -- a kept plane the block's where there is none -- and nothing is copied.
struct Layout {
    static constexpr int kMaxPlanes = 12;
    size_t align, total = 0;
    bool to_host;
    int n = 0;
    Plane plane[kMaxPlanes];
    char *base = nullptr;   // the block, once there is one

    explicit Layout(size_t align_, bool to_host_ = true) : align(align_), to_host(to_host_) {}
    // -> the plane's index, for at()
    int add(Dir dir, size_t bytes, const void *user, void *fixed = nullptr) {
        assert(n < kMaxPlanes);
        const size_t offset = fixed ? 0 : align_up(total, align);
        if (!fixed) total = offset + bytes;
        plane[n] = Plane{bytes, offset, dir, const_cast<void *>(user), fixed};
        return n++;
    }
    int in(size_t bytes, const void *user, void *fixed = nullptr) { return add(kIn, bytes, user, fixed); }
    int out(size_t bytes, void *user, void *fixed = nullptr) { return add(kOut, bytes, user, fixed); }
    int kept(size_t bytes, void *user = nullptr) { return add(kKept, bytes, user); }
    // where the plane lies on the device, whether or not the launch gets it
    char *device(int i) const { return plane[i].fixed ? static_cast<char *>(plane[i].fixed) : base + plane[i].offset; }
    // the plane as the launch gets it
    template <class T = void>
    T *at(int i) const {
        const Plane &p = plane[i];
        void *const block = device(i);
        if (!to_host) return static_cast<T *>(p.user || p.dir != kKept ? p.user : block);
        return static_cast<T *>(p.user || p.dir == kKept ? block : nullptr);
    }
};

}  // namespace vrt_stage

#ifndef VRT_STAGE_LAYOUT_ONLY
#include "vrt_internal.h"

namespace vrt_stage {

// ... and its transfers, each on the stream given and in the order the planes were declared
struct Stage : Layout {
    using Layout::Layout;
    // room for the block in `buf`, which only work on the context's stream touches: by reserve_staging's 1.5 x rule, or exactly
    template <class T>
    int reserve_staging(vrt_ctx *c, DevBuf<T> &buf) { return bind(buf, vrt_internal::reserve_staging(c, buf, total)); }
    template <class T>
    int reserve_synced(vrt_ctx *c, DevBuf<T> &buf) {
        return bind(buf, total <= buf.bytes() ? VRT_OK : vrt_internal::reserve_synced(c, {{&buf, total}}));
    }
    template <class T>
    int bind(const DevBuf<T> &buf, int r) {
        base = static_cast<char *>(static_cast<void *>(buf.get()));
        return r;
    }
    int upload(vrt_ctx *c, hipStream_t s) const {
        for (int i = 0; to_host && i < n; ++i)
            if (plane[i].dir == kIn && plane[i].user)
                VRT_HIP(c, hipMemcpyAsync(device(i), plane[i].user, plane[i].bytes, hipMemcpyHostToDevice, s));
        return VRT_OK;
    }
    // ... and the wait for the stream: the caller's buffers hold the outputs when this returns
    int download(vrt_ctx *c, hipStream_t s) const {
        if (!to_host) return VRT_OK;
        for (int i = 0; i < n; ++i)
            if (plane[i].dir != kIn && plane[i].user)
                VRT_HIP(c, hipMemcpyAsync(plane[i].user, device(i), plane[i].bytes, hipMemcpyDeviceToHost, s));
        VRT_HIP(c, hipStreamSynchronize(s));
        return VRT_OK;
    }
};

}  // namespace vrt_stage
#endif
