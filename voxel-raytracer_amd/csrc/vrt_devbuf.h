// vrt_devbuf.h -- DevBuf<T>: the one owner of device memory in the host code of libvrt_hip.so. Every buffer a context (vrt_internal.h)
// or a vrt_multi (vrt_multi.hip) keeps is a DevBuf member: freed by the destructor, grown by reserve() and by nothing else.
//
// reserve() allocates the new block BEFORE the old one goes, so a failure leaves the buffer as it was; contents are not carried over.
// It does not synchronise: what may still read or write the old block differs from buffer to buffer (the context's stream, any
// stream of the device, the slot's own stream, nothing), and the caller waits for exactly that in front of the call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

// the owner itself, untyped: what the helpers that grow several buffers together take
class DevMem {
public:
    DevMem() = default;
    DevMem(DevMem &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DevMem &operator=(DevMem &&o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
        return *this;
    }
    ~DevMem() { reset(); }
    // room for `bytes`: nothing when there is; else a new block, and only once that exists the old one is freed. *fresh (optional):
    // the block is a new one, whatever the caller keeps about its contents starts again
    hipError_t reserve(size_t bytes, bool *fresh = nullptr) {
        if (fresh) *fresh = false;
        if (bytes <= bytes_) return hipSuccess;
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return e;
        reset();
        p_ = q;
        bytes_ = bytes;
        if (fresh) *fresh = true;
        return hipSuccess;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    size_t bytes() const { return bytes_; }   // capacity

protected:
    void *p_ = nullptr;
    size_t bytes_ = 0;
};

// ... and its typed view. Converts to T* where a pointer is expected (kernel arguments, copies, pointer arithmetic); it cannot be
// copied, and nothing but reserve() / reset() / the destructor may allocate or free what it points at.
template <class T>
class DevBuf : public DevMem {
public:
    T *get() const { return static_cast<T *>(p_); }
    operator T *() const { return get(); }
};
