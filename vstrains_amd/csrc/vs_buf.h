// The one owner of device and pinned host memory: a move-only, grow-only buffer.  Every allocation of the library is made
// and freed here (the exception: vs_dev_alloc / vs_dev_free, which hand the caller a raw pointer).  Host code only, and
// nothing but the runtime's API header, so that a CPU test can instantiate the template with an allocator of its own.
//
// What holds after EVERY call, a failed one included: ptr() == nullptr exactly when capacity() == 0.
// What the type does not do: no stream, no synchronisation, no fill, no rounding, no pooling.  Whoever regrows a buffer
// that the device may still use synchronises first.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stddef.h>

template <class Alloc>
struct VsBuf {
    VsBuf() = default;
    VsBuf(const VsBuf &) = delete;
    VsBuf &operator=(const VsBuf &) = delete;
    VsBuf(VsBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    VsBuf &operator=(VsBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, cap_ = o.cap_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~VsBuf() { reset(); }

    void *ptr() const { return p_; }
    size_t capacity() const { return cap_; }  // bytes
    template <class T>
    T *as() const { return (T *)p_; }

    void reset() {
        if (p_) Alloc::free(p_);
        p_ = nullptr, cap_ = 0;
    }
    // At least `need` bytes: nothing happens while capacity() >= need; otherwise the old block is freed FIRST (the two are
    // never held at once, and the contents are not kept) and one of `alloc` >= need bytes (0 = need: no slack) is made.
    // *fresh, if given: whether this call allocated.  On failure the buffer is empty and the error is returned.
    hipError_t reserve(size_t need, size_t alloc = 0, bool *fresh = nullptr) {
        if (fresh) *fresh = false;
        if (cap_ >= need) return hipSuccess;
        reset();
        if (alloc < need) alloc = need;
        void *q = nullptr;
        const hipError_t e = Alloc::alloc(&q, alloc);  // (a failed hipMalloc leaves its out-pointer as it was: q is not trusted then)
        if (e != hipSuccess) return e;
        if (!q) return hipErrorOutOfMemory;
        p_ = q, cap_ = alloc;
        if (fresh) *fresh = true;
        return hipSuccess;
    }
    // hand the block to someone else: the buffer is empty afterwards and frees nothing
    void *release() {
        void *q = p_;
        p_ = nullptr, cap_ = 0;
        return q;
    }
    // take over a block of `bytes` bytes that came from the same allocator
    void adopt(void *p, size_t bytes) {
        reset();
        if (p && bytes) p_ = p, cap_ = bytes;
    }

private:
    void *p_ = nullptr;
    size_t cap_ = 0;
};

struct VsDevAlloc {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void *p) { (void)hipFree(p); }
};
struct VsPinnedAlloc {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void *p) { (void)hipHostFree(p); }
};
using VsDevBuf = VsBuf<VsDevAlloc>;
using VsPinnedBuf = VsBuf<VsPinnedAlloc>;
