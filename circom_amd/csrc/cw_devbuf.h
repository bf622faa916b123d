// cw_devbuf.h — DevBuf<T>: the one owner of a device allocation.  Move-only; frees what it holds when it is reset,
// re-allocated or destroyed, and converts to T* wherever a kernel wrapper or a HIP call takes the pointer.
// The allocator is named through two macros so that tests/host/devbuf_test.cpp can count calls without a HIP runtime:
// with both predefined no HIP header is read (the test then supplies hipError_t / hipSuccess itself).
#pragma once
#include <cstddef>

#if !defined(CW_DEVBUF_MALLOC) || !defined(CW_DEVBUF_FREE)
#include <hip/hip_runtime_api.h>
#endif
#ifndef CW_DEVBUF_MALLOC
#define CW_DEVBUF_MALLOC hipMalloc
#endif
#ifndef CW_DEVBUF_FREE
#define CW_DEVBUF_FREE hipFree
#endif

template <typename T>
class DevBuf {
    T *p_ = nullptr;
    size_t cap_ = 0;                                   // bytes held
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p_) (void)CW_DEVBUF_FREE(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    hipError_t alloc(size_t bytes) {                   // what was held goes first; after a failure the holder is empty
        reset();
        void *q = nullptr;
        hipError_t e = CW_DEVBUF_MALLOC(&q, bytes);
        if (e == hipSuccess) { p_ = static_cast<T *>(q); cap_ = bytes; }
        return e;
    }
    hipError_t grow(size_t bytes) { return p_ && bytes <= cap_ ? hipSuccess : alloc(bytes); }   // contents are NOT kept
    operator T *() const { return p_; }
    T *get() const { return p_; }                      // for casts to another pointer type
};
