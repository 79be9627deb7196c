// devbuf.h — one owner for a device block of libgcnhip.so.  Reads keep plain T* (kernel arguments, `if (f->keep_bits)`);
// the block goes with its object, so a new buffer is freed without being named in a destroy function.  The device of the
// owning context must be current when a DevBuf is filled or dies (the destroy entry points make it so before `delete`).
// Every hipMalloc / hipFree of the library is in this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

inline hipError_t dev_malloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t dev_free(void *p) { return hipFree(p); }

template <class T>
class DevBuf {
    T *p_ = nullptr;
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;                           // so the compiler proves that no object is copied by value
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
    ~DevBuf() { reset(); }
    operator T *() const { return p_; }
    void reset() { if (p_) dev_free(p_); p_ = nullptr; }
    // each returns HIP's error code, for GCNHIP_TRY; the old block goes first, contents are not kept
    hipError_t alloc(size_t n) {                               // n elements exactly: floors and paddings are the caller's
        reset();
        return dev_malloc((void **)&p_, n * sizeof(T));
    }
    hipError_t upload(const T *h, size_t n) { return fill(h, n, hipMemcpyHostToDevice); }      // h[0..n) (one element when n == 0)
    hipError_t copy_from(const T *d, size_t n) { return fill(d, n, hipMemcpyDeviceToDevice); } // the same from device memory
private:
    hipError_t fill(const T *src, size_t n, hipMemcpyKind kind) {
        const hipError_t e = alloc(n ? n : 1);
        return e != hipSuccess || n == 0 ? e : hipMemcpy(p_, src, n * sizeof(T), kind);
    }
};
