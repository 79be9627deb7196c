// device_arena.h — one owner for the device buffers of a context.  Call sites keep plain T* (modules and kernels borrow
// them); the arena remembers every block it handed out, so a new buffer is freed without being named anywhere else.  The
// owner calls free_all() once, after whatever borrows the buffers has gone and before the context is destroyed; on a
// half-built object that frees exactly what exists.
#pragma once
#include <algorithm>
#include <vector>
#include "hip_check.h"

class DeviceArena {
    gcnhip_ctx *ctx_ = nullptr;
    std::vector<void *> blocks_;
public:
    DeviceArena() = default;
    DeviceArena(const DeviceArena &) = delete;
    DeviceArena &operator=(const DeviceArena &) = delete;
    void bind(gcnhip_ctx *ctx) { ctx_ = ctx; }

    template <class T>
    T *alloc(size_t n) {                                       // n elements exactly: floors and paddings are the caller's
        blocks_.reserve(blocks_.size() + 1);                   // (so that recording the block cannot throw)
        void *p = nullptr;
        GCNHIP_CHECK(gcnhip_malloc(ctx_, &p, n * sizeof(T)));
        blocks_.push_back(p);
        return (T *)p;
    }
    template <class T>
    T *alloc_zeroed(size_t n) {                                // the memset is enqueued on the context's stream
        T *p = alloc<T>(n);
        GCNHIP_CHECK(gcnhip_memset_async(ctx_, p, 0, n * sizeof(T)));
        return p;
    }
    template <class T>
    T *upload(const T *h, size_t n) {                          // h[0..n) (one element when n == 0); gcnhip_h2d synchronises
        T *p = alloc<T>(n ? n : 1);
        if (n) GCNHIP_CHECK(gcnhip_h2d(ctx_, p, h, n * sizeof(T)));
        return p;
    }
    void release(void *p) {                                    // give one block back early (NULL: nothing)
        auto it = std::find(blocks_.begin(), blocks_.end(), p);
        if (!p || it == blocks_.end()) return;
        gcnhip_free(ctx_, p);
        blocks_.erase(it);
    }
    template <class T>
    void regrow(T *&p, size_t n) {                             // scratch that grows: the old block goes, p names a new one (contents not kept)
        release(p);
        p = nullptr;
        p = alloc<T>(n);
    }
    void free_all() {
        for (void *p : blocks_) gcnhip_free(ctx_, p);
        blocks_.clear();
    }
};
