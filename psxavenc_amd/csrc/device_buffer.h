// device_buffer.h -- the one owner of a block of device memory on the host layer: a handle's grow-on-demand buffers and a call's
// temporaries.  Move-only; freed by the destructor, so it is never a static or thread_local object (hipFree during thread or
// process teardown): the per-thread pools (ScratchPool, BlockCache) are policies of their own and keep their own blocks.
#pragma once
#include "psxhip_internal.h"

struct __attribute__((visibility("hidden"))) DeviceBuffer {      // (not part of the library's surface)
    void* p = nullptr;
    size_t cap = 0;

    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p; cap = o.cap;
            o.p = nullptr; o.cap = 0;
        }
        return *this;
    }
    ~DeviceBuffer() { release(); }

    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // a block of at least `need` bytes on the current device: the one it has when that is large enough (its contents stay), else a
    // new one (the old contents are gone).  On failure the buffer is empty and the error text is set.
    int reserve(size_t need) {
        if (need <= cap) return PSXHIP_OK;
        release();
        HIP_TRY(hipMalloc(&p, need), PSXHIP_ENOMEM);
        cap = need;
        return PSXHIP_OK;
    }
    template <class T> T* as() const { return (T*)p; }
};
