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

// The other things a handle owns, by the same rules (move-only, not part of the library's surface, never static): a page-locked host
// block, a stream, an event
template <class T, hipError_t (*Destroy)(T)>
struct __attribute__((visibility("hidden"))) HipOwned {
    T h = nullptr;

    HipOwned() = default;
    HipOwned(const HipOwned&) = delete;
    HipOwned& operator=(const HipOwned&) = delete;
    HipOwned(HipOwned&& o) noexcept : h(o.h) { o.h = nullptr; }
    HipOwned& operator=(HipOwned&& o) noexcept {
        if (this != &o) {
            release();
            h = o.h;
            o.h = nullptr;
        }
        return *this;
    }
    ~HipOwned() { release(); }

    void release() {
        if (h) (void)Destroy(h);
        h = nullptr;
    }
    operator T() const { return h; }
};
struct __attribute__((visibility("hidden"))) PinnedBlock : HipOwned<void*, hipHostFree> {
    // a new block of `bytes` (the old one is gone): hipHostMalloc's flags
    int alloc(size_t bytes, unsigned flags) {
        release();
        HIP_TRY(hipHostMalloc(&h, bytes, flags), PSXHIP_ENOMEM);
        return PSXHIP_OK;
    }
    uint8_t* bytes() const { return (uint8_t*)h; }
};
struct __attribute__((visibility("hidden"))) Stream : HipOwned<hipStream_t, hipStreamDestroy> {
    int ensure() {          // a non-blocking stream, created at first use
        if (!h) HIP_TRY(hipStreamCreateWithFlags(&h, hipStreamNonBlocking), PSXHIP_EDEVICE);
        return PSXHIP_OK;
    }
};
struct __attribute__((visibility("hidden"))) Event : HipOwned<hipEvent_t, hipEventDestroy> {
    int ensure() {          // an event without timing, created at first use
        if (!h) HIP_TRY(hipEventCreateWithFlags(&h, hipEventDisableTiming), PSXHIP_EDEVICE);
        return PSXHIP_OK;
    }
};
