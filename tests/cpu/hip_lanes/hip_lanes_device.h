// tests/cpu/hip_lanes/hip_lanes_device.h -- TEST INFRASTRUCTURE, NOT HIP: a CPU "device" for the host layer of the reader modules
// (device_buffer.h and the psxhip_*.cpp files the lane programs include), part of the stand-in when HIP_LANES_WAVES is defined.
// Device memory is the heap, allocated at the exact size asked for, so the host sanitizers see the true end of every allocation;
// copies and fills happen at once; streams and events are inert handles; there is one device.
#pragma once
#include <stdlib.h>
#include <string.h>

enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3, hipMemcpyDefault = 4 };
constexpr hipError_t hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2;
enum { hipStreamNonBlocking = 1, hipEventDisableTiming = 2, hipHostMallocDefault = 0, hipHostMallocMapped = 2, hipHostMallocPortable = 1 };
enum hipDeviceAttribute_t { hipDeviceAttributeMultiprocessorCount = 63 };
typedef struct hip_lanes_event* hipEvent_t;

namespace hip_lanes {
inline uint64_t device_allocs = 0, device_frees = 0;
}

inline hipError_t hipMalloc(void** p, size_t bytes) {
    *p = malloc(bytes);
    hip_lanes::device_allocs++;
    return *p || !bytes ? hipSuccess : hipErrorOutOfMemory;
}
template <typename T> inline hipError_t hipMalloc(T** p, size_t bytes) { return hipMalloc((void**)p, bytes); }
inline hipError_t hipFree(void* p) {
    if (p) hip_lanes::device_frees++;
    free(p);
    return hipSuccess;
}
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned = 0) {
    *p = malloc(bytes);
    return *p || !bytes ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t hipHostFree(void* p) {
    free(p);
    return hipSuccess;
}
inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
    if (bytes) memcpy(dst, src, bytes);
    return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind k, hipStream_t = nullptr) { return hipMemcpy(dst, src, bytes, k); }
inline hipError_t hipMemcpy2D(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind) {
    if (width > dpitch || width > spitch) return hipErrorInvalidValue;
    for (size_t r = 0; r < height && width; r++) memcpy((char*)dst + r * dpitch, (const char*)src + r * spitch, width);
    return hipSuccess;
}
inline hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind k,
                                   hipStream_t = nullptr) {
    return hipMemcpy2D(dst, dpitch, src, spitch, width, height, k);
}
inline hipError_t hipMemset(void* dst, int value, size_t bytes) {
    if (bytes) memset(dst, value, bytes);
    return hipSuccess;
}
inline hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t = nullptr) { return hipMemset(dst, value, bytes); }
inline hipError_t hipMemcpyToSymbol(void* symbol, const void* src, size_t bytes, size_t offset = 0, hipMemcpyKind = hipMemcpyHostToDevice) {
    memcpy((char*)symbol + offset, src, bytes);
    return hipSuccess;
}
template <typename T>
inline hipError_t hipMemcpyToSymbol(T* symbol, const void* src, size_t bytes, size_t offset = 0, hipMemcpyKind k = hipMemcpyHostToDevice) {
    return hipMemcpyToSymbol((void*)symbol, src, bytes, offset, k);
}

inline hipError_t hipSetDevice(int device) { return device == 0 ? hipSuccess : hipErrorInvalidValue; }
inline hipError_t hipGetDevice(int* device) { *device = 0; return hipSuccess; }
inline hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
inline hipError_t hipDeviceGetAttribute(int* value, hipDeviceAttribute_t, int) { *value = 4; return hipSuccess; }      // (four "CUs")
inline hipError_t hipDeviceSynchronize() { return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = (hipStream_t)malloc(1); return hipSuccess; }
inline hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
inline hipError_t hipEventCreate(hipEvent_t* e) { *e = (hipEvent_t)malloc(1); return hipSuccess; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
inline hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t = nullptr) { return hipSuccess; }
inline hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.0f; return hipSuccess; }
