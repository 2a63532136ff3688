// psxhip_ingest.cpp -- host side of the picture ingest (psxhip_ingest_*; include/psxav_hip.h): the handle, the
// entry points' staging and launches (ingest_kernels.hip).  The source's rules, the matrix in exact integers, the conversions'
// argument rules and the planners that need no device are picture_plan.h's.  No pixel is touched on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "device_buffer.h"
#include "picture_plan.h"
#include "psxhip_ingest_internal.h"
#include "psxhip_internal.h"

struct psxhip_ingest {
    int device;
    IngestPlan p;
};

extern "C" const char* psxhip_ingest_kernel_rev(void) { return PSXHIP_INGEST_KERNEL_REV; }

extern "C" void psxhip_ingest_destroy(psxhip_ingest_t* g) { delete g; }

extern "C" int psxhip_ingest_create(psxhip_ingest_t** out, int device, int src_format, int width, int height,
                                    const psxhip_ingest_plane_t* planes, int n_planes, int matrix, int full_range, int out_format,
                                    uint32_t options) {
    if (!out) return picture_bad("psxhip_ingest_create", "NULL argument");
    *out = nullptr;
    IngestPlan p;
    const int rc = ingest_create_plan(src_format, width, height, planes, n_planes, matrix, full_range, out_format, options, &p);
    if (rc) return rc;
    psxhip_ingest* g = new (std::nothrow) psxhip_ingest;
    if (!g) return PSXHIP_ENOMEM;
    g->device = device; g->p = p;
    *out = g;
    return PSXHIP_OK;
}

extern "C" size_t psxhip_ingest_output_bytes(const psxhip_ingest_t* g) { return g ? g->p.out_bytes : 0; }
extern "C" size_t psxhip_ingest_source_bytes(const psxhip_ingest_t* g) { return g ? g->p.src_bytes : 0; }

extern "C" int psxhip_ingest_matrix(const psxhip_ingest_t* g, int32_t out[7]) {
    if (!g || !out) return picture_bad("psxhip_ingest_matrix", "NULL argument");
    const IngestDesc& d = g->p.d;
    const int32_t m[7] = {d.cy, d.rv, d.gu, d.gv, d.bu, d.yoff, d.coff};
    for (int i = 0; i < 7; i++) out[i] = m[i];
    return PSXHIP_OK;
}

static psxhip_ingest_job_t job_of(const psxhip_ingest_t* g, const uint8_t* d_src, size_t src_stride, int n_src, const int32_t* d_src_index,
                                  int n_out, uint8_t* d_out, size_t out_stride) {
    psxhip_ingest_job_t j;
    j.d = g->p.d; j.d_src = d_src; j.src_stride = src_stride; j.n_src = n_src; j.d_src_index = d_src_index; j.first = 0; j.n_out = n_out;
    j.d_out = d_out; j.out_stride = out_stride; j.out_format = g->p.out_format;
    return j;
}

// (no temporary memory: the kernel reads the caller's pictures and index and writes the caller's output)
extern "C" int psxhip_ingest_convert_device(psxhip_ingest_t* g, const uint8_t* d_src, size_t src_stride, int n_src, const int32_t* d_src_index,
                                            int n_out, uint8_t* d_out, size_t out_stride, void* stream) {
    bool go;
    int rc = ingest_check("psxhip_ingest_convert_device", g ? &g->p : nullptr, (uintptr_t)d_src, src_stride, n_src, n_out, (uintptr_t)d_out, out_stride, true, &go);
    if (rc || !go) return rc;
    if ((rc = psxhip_ensure_device(g->device))) return rc;
    HIP_TRY(hipSetDevice(g->device), PSXHIP_EDEVICE);
    const psxhip_ingest_job_t j = job_of(g, d_src, src_stride, n_src, d_src_index, n_out, d_out, out_stride);
    HIP_TRY(psxhip_ingest_launch(&j, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_ingest_convert_host(psxhip_ingest_t* g, const uint8_t* src, size_t src_stride, int n_src, const int32_t* src_index,
                                          int n_out, uint8_t* out, size_t out_stride) {
    bool go;
    int rc = ingest_check("psxhip_ingest_convert_host", g ? &g->p : nullptr, (uintptr_t)src, src_stride, n_src, n_out, (uintptr_t)out, out_stride, false, &go);
    if (rc || !go) return rc;
    if ((rc = psxhip_ensure_device(g->device))) return rc;
    HIP_TRY(hipSetDevice(g->device), PSXHIP_EDEVICE);
    const size_t src_bytes = (size_t)(n_src - 1) * src_stride + g->p.src_bytes, out_bytes = (size_t)(n_out - 1) * out_stride + g->p.out_bytes;
    DeviceBuffer d_src, d_out, d_index;                  // a call's temporaries
    if ((rc = d_src.reserve(src_bytes)) || (rc = d_out.reserve(out_bytes)) || (src_index && (rc = d_index.reserve((size_t)n_out * sizeof(int32_t))))) return rc;
    HIP_TRY(hipMemcpy(d_src.p, src, src_bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    // the output goes up as well: what the kernel does not write (between pictures, pictures of negative indices) comes back as it was
    HIP_TRY(hipMemcpy(d_out.p, out, out_bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    if (src_index) HIP_TRY(hipMemcpy(d_index.p, src_index, (size_t)n_out * sizeof(int32_t), hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    const psxhip_ingest_job_t j = job_of(g, d_src.as<uint8_t>(), src_stride, n_src, src_index ? d_index.as<int32_t>() : nullptr, n_out,
                                         d_out.as<uint8_t>(), out_stride);
    HIP_TRY(psxhip_ingest_launch(&j, nullptr), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost), PSXHIP_EDEVICE);
    HIP_TRY(hipDeviceSynchronize(), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}
