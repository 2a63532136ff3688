// psxhip_display.cpp -- host side of the display back-end (psxhip_display_*; include/psxav_hip.h): the host
// entry's staging, the launches (display_kernels.hip).  The argument rules (psxhip_display_check) and psxhip_display_row_bytes are
// picture_plan.cpp's.  The decode-and-display entry is psxhip_decode.cpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_buffer.h"
#include "psxhip_display_internal.h"
#include "psxhip_internal.h"

extern "C" const char* psxhip_display_kernel_rev(void) { return PSXHIP_DISPLAY_KERNEL_REV; }

extern "C" int psxhip_display_convert_device(int device, const uint8_t* d_frames, size_t frame_stride, int width, int height, int n_frames,
                                             const psxhip_mdec_decoded_t* d_decoded, int out_format, uint32_t options, uint8_t* d_dst,
                                             size_t dst_pitch, size_t dst_stride, void* stream) {
    psxhip_display_job_t j;
    j.d_frames = d_frames; j.frame_stride = frame_stride; j.d_decoded = d_decoded; j.d_dst = d_dst; j.dst_pitch = dst_pitch;
    j.dst_stride = dst_stride; j.width = width; j.height = height; j.n_frames = n_frames; j.out_format = out_format; j.options = options;
    int rc = psxhip_display_check("psxhip_display_convert_device", &j, true);
    if (rc) return rc;
    if ((rc = psxhip_ensure_device(device))) return rc;
    if (n_frames == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    HIP_TRY(psxhip_display_launch(&j, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_display_convert_host(int device, const uint8_t* frames, int width, int height, int n_frames, int out_format,
                                           uint32_t options, uint8_t* dst) {
    psxhip_display_job_t j;
    const size_t row = psxhip_display_row_bytes(out_format, width), rows = height > 0 ? (size_t)height : 0;
    j.d_frames = frames; j.frame_stride = (width > 0 ? (size_t)width : 0) * rows * 3 / 2; j.d_decoded = nullptr;
    j.d_dst = dst; j.dst_pitch = row; j.dst_stride = row * rows;                 // back to back
    j.width = width; j.height = height; j.n_frames = n_frames; j.out_format = out_format; j.options = options;
    int rc = psxhip_display_check("psxhip_display_convert_host", &j, false);     // host pointers: any alignment
    if (rc) return rc;
    if ((rc = psxhip_ensure_device(device))) return rc;
    if (n_frames == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    const size_t n = (size_t)n_frames;
    DeviceBuffer src, out;                               // a call's temporaries
    if ((rc = src.reserve(n * j.frame_stride)) || (rc = out.reserve(n * j.dst_stride))) return rc;
    j.d_frames = src.as<uint8_t>();
    j.d_dst = out.as<uint8_t>();
    HIP_TRY(hipMemcpy(src.p, frames, n * j.frame_stride, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    HIP_TRY(psxhip_display_launch(&j, nullptr), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpy(dst, out.p, n * j.dst_stride, hipMemcpyDeviceToHost), PSXHIP_EDEVICE);
    HIP_TRY(hipDeviceSynchronize(), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}
