// psxhip_display.cpp -- host side of the display back-end (psxhip_display_*; include/psxav_hip.h): argument
// checks, the host entry's staging, the launches (display_kernels.hip).  The decode-and-display entry is psxhip_decode.cpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_buffer.h"
#include "display_core.h"
#include "psxhip_display_internal.h"
#include "psxhip_internal.h"

static_assert(DISP_RGB24 == PSXHIP_OUT_RGB24 && DISP_RGBX32 == PSXHIP_OUT_RGBX32 && DISP_RGB555 == PSXHIP_OUT_RGB555, "display_core.h restates the formats");
static_assert(DISP_CHROMA_BILINEAR == PSXHIP_DISPLAY_CHROMA_BILINEAR && DISP_DITHER == PSXHIP_DISPLAY_DITHER && DISP_MASK_BIT == PSXHIP_DISPLAY_MASK_BIT,
              "display_core.h restates the options");

extern "C" const char* psxhip_display_kernel_rev(void) { return PSXHIP_DISPLAY_KERNEL_REV; }

extern "C" size_t psxhip_display_row_bytes(int out_format, int width) {
    return width > 0 ? (size_t)disp_row_bytes(out_format, width) : 0;
}

int psxhip_display_check(const char* who, const psxhip_display_job_t* j, bool device_pointers) {
    if (j->n_frames < 0 || (j->n_frames > 0 && (!j->d_frames || !j->d_dst))) {
        psxhip_set_error("%s: NULL argument or negative frame count", who);
        return PSXHIP_EINVAL;
    }
    if (j->width < 16 || j->height < 16 || j->width > 1024 || j->height > 1024 || (j->width & 15) || (j->height & 15)) {
        psxhip_set_error("%s: %dx%d is not a multiple of 16 in 16 .. 1024", who, j->width, j->height);
        return PSXHIP_EINVAL;
    }
    const size_t row = psxhip_display_row_bytes(j->out_format, j->width);
    if (!row) {
        psxhip_set_error("%s: unknown out_format %d", who, j->out_format);
        return PSXHIP_EINVAL;
    }
    const uint32_t known = PSXHIP_DISPLAY_CHROMA_BILINEAR | PSXHIP_DISPLAY_DITHER | PSXHIP_DISPLAY_MASK_BIT;
    if ((j->options & ~known) ||
        (j->out_format != PSXHIP_OUT_RGB555 && (j->options & (PSXHIP_DISPLAY_DITHER | PSXHIP_DISPLAY_MASK_BIT)))) {
        psxhip_set_error("%s: options 0x%x: an unknown bit, or dither / mask bit with a format other than RGB555", who, (unsigned)j->options);
        return PSXHIP_EINVAL;
    }
    const size_t frame_bytes = (size_t)j->width * j->height * 3 / 2;
    if ((device_pointers && ((uintptr_t)j->d_frames & 3)) || (j->frame_stride & 3) || j->frame_stride < frame_bytes) {
        psxhip_set_error("%s: d_frames / frame_stride not 4-byte aligned, or frame_stride below %zu", who, frame_bytes);
        return PSXHIP_EINVAL;
    }
    const size_t picture = (size_t)(j->height - 1) * j->dst_pitch + row;
    if ((device_pointers && ((uintptr_t)j->d_dst & 3)) || (j->dst_pitch & 3) || (j->dst_stride & 3) || j->dst_pitch < row || j->dst_stride < picture) {
        psxhip_set_error("%s: d_dst / dst_pitch / dst_stride not 4-byte aligned, dst_pitch below %zu or dst_stride below %zu", who, row, picture);
        return PSXHIP_EINVAL;
    }
    if (device_pointers && j->n_frames > 0) {
        const uintptr_t src = (uintptr_t)j->d_frames, src_end = src + (size_t)(j->n_frames - 1) * j->frame_stride + frame_bytes;
        const uintptr_t dst = (uintptr_t)j->d_dst, dst_end = dst + (size_t)(j->n_frames - 1) * j->dst_stride + picture;
        if (src < dst_end && dst < src_end) {
            psxhip_set_error("%s: d_dst overlaps d_frames", who);
            return PSXHIP_EINVAL;
        }
    }
    return PSXHIP_OK;
}

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
