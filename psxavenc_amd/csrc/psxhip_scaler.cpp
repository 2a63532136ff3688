// psxhip_scaler.cpp -- the scaler's C ABI (include/psxav_hip.h, psxhip_scaler_*): the handle, its device
// tables and the launches.  What a call's arguments decide -- the refusals, the filter banks, the tile and its LDS size, the segments
// -- is picture_plan.h's; the kernel is frontend_kernels.hip; no pixel is touched on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <cstring>
#include <new>

#include "device_buffer.h"
#include "picture_plan.h"
#include "psxhip_internal.h"

struct psxhip_scaler {
    int device, fmt, sw, sh, full_range, dw, dh;
    HostBank h[4];                 // lh, lv, ch, cv
    DeviceBuffer d_left[4], d_coef[4], d_digits[4];      // ... and their tables on the device
    psxhip_scaler_job_t job;
    size_t lds_bytes;
    size_t src_bytes;              // bytes of one source picture
    int n_cus;
};

extern "C" void psxhip_scaler_destroy(psxhip_scaler_t* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

extern "C" int psxhip_scaler_create(psxhip_scaler_t** out, int device, int src_format, int src_width, int src_height,
                                    int src_full_range, int dst_width, int dst_height) {
    if (!out) return PSXHIP_EINVAL;
    *out = nullptr;
    int rc = scaler_geometry_check(src_format, src_width, src_height, dst_width, dst_height);
    if (rc) return rc;
    const bool yuv = src_format == PSXHIP_PIX_YUV420P;
    rc = psxhip_ensure_device(device);
    if (rc) return rc;
    psxhip_scaler* s = new (std::nothrow) psxhip_scaler;
    if (!s) return PSXHIP_ENOMEM;
    struct Guard { psxhip_scaler* p; ~Guard() { if (p) psxhip_scaler_destroy(p); } } guard{s};
    s->device = device; s->fmt = src_format; s->sw = src_width; s->sh = src_height; s->full_range = src_full_range;
    s->dw = dst_width; s->dh = dst_height;
    const int csw = yuv ? src_width / 2 : src_width, csh = yuv ? src_height / 2 : src_height;
    if ((rc = scaler_design_banks(src_format, src_width, src_height, dst_width, dst_height, s->h))) return rc;
    s->src_bytes = yuv ? (size_t)src_width * src_height * 3 / 2 : (size_t)src_width * src_height * 3;
    psxhip_scaler_job_t& j = s->job;
    memset(&j, 0, sizeof j);
    j.sw = src_width; j.sh = src_height; j.dw = dst_width; j.dh = dst_height;
    j.csw = csw; j.csh = csh;
    j.limited = yuv && !src_full_range;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device), PSXHIP_EDEVICE);
    s->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if ((rc = scaler_choose_tile(s->h, yuv, dst_width, dst_height, (size_t)prop.maxSharedMemoryPerMultiProcessor, getenv("PSXHIP_SCALER_TILE"), &j,
                                 &s->lds_bytes)))
        return rc;
    psxhip_scaler_bank_t* banks[4] = {&j.lh, &j.lv, &j.ch, &j.cv};
    for (int i = 0; i < 4; i++) {
        const HostBank& h = s->h[i];
        const size_t left_bytes = h.left.size() * sizeof(int32_t), coef_bytes = h.coef.size() * sizeof(int16_t), digits_bytes = h.digits.size() * sizeof(uint32_t);
        if ((rc = s->d_left[i].reserve(left_bytes)) || (rc = s->d_coef[i].reserve(coef_bytes)) || (rc = s->d_digits[i].reserve(digits_bytes))) return rc;
        HIP_TRY(hipMemcpy(s->d_left[i].p, h.left.data(), left_bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
        HIP_TRY(hipMemcpy(s->d_coef[i].p, h.coef.data(), coef_bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
        HIP_TRY(hipMemcpy(s->d_digits[i].p, h.digits.data(), digits_bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
        banks[i]->left = s->d_left[i].as<int32_t>();
        banks[i]->coef = s->d_coef[i].as<int16_t>();
        banks[i]->digits = s->d_digits[i].as<uint32_t>();
    }
    HIP_TRY(psxhip_scaler_prepare(yuv, (int)prop.maxSharedMemoryPerMultiProcessor), PSXHIP_EDEVICE);
    guard.p = nullptr;
    *out = s;
    return PSXHIP_OK;
}

extern "C" size_t psxhip_scaler_source_bytes(const psxhip_scaler_t* s) { return s ? s->src_bytes : 0; }

extern "C" int psxhip_scaler_filter(const psxhip_scaler_t* s, int which, int* taps, int32_t* left, int16_t* coef, int cap) {
    if (!s || which < 0 || which > 3) return PSXHIP_EINVAL;
    const HostBank& b = s->h[which];
    if (taps) *taps = b.taps;
    const int n = (int)b.left.size();
    if (left && coef) {
        if (cap < n * b.taps) return PSXHIP_EINVAL;
        memcpy(left, b.left.data(), (size_t)n * sizeof(int32_t));
        memcpy(coef, b.coef.data(), (size_t)n * b.taps * sizeof(int16_t));
    }
    return n;
}

extern "C" int psxhip_scaler_convert_device(psxhip_scaler_t* s, const uint8_t* d_src, size_t src_stride, int n_frames,
                                            uint8_t* d_frames, size_t frame_stride, void* stream) {
    bool go;
    const int rc = scaler_convert_check("psxhip_scaler_convert_device", s != nullptr, (uintptr_t)d_src, (uintptr_t)d_frames, n_frames, true, src_stride,
                                        frame_stride, s ? s->src_bytes : 0, s ? s->dw : 0, s ? s->dh : 0, &go);
    if (rc || !go) return rc;
    HIP_TRY(hipSetDevice(s->device), PSXHIP_EDEVICE);
    psxhip_scaler_job_t j = s->job;
    j.src = d_src; j.src_stride = src_stride; j.out = d_frames; j.frame_stride = frame_stride;
    j.vsegs = scaler_vsegs(s->n_cus, j.tiles_x, j.tiles_y, n_frames, getenv("PSXHIP_SCALER_VSEGS"));
    for (int f0 = 0; f0 < n_frames; f0 += kScalerLaunchFrames) {
        const int nf = scaler_launch_frames(n_frames, f0);
        j.src = d_src + (size_t)f0 * src_stride;
        j.out = d_frames + (size_t)f0 * frame_stride;
        HIP_TRY(psxhip_scaler_launch(&j, s->fmt == PSXHIP_PIX_YUV420P, nf, s->lds_bytes, stream), PSXHIP_EDEVICE);
    }
    return PSXHIP_OK;
}

extern "C" int psxhip_scaler_convert_host(psxhip_scaler_t* s, const uint8_t* src, int n_frames, uint8_t* frames) {
    bool go;
    int rc = scaler_convert_check("psxhip_scaler_convert_host", s != nullptr, (uintptr_t)src, (uintptr_t)frames, n_frames, false, 0, 0, 0, 0, 0, &go);
    if (rc || !go) return rc;
    HIP_TRY(hipSetDevice(s->device), PSXHIP_EDEVICE);
    const size_t fsz = (size_t)s->dw * s->dh * 3 / 2;
    DeviceBuffer d_src, d_out;
    if ((rc = d_src.reserve(s->src_bytes * (size_t)n_frames)) || (rc = d_out.reserve(fsz * (size_t)n_frames))) return rc;
    HIP_TRY(hipMemcpy(d_src.p, src, s->src_bytes * (size_t)n_frames, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    rc = psxhip_scaler_convert_device(s, d_src.as<uint8_t>(), s->src_bytes, n_frames, d_out.as<uint8_t>(), fsz, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(frames, d_out.p, fsz * (size_t)n_frames, hipMemcpyDeviceToHost), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}
