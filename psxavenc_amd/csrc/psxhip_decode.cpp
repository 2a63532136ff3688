// psxhip_decode.cpp -- host side of the MDEC decoder (psxhip_mdec_decoder_*, psxhip_mdec_decode_frames_*, psxhip_mdec_sse_device;
// include/psxav_hip.h): argument checks, the context's workspace and staging buffers, the launches
// (mdec_decode_kernels.hip); and psxhip_mdec_decode_display_device, the decoder followed by the display back-end (section 18).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "device_buffer.h"
#include "host_layout.h"
#include "psxhip_decode_internal.h"
#include "psxhip_display_internal.h"
#include "psxhip_internal.h"

struct psxhip_mdec_decoder {
    int device, width, height, nblk, wrap;
    DeviceBuffer ws;                  // levels of a call that wants pixels only
    DeviceBuffer nv21;                // decode_display_device: the frames between the reconstruction and the conversion
    DeviceBuffer stage;               // decode_frames_host: bitstreams, sizes, results, pixels
    DeviceBuffer stage_levels;
};

extern "C" const char* psxhip_mdec_decode_kernel_rev(void) { return PSXHIP_MDEC_DECODE_KERNEL_REV; }

extern "C" void psxhip_mdec_decoder_destroy(psxhip_mdec_decoder_t* dec) {
    if (!dec) return;
    (void)hipSetDevice(dec->device);
    delete dec;
}

extern "C" int psxhip_mdec_decoder_create(psxhip_mdec_decoder_t** out, int device, int width, int height, int dc_wrap) {
    if (!out) return PSXHIP_EINVAL;
    *out = nullptr;
    if (width < 16 || height < 16 || width > 1024 || height > 1024 || (width & 15) || (height & 15)) {
        psxhip_set_error("psxhip_mdec_decoder_create: %dx%d is not a multiple of 16 in 16 .. 1024", width, height);
        return PSXHIP_EINVAL;
    }
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    psxhip_mdec_decoder* d = new (std::nothrow) psxhip_mdec_decoder;
    if (!d) return PSXHIP_ENOMEM;
    d->device = device;
    d->width = width;
    d->height = height;
    d->nblk = (width / 16) * (height / 16) * 6;
    d->wrap = dc_wrap != 0;
    *out = d;
    return PSXHIP_OK;
}

extern "C" int psxhip_mdec_decode_frames_device(psxhip_mdec_decoder_t* dec, const uint8_t* d_bs, size_t bs_stride,
                                                const int32_t* d_bs_sizes, int uniform_size, int n_frames, int16_t* d_levels,
                                                uint8_t* d_frames, size_t frame_stride, psxhip_mdec_decoded_t* d_decoded,
                                                void* stream) {
    if (!dec || n_frames < 0 || (n_frames > 0 && (!d_bs || !d_decoded))) {
        psxhip_set_error("psxhip_mdec_decode_frames_device: NULL argument or negative frame count");
        return PSXHIP_EINVAL;
    }
    if (((uintptr_t)d_bs & 3) || (bs_stride & 3) || (!d_bs_sizes && (uniform_size < 0 || (size_t)uniform_size > bs_stride))) {
        psxhip_set_error("psxhip_mdec_decode_frames_device: d_bs / bs_stride not 4-byte aligned, or uniform_size %d outside 0 .. bs_stride",
                         uniform_size);
        return PSXHIP_EINVAL;
    }
    const size_t frame_bytes = (size_t)dec->width * dec->height * 3 / 2;
    if (d_frames && (((uintptr_t)d_frames & 3) || (frame_stride & 3) || frame_stride < frame_bytes)) {
        psxhip_set_error("psxhip_mdec_decode_frames_device: d_frames / frame_stride not 4-byte aligned, or frame_stride below %zu", frame_bytes);
        return PSXHIP_EINVAL;
    }
    if (d_levels && ((uintptr_t)d_levels & 1)) {
        psxhip_set_error("psxhip_mdec_decode_frames_device: d_levels is not 2-byte aligned");
        return PSXHIP_EINVAL;
    }
    if (n_frames == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(dec->device), PSXHIP_EDEVICE);
    int16_t* levels = d_levels;
    if (!levels && d_frames) {
        const int rc = dec->ws.reserve((size_t)n_frames * dec->nblk * 64 * sizeof(int16_t));
        if (rc) return rc;
        levels = dec->ws.as<int16_t>();
    }
    psxhip_mdec_parse_job_t pj;
    pj.d_bs = d_bs; pj.bs_stride = bs_stride; pj.d_sizes = d_bs_sizes; pj.uniform_size = uniform_size;
    pj.n_frames = n_frames; pj.nblk = dec->nblk; pj.wrap = dec->wrap; pj.d_levels = levels; pj.d_decoded = d_decoded;
    HIP_TRY(psxhip_mdec_parse_launch(&pj, stream), PSXHIP_EDEVICE);
    if (d_frames) {
        psxhip_mdec_recon_job_t rj;
        rj.d_levels = levels; rj.d_decoded = d_decoded; rj.d_frames = d_frames; rj.frame_stride = frame_stride;
        rj.n_frames = n_frames; rj.width = dec->width; rj.height = dec->height;
        HIP_TRY(psxhip_mdec_reconstruct_launch(&rj, stream), PSXHIP_EDEVICE);
    }
    return PSXHIP_OK;
}

extern "C" int psxhip_mdec_decode_display_device(psxhip_mdec_decoder_t* dec, const uint8_t* d_bs, size_t bs_stride,
                                                 const int32_t* d_bs_sizes, int uniform_size, int n_frames,
                                                 psxhip_mdec_decoded_t* d_decoded, int out_format, uint32_t options, uint8_t* d_dst,
                                                 size_t dst_pitch, size_t dst_stride, void* stream) {
    if (!dec || n_frames < 0 || (n_frames > 0 && (!d_bs || !d_decoded || !d_dst))) {
        psxhip_set_error("psxhip_mdec_decode_display_device: NULL argument or negative frame count");
        return PSXHIP_EINVAL;
    }
    psxhip_display_job_t j;
    j.frame_stride = (size_t)dec->width * dec->height * 3 / 2;
    j.d_decoded = d_decoded; j.d_dst = d_dst; j.dst_pitch = dst_pitch; j.dst_stride = dst_stride;
    j.width = dec->width; j.height = dec->height; j.n_frames = 0; j.out_format = out_format; j.options = options;
    j.d_frames = nullptr;                                // the workspace: reserved below, and no buffer of the caller's
    int rc = psxhip_display_check("psxhip_mdec_decode_display_device", &j, true);
    if (rc) return rc;
    if (n_frames == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(dec->device), PSXHIP_EDEVICE);
    if ((rc = dec->nv21.reserve((size_t)n_frames * j.frame_stride))) return rc;
    j.d_frames = dec->nv21.as<uint8_t>();
    j.n_frames = n_frames;
    // a frame that does not parse leaves its part of the workspace as it was, and the conversion skips it by the same record
    rc = psxhip_mdec_decode_frames_device(dec, d_bs, bs_stride, d_bs_sizes, uniform_size, n_frames, nullptr, dec->nv21.as<uint8_t>(),
                                          j.frame_stride, d_decoded, stream);
    if (rc) return rc;
    HIP_TRY(psxhip_display_launch(&j, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_mdec_decode_frames_host(psxhip_mdec_decoder_t* dec, const uint8_t* bs, size_t bs_stride, const int32_t* bs_sizes,
                                              int uniform_size, int n_frames, int16_t* levels, uint8_t* frames,
                                              psxhip_mdec_decoded_t* decoded) {
    if (!dec || n_frames < 0 || (n_frames > 0 && (!bs || !decoded))) {
        psxhip_set_error("psxhip_mdec_decode_frames_host: NULL argument or negative frame count");
        return PSXHIP_EINVAL;
    }
    if (!bs_sizes && (uniform_size < 0 || (size_t)uniform_size > bs_stride)) {
        psxhip_set_error("psxhip_mdec_decode_frames_host: uniform_size %d outside 0 .. bs_stride", uniform_size);
        return PSXHIP_EINVAL;
    }
    if (n_frames == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(dec->device), PSXHIP_EDEVICE);
    const size_t n = (size_t)n_frames;
    const size_t row = (bs_stride + 3) & ~(size_t)3;                 // device rows are 4-byte aligned whatever the host's stride
    const size_t frame_bytes = (size_t)dec->width * dec->height * 3 / 2;
    BumpOffsets o;
    o.take(n * row);
    const size_t off_sizes = o.take(n * sizeof(int32_t)), off_dec = o.take(n * sizeof(psxhip_mdec_decoded_t)), off_px = o.end;
    int rc = dec->stage.reserve(off_px + (frames ? n * frame_bytes : 0));
    if (rc) return rc;
    const size_t level_bytes = n * dec->nblk * 64 * sizeof(int16_t);
    if (levels && (rc = dec->stage_levels.reserve(level_bytes))) return rc;
    uint8_t* base = dec->stage.as<uint8_t>();
    int16_t* const d_levels = levels ? dec->stage_levels.as<int16_t>() : nullptr;
    if (row != bs_stride) HIP_TRY(hipMemset(base, 0, n * row), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpy2D(base, row, bs, bs_stride, bs_stride, n, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    if (bs_sizes) HIP_TRY(hipMemcpy(base + off_sizes, bs_sizes, n * sizeof(int32_t), hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    // a frame that does not parse leaves its pixels untouched: they start from the caller's
    if (frames) HIP_TRY(hipMemcpy(base + off_px, frames, n * frame_bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    rc = psxhip_mdec_decode_frames_device(dec, base, row, bs_sizes ? (const int32_t*)(base + off_sizes) : nullptr, uniform_size, n_frames,
                                          d_levels, frames ? base + off_px : nullptr, frame_bytes,
                                          (psxhip_mdec_decoded_t*)(base + off_dec), nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(decoded, base + off_dec, n * sizeof(psxhip_mdec_decoded_t), hipMemcpyDeviceToHost), PSXHIP_EDEVICE);
    if (levels) HIP_TRY(hipMemcpy(levels, d_levels, level_bytes, hipMemcpyDeviceToHost), PSXHIP_EDEVICE);
    if (frames) HIP_TRY(hipMemcpy(frames, base + off_px, n * frame_bytes, hipMemcpyDeviceToHost), PSXHIP_EDEVICE);
    HIP_TRY(hipDeviceSynchronize(), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_mdec_sse_device(int device, const uint8_t* d_a, const uint8_t* d_b, size_t frame_stride, int width, int height,
                                      int n_frames, uint64_t* d_sse, void* stream) {
    if (n_frames < 0 || (n_frames > 0 && (!d_a || !d_b || !d_sse))) {
        psxhip_set_error("psxhip_mdec_sse_device: NULL argument or negative frame count");
        return PSXHIP_EINVAL;
    }
    if (width < 16 || height < 16 || width > 1024 || height > 1024 || (width & 15) || (height & 15) || ((uintptr_t)d_a & 3) ||
        ((uintptr_t)d_b & 3) || ((uintptr_t)d_sse & 7) || (frame_stride & 3) || frame_stride < (size_t)width * height * 3 / 2) {
        psxhip_set_error("psxhip_mdec_sse_device: bad size %dx%d, misaligned pointer or frame_stride too small", width, height);
        return PSXHIP_EINVAL;
    }
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_frames == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    HIP_TRY(hipMemsetAsync(d_sse, 0, (size_t)n_frames * 3 * sizeof(uint64_t), (hipStream_t)stream), PSXHIP_EDEVICE);
    HIP_TRY(psxhip_mdec_sse_launch(d_a, d_b, frame_stride, width, height, n_frames, (unsigned long long*)d_sse, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}
