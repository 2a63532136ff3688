// display_kernels.hip -- the display back-end's kernel for gfx950: NV21 frames -> RGB24 / RGBX32 / RGB555 ("psxhip display v1",
// DESIGN.md section 18; the arithmetic of one pixel is display_core.h, the text the CPU test runs).
//
// The conversion streams: 1.5 bytes read and 2 .. 4 written per pixel, a handful of integer operations in between, so the kernel is
// shaped by its memory accesses.  A lane owns 4 x 2 pixels: one chroma dword (two Cr/Cb pairs) and the two luma dwords above it, so
// a chroma row is read once for the two luma rows that share it.  It stores whole dwords -- three per row for RGB24, two (one
// dwordx2) for RGB555, four (one dwordx4) for RGBX32 -- and consecutive lanes take consecutive addresses along a row, so a
// wavefront's loads and stores are contiguous runs.  Bilinear chroma needs the chroma rows above and below and the samples left and
// right of the lane's dword: they come from extra loads of neighbouring dwords, which the lane's neighbours have fetched into the
// same cache lines (no cross-lane exchange: a lane's neighbour in x may sit in another wavefront, and the plane's edges clamp).
// Format and options are template parameters: no branch depends on a pixel.  No LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "display_core.h"
#include "psxhip_display_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxFramesPerLaunch = 65535;                     // gridDim.y

struct Dwords2 { uint32_t v[2]; };                             // (alignment 4: a row starts on a dword, not more)
struct Dwords3 { uint32_t v[3]; };
struct Dwords4 { uint32_t v[4]; };

// Cr and Cb of the lane's four pixels: the bytes, or a chroma row's horizontal mixes (disp_hmix: four times a byte's scale)
struct Chroma4 {
    int cr[4], cb[4];
};

__device__ __forceinline__ int byte_of(uint32_t w, int i) { return (int)((w >> (8 * i)) & 255u); }

// b0 | b1 << 8 | b2 << 16 | b3 << 24 of four values in 0 .. 255, by two byte permutes and an or.  Not by shifts and ors of the clamped
// values: hipcc of ROCm 7 turns `clamp(a >> 16, 0, 255) | clamp(b >> 16, 0, 255) << 8` into one v_ashr_pk_u8_i32 and takes the
// upper half of its result for zero, while an MI355X leaves that half of the register as it was -- the two bytes ORed in above came
// out mixed with stale register contents (tests/test_display_resources.py keeps the instruction out of this file's code).
__device__ __forceinline__ uint32_t pack4(int b0, int b1, int b2, int b3) {
    const uint32_t lo = __builtin_amdgcn_perm((uint32_t)b1, (uint32_t)b0, 0x0c0c0400u);      // bytes b0, b1, 0, 0
    const uint32_t hi = __builtin_amdgcn_perm((uint32_t)b3, (uint32_t)b2, 0x04000c0cu);      // bytes 0, 0, b2, b3
    return lo | hi;
}

__device__ __forceinline__ Chroma4 chroma_replicate(uint32_t cw) {
    Chroma4 c;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        c.cr[i] = byte_of(cw, 2 * (i >> 1));
        c.cb[i] = byte_of(cw, 2 * (i >> 1) + 1);
    }
    return c;
}

// disp_hmix() of one chroma row for the lane's four pixels: samples 2 ux - 1 .. 2 ux + 2, the outer two clamped to the plane
__device__ __forceinline__ Chroma4 chroma_hmix(const uint8_t* row, int ux, int wq) {
    const uint32_t* r = (const uint32_t*)row;
    const uint32_t mid = r[ux], left = r[ux > 0 ? ux - 1 : 0], right = r[ux < wq - 1 ? ux + 1 : wq - 1];
    const uint32_t before = ux > 0 ? left >> 16 : mid, after = ux < wq - 1 ? right : mid >> 16;      // their low 16 bits: Cr, Cb
    const int cr[4] = {byte_of(before, 0), byte_of(mid, 0), byte_of(mid, 2), byte_of(after, 0)};
    const int cb[4] = {byte_of(before, 1), byte_of(mid, 1), byte_of(mid, 3), byte_of(after, 1)};
    Chroma4 h;                                                  // pixel i: near sample 1 + (i >> 1), far one to its left (even i) or right
    h.cr[0] = disp_hmix(cr[1], cr[0]); h.cr[1] = disp_hmix(cr[1], cr[2]); h.cr[2] = disp_hmix(cr[2], cr[1]); h.cr[3] = disp_hmix(cr[2], cr[3]);
    h.cb[0] = disp_hmix(cb[1], cb[0]); h.cb[1] = disp_hmix(cb[1], cb[2]); h.cb[2] = disp_hmix(cb[2], cb[1]); h.cb[3] = disp_hmix(cb[2], cb[3]);
    return h;
}

__device__ __forceinline__ Chroma4 chroma_vmix(const Chroma4& near_row, const Chroma4& far_row) {
    Chroma4 c;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        c.cr[i] = disp_vmix(near_row.cr[i], far_row.cr[i]);
        c.cb[i] = disp_vmix(near_row.cb[i], far_row.cb[i]);
    }
    return c;
}

// the lane's four pixels of row y to `out` (their address in the picture); pixel i has x & 3 == i
template <int FMT, bool DITHER, bool MASK>
__device__ __forceinline__ void store4(uint8_t* out, uint32_t luma, const Chroma4& c, int y) {
    DispRgb p[4];
#pragma unroll
    for (int i = 0; i < 4; i++) p[i] = disp_matrix(byte_of(luma, i), c.cr[i], c.cb[i]);
    if (FMT == DISP_RGB24) {
        Dwords3 d;
        d.v[0] = pack4(p[0].r, p[0].g, p[0].b, p[1].r);
        d.v[1] = pack4(p[1].g, p[1].b, p[2].r, p[2].g);
        d.v[2] = pack4(p[2].b, p[3].r, p[3].g, p[3].b);
        *(Dwords3*)out = d;
    } else if (FMT == DISP_RGBX32) {
        Dwords4 d;
#pragma unroll
        for (int i = 0; i < 4; i++) d.v[i] = pack4(p[i].r, p[i].g, p[i].b, 255);
        *(Dwords4*)out = d;
    } else {
        uint32_t q[4];
#pragma unroll
        for (int i = 0; i < 4; i++) q[i] = disp_pack555(p[i], DITHER ? disp_dither(i, y) : 0, MASK ? 1 : 0);      // x & 3 == i
        Dwords2 d;
        d.v[0] = q[0] | (q[1] << 16);
        d.v[1] = q[2] | (q[3] << 16);
        *(Dwords2*)out = d;
    }
}

template <int FMT, bool BILINEAR, bool DITHER, bool MASK>
__global__ __launch_bounds__(kThreads) void display_convert_kernel(const psxhip_display_job_t j) {
    const int f = (int)blockIdx.y;
    if (j.d_decoded && j.d_decoded[f].status != PSXHIP_DEC_OK) return;            // the reconstruct kernel's rule, one stage further
    const int wq = j.width >> 2, hh = j.height >> 1;
    const int u = (int)(blockIdx.x * (unsigned)kThreads + threadIdx.x);           // < 512 * 256
    if (u >= wq * hh) return;
    const int uy = u / wq, ux = u - uy * wq;
    const size_t w = (size_t)j.width;
    const uint8_t* frame = j.d_frames + (size_t)f * j.frame_stride;
    const uint8_t* chroma = frame + w * (size_t)j.height;
    const uint32_t luma0 = ((const uint32_t*)(frame + w * (size_t)(2 * uy)))[ux];
    const uint32_t luma1 = ((const uint32_t*)(frame + w * (size_t)(2 * uy + 1)))[ux];
    constexpr int kPixelBytes = FMT == DISP_RGB24 ? 3 : (FMT == DISP_RGBX32 ? 4 : 2);
    uint8_t* out = j.d_dst + (size_t)f * j.dst_stride + (size_t)(2 * uy) * j.dst_pitch + (size_t)ux * (4 * kPixelBytes);
    if (BILINEAR) {
        const Chroma4 mid = chroma_hmix(chroma + w * (size_t)uy, ux, wq);
        const Chroma4 up = chroma_hmix(chroma + w * (size_t)(uy > 0 ? uy - 1 : 0), ux, wq);
        const Chroma4 down = chroma_hmix(chroma + w * (size_t)(uy < hh - 1 ? uy + 1 : hh - 1), ux, wq);
        store4<FMT, DITHER, MASK>(out, luma0, chroma_vmix(mid, up), 2 * uy);
        store4<FMT, DITHER, MASK>(out + j.dst_pitch, luma1, chroma_vmix(mid, down), 2 * uy + 1);
    } else {
        const Chroma4 c = chroma_replicate(((const uint32_t*)(chroma + w * (size_t)uy))[ux]);
        store4<FMT, DITHER, MASK>(out, luma0, c, 2 * uy);
        store4<FMT, DITHER, MASK>(out + j.dst_pitch, luma1, c, 2 * uy + 1);
    }
}

template <int FMT, bool BILINEAR, bool DITHER, bool MASK>
void launch(const psxhip_display_job_t& j, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((display_convert_kernel<FMT, BILINEAR, DITHER, MASK>), grid, dim3(kThreads), 0, stream, j);
}

template <int FMT, bool DITHER, bool MASK>
void launch_chroma(const psxhip_display_job_t& j, dim3 grid, hipStream_t stream) {
    if (j.options & PSXHIP_DISPLAY_CHROMA_BILINEAR) launch<FMT, true, DITHER, MASK>(j, grid, stream);
    else launch<FMT, false, DITHER, MASK>(j, grid, stream);
}

}  // namespace

extern "C" hipError_t psxhip_display_launch(const psxhip_display_job_t* job, void* stream) {
    const int units = (job->width / 4) * (job->height / 2);
    for (int base = 0; base < job->n_frames; base += kMaxFramesPerLaunch) {
        psxhip_display_job_t j = *job;
        j.n_frames = job->n_frames - base < kMaxFramesPerLaunch ? job->n_frames - base : kMaxFramesPerLaunch;
        j.d_frames += (size_t)base * job->frame_stride;
        j.d_dst += (size_t)base * job->dst_stride;
        if (j.d_decoded) j.d_decoded += base;
        const dim3 grid((unsigned)((units + kThreads - 1) / kThreads), (unsigned)j.n_frames);
        const bool dither = (j.options & PSXHIP_DISPLAY_DITHER) != 0, mask = (j.options & PSXHIP_DISPLAY_MASK_BIT) != 0;
        if (j.out_format == PSXHIP_OUT_RGB24) launch_chroma<DISP_RGB24, false, false>(j, grid, (hipStream_t)stream);
        else if (j.out_format == PSXHIP_OUT_RGBX32) launch_chroma<DISP_RGBX32, false, false>(j, grid, (hipStream_t)stream);
        else if (dither && mask) launch_chroma<DISP_RGB555, true, true>(j, grid, (hipStream_t)stream);
        else if (dither) launch_chroma<DISP_RGB555, true, false>(j, grid, (hipStream_t)stream);
        else if (mask) launch_chroma<DISP_RGB555, false, true>(j, grid, (hipStream_t)stream);
        else launch_chroma<DISP_RGB555, false, false>(j, grid, (hipStream_t)stream);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
