// audio_frontend_kernels.hip -- audio front-end for MI355X (gfx950): decoded PCM (S16 / S32 / F32, interleaved or planar, 1-8
// channels, any rate) -> interleaved int16 at the target rate and channel count, written where the ADPCM and STR kernels read
// their input (include/psxav_hip.h, psxhip_resampler_*; DESIGN.md section 10, "psxhip audio front-end v1").
//
// The reference hands this step to libswresample (psxavenc/decoding.c:215-254, :370-406).  The arithmetic here is this
// library's own and integer-only after the coefficient table (psxhip_resample.cpp designs it): int16 conversion, a Q14 channel
// matrix at the source rate, a Q15 polyphase filter summed exactly as two int32 halves, round, clamp.
//
// Mapping: HBM-bound streaming work.  A workgroup of 256 lanes walks tiles of 256 consecutive outputs (all output channels);
// lane t owns output t of the tile.  Per tile the workgroup stages the input span its outputs reach -- converted and mixed, from
// the launch's new samples or the filter history -- in LDS twice per channel, the second copy shifted by one sample, so that
// every (y[j], y[j + 1]) pair is one aligned dword whatever the parity of j.  Taps are read as dword pairs too (T is even) and
// multiplied with v_dot2_i32_i16 into two partial sums, one per half of the taps.  The coefficient table sits in LDS for the
// whole walk when it fits.  The tile after the last one writes the new history (the last T - 1 mixed samples per channel) into
// the other half of the handle's double buffer, so a stream cut into calls needs no second launch and no host round trip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psxhip_internal.h"

namespace {

typedef short s16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), c, false);
}

__device__ __forceinline__ int clamp16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// source sample (frame j, channel k) as int16 (spec step 1); p: the channel's plane (planar) or the interleaved buffer
__device__ __forceinline__ int load_x(int fmt, int sch, const void* p, int64_t j, int k) {
    const int64_t at = (fmt & 1) ? j : j * sch + k;
    if (fmt <= PSXHIP_PCM_S16P) return ((const int16_t*)p)[at];
    if (fmt <= PSXHIP_PCM_S32P) {
        const int64_t v = (((int64_t)((const int32_t*)p)[at]) + 32768) >> 16;
        return v > 32767 ? 32767 : (int)v;
    }
    const float f = ((const float*)p)[at] * 32768.0f;
    if (f != f) return 0;
    const float r = rintf(f);                        // half to even
    return r <= -32768.0f ? -32768 : (r >= 32767.0f ? 32767 : (int)r);
}

// LDS header of every workgroup: the matrix as int32 [8][8] and the source pointers.  (Held in scalar registers, unrolled over
// eight source channels, they spilled the kernel's scalar registers.)
struct Header {
    int mix[8][8];
    const void* src[8];
};
constexpr int kHeader = kAfeHeaderDwords;
static_assert(sizeof(Header) == kAfeHeaderBytes, "afe_layout.h: 80 dwords before the table");

// mixed samples y_c at relative input index j (spec step 2); j < 0 reads the history, j >= n_in reads zero
template <int DCH>
__device__ __forceinline__ void mixed(const psxhip_afe_job_t& a, const Header* hd, int64_t j, int* y) {
    if (j >= a.n_in) {
#pragma unroll
        for (int c = 0; c < DCH; c++) y[c] = 0;
        return;
    }
    if (j < 0) {
        const int h = (int)j + a.T - 1;
#pragma unroll
        for (int c = 0; c < DCH; c++) y[c] = h >= 0 ? a.hist_in[c * (a.T - 1) + h] : 0;
        return;
    }
    int s[DCH];
#pragma unroll
    for (int c = 0; c < DCH; c++) s[c] = 8192;
#pragma unroll 1
    for (int k = 0; k < a.sch; k++) {
        const int x = load_x(a.fmt, a.sch, hd->src[(a.fmt & 1) ? k : 0], j, k);
#pragma unroll
        for (int c = 0; c < DCH; c++) s[c] += hd->mix[c][k] * x;
    }
#pragma unroll
    for (int c = 0; c < DCH; c++) y[c] = clamp16(s[c] >> 14);
}

// load of source sample (frame j, channel k), FMT known at compile time (no format branch between a lane's loads)
template <int FMT>
__device__ __forceinline__ int load_t(const void* p, int sch, int64_t j, int k) {
    return load_x(FMT, sch, p, j, k);
}

// staging of a tile whose span lies inside [0, n_in): every lane converts and mixes span samples s and s + 256 in one go.  All
// of a lane's loads for a pair of source channels are issued before the first is used, so a staging pass waits for one memory
// latency per pair of source channels, not one per sample and channel.  A channel past the last (odd counts) reloads the last
// one; its matrix weight is zero.
template <int DCH, int FMT>
__device__ __forceinline__ void stage_inside(const psxhip_afe_job_t& a, const Header* hd, int64_t j0, int span, int16_t* y16, int tid) {
    const int sch = a.sch;
    for (int s = tid; s < span; s += 2 * PSXHIP_AFE_TILE) {
        const int s2 = s + PSXHIP_AFE_TILE < span ? s + PSXHIP_AFE_TILE : s;     // (a repeat of s when there is no second sample)
        int acc_a[DCH], acc_b[DCH];
#pragma unroll
        for (int c = 0; c < DCH; c++) acc_a[c] = acc_b[c] = 8192;
#pragma unroll 1
        for (int k = 0; k < sch; k += 2) {
            const int k1 = k + 1 < sch ? k + 1 : k;
            const void* p0 = hd->src[(FMT & 1) ? k : 0];
            const void* p1 = hd->src[(FMT & 1) ? k1 : 0];
            const int xa0 = load_t<FMT>(p0, sch, j0 + s, k), xa1 = load_t<FMT>(p1, sch, j0 + s, k1);
            const int xb0 = load_t<FMT>(p0, sch, j0 + s2, k), xb1 = load_t<FMT>(p1, sch, j0 + s2, k1);
#pragma unroll
            for (int c = 0; c < DCH; c++) {
                const int m0 = hd->mix[c][k], m1 = k + 1 < sch ? hd->mix[c][k1] : 0;
                acc_a[c] += m0 * xa0 + m1 * xa1;
                acc_b[c] += m0 * xb0 + m1 * xb1;
            }
        }
#pragma unroll
        for (int c = 0; c < DCH; c++) {
            const int ya = clamp16(acc_a[c] >> 14), yb = clamp16(acc_b[c] >> 14);
            y16[(2 * c) * span + s] = (int16_t)ya;
            if (s) y16[(2 * c + 1) * span + s - 1] = (int16_t)ya;
            if (s2 != s) {
                y16[(2 * c) * span + s2] = (int16_t)yb;
                y16[(2 * c + 1) * span + s2 - 1] = (int16_t)yb;
            }
        }
    }
}

template <int DCH, bool COEF_LDS>
__global__ void __launch_bounds__(PSXHIP_AFE_TILE) afe_kernel(const psxhip_afe_job_t a) {
    extern __shared__ uint32_t lds[];
    const int tid = threadIdx.x;
    const int64_t n_tiles = (a.n_out + PSXHIP_AFE_TILE - 1) / PSXHIP_AFE_TILE;
    Header* hd = (Header*)lds;
    if (tid < 64) hd->mix[tid >> 3][tid & 7] = a.mix[tid >> 3][tid & 7];
    if (tid < 8) hd->src[tid] = a.src[tid];
    __syncthreads();

    if (a.bypass) {
        for (int64_t n = (int64_t)blockIdx.x * PSXHIP_AFE_TILE + tid; n < a.n_out; n += (int64_t)gridDim.x * PSXHIP_AFE_TILE) {
            int y[DCH];
            mixed<DCH>(a, hd, n, y);
#pragma unroll
            for (int c = 0; c < DCH; c++) a.dst[n * DCH + c] = (int16_t)y[c];
        }
        return;
    }

    const int T = a.T, H = a.H, L = a.L, M = a.M, P = a.P;
    // LDS (afe_layout.h): [the header, 80 dwords] [the coefficient table, P * T / 2 dwords, when COEF_LDS] then per channel the span
    // (span / 2 dwords) and its shifted copy
    uint32_t* ybuf = lds + kHeader + afe_table_dwords(COEF_LDS, P, T);
    int16_t* y16 = (int16_t*)ybuf;
    const uint32_t* coef32 = (const uint32_t*)a.coef;
    if (COEF_LDS) {
        for (int i = tid; i < (P * T) >> 1; i += PSXHIP_AFE_TILE) lds[kHeader + i] = coef32[i];
        coef32 = lds + kHeader;
    }
    const int span = a.span;

    // the tile's first output sits at input index ib with remainder rb ((its index * M) mod L).  One 64-bit division per workgroup
    // for the first tile and the step; the walk then advances both without dividing (the per-tile division was most of the
    // kernel's scalar instructions, profiles/afe-k1.1_pmc.txt)
    const int64_t stepq = (int64_t)gridDim.x * PSXHIP_AFE_TILE * M;
    const int64_t step_i = stepq / L;
    const uint32_t step_r = (uint32_t)(stepq % L);
    const int64_t q0 = (int64_t)a.r0 + (int64_t)blockIdx.x * PSXHIP_AFE_TILE * M;
    int64_t ib = a.i0 + q0 / L;
    uint32_t rb = (uint32_t)(q0 % L);
    for (int64_t b = blockIdx.x; b <= n_tiles;
         b += gridDim.x, ib += step_i + (rb + step_r >= (uint32_t)L), rb = rb + step_r >= (uint32_t)L ? rb + step_r - L : rb + step_r) {
        if (b == n_tiles) {
            // the history the next call starts from: y[n_in - (T - 1) .. n_in - 1]
            for (int t = tid; t < T - 1; t += PSXHIP_AFE_TILE) {
                int y[DCH];
                mixed<DCH>(a, hd, a.n_in - (T - 1) + t, y);
#pragma unroll
                for (int c = 0; c < DCH; c++) a.hist_out[c * (T - 1) + t] = (int16_t)y[c];
            }
            continue;
        }
        const int64_t j0 = ib - H + 1;                       // span[0] is y[j0]

        __syncthreads();                                     // the previous tile's reads are done
        if (j0 >= 0 && j0 + span <= a.n_in) {                // the common case: the whole span is new samples
            switch (a.fmt) {
            case PSXHIP_PCM_S16: stage_inside<DCH, PSXHIP_PCM_S16>(a, hd, j0, span, y16, tid); break;
            case PSXHIP_PCM_S16P: stage_inside<DCH, PSXHIP_PCM_S16P>(a, hd, j0, span, y16, tid); break;
            case PSXHIP_PCM_S32: stage_inside<DCH, PSXHIP_PCM_S32>(a, hd, j0, span, y16, tid); break;
            case PSXHIP_PCM_S32P: stage_inside<DCH, PSXHIP_PCM_S32P>(a, hd, j0, span, y16, tid); break;
            case PSXHIP_PCM_F32: stage_inside<DCH, PSXHIP_PCM_F32>(a, hd, j0, span, y16, tid); break;
            default: stage_inside<DCH, PSXHIP_PCM_F32P>(a, hd, j0, span, y16, tid); break;
            }
        } else {                                             // history, stream start or end: per sample, with the range checks
            for (int s = tid; s < span; s += PSXHIP_AFE_TILE) {
                int y[DCH];
                mixed<DCH>(a, hd, j0 + s, y);
#pragma unroll
                for (int c = 0; c < DCH; c++) {
                    y16[(2 * c) * span + s] = (int16_t)y[c];
                    if (s) y16[(2 * c + 1) * span + s - 1] = (int16_t)y[c];
                }
            }
        }
        __syncthreads();

        const int64_t n = b * PSXHIP_AFE_TILE + tid;
        if (n >= a.n_out) continue;
        const uint32_t pos = rb + (uint32_t)tid * (uint32_t)M;  // < L + 255 M < 2^27
        const uint32_t di = pos / (uint32_t)L;
        const uint32_t r = pos - di * (uint32_t)L;
        const uint32_t ph = P == L ? r : (r * (uint32_t)P) / (uint32_t)L;
        const uint32_t* cp = coef32 + ((ph * (uint32_t)T) >> 1);
        // output t reads span[di .. di + T - 1]: from the plain copy when di is even, else from the shifted one at di - 1
        const uint32_t* yp[DCH];
#pragma unroll
        for (int c = 0; c < DCH; c++)
            yp[c] = ybuf + ((((2 * c + (di & 1)) * span) + di - (di & 1)) >> 1);
        int acc0[DCH], acc1[DCH];
#pragma unroll
        for (int c = 0; c < DCH; c++) acc0[c] = acc1[c] = 0;
        const int h2 = H >> 1;
#pragma unroll 4
        for (int m = 0; m < h2; m++) {
            const uint32_t k = cp[m];
#pragma unroll
            for (int c = 0; c < DCH; c++) acc0[c] = dot2(k, yp[c][m], acc0[c]);
        }
        if (H & 1) {                                         // the pair (H - 1, H) straddles the halves
            const uint32_t k = cp[h2];
#pragma unroll
            for (int c = 0; c < DCH; c++) {
                acc0[c] = dot2(k & 0xFFFFu, yp[c][h2], acc0[c]);
                acc1[c] = dot2(k & 0xFFFF0000u, yp[c][h2], acc1[c]);
            }
        }
#pragma unroll 4
        for (int m = (H + 1) >> 1; m < H; m++) {
            const uint32_t k = cp[m];
#pragma unroll
            for (int c = 0; c < DCH; c++) acc1[c] = dot2(k, yp[c][m], acc1[c]);
        }
        int o[DCH];
#pragma unroll
        for (int c = 0; c < DCH; c++) {
            const int64_t S = (int64_t)acc0[c] + acc1[c];
            const int64_t v = (S + 16384) >> 15;
            o[c] = v < -32768 ? -32768 : (v > 32767 ? 32767 : (int)v);
        }
        if (DCH == 2 && !((uintptr_t)a.dst & 3)) {
            ((uint32_t*)a.dst)[n] = (uint32_t)(uint16_t)o[0] | ((uint32_t)(uint16_t)o[DCH - 1] << 16);
        } else {
#pragma unroll
            for (int c = 0; c < DCH; c++) a.dst[n * DCH + c] = (int16_t)o[c];
        }
    }
}

template <int DCH>
const void* kernel_of(int coef_lds) {
    return coef_lds ? (const void*)afe_kernel<DCH, true> : (const void*)afe_kernel<DCH, false>;
}

const void* kernel_for(int dch, int coef_lds) {
    switch (dch) {
    case 1: return kernel_of<1>(coef_lds);
    case 2: return kernel_of<2>(coef_lds);
    case 3: return kernel_of<3>(coef_lds);
    case 4: return kernel_of<4>(coef_lds);
    case 5: return kernel_of<5>(coef_lds);
    case 6: return kernel_of<6>(coef_lds);
    case 7: return kernel_of<7>(coef_lds);
    case 8: return kernel_of<8>(coef_lds);
    }
    return nullptr;
}

}  // namespace

extern "C" size_t psxhip_afe_lds_bytes(const psxhip_afe_job_t* j) {
    return afe_lds_bytes(j->bypass != 0, j->coef_lds != 0, j->P, j->T, j->dch, j->span);
}

extern "C" hipError_t psxhip_afe_prepare(int dch, int coef_lds, size_t lds_bytes) {
    const void* k = kernel_for(dch, coef_lds);
    if (!k) return hipErrorInvalidValue;
    return lds_bytes > 65536 ? hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) : hipSuccess;
}

extern "C" hipError_t psxhip_afe_launch(const psxhip_afe_job_t* j, int grid, void* stream) {
    const void* k = kernel_for(j->dch, j->coef_lds);
    if (!k || grid < 1) return hipErrorInvalidValue;
    void* args[] = {(void*)j};
    return hipLaunchKernel(k, dim3((unsigned)grid), dim3(PSXHIP_AFE_TILE), args, psxhip_afe_lds_bytes(j), (hipStream_t)stream);
}
