// afe_layout.h -- the audio front-end's job (what psxhip_resample.cpp hands audio_frontend_kernels.hip) and the LDS working set of
// afe_kernel: [the header] [the coefficient table, when it sits in LDS] then per output channel the span and its shifted copy.  The
// kernel places the spans by it, the launch sizes its dynamic LDS by it, and the host's plan (resample_plan.cpp) decides coef_lds and
// the grid by it.  Constants and arithmetic only, no HIP: the kernel and a host compiler read the same text (PSX_LAYOUT_HD: the
// pattern of mdec_layout.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PSX_LAYOUT_HD __host__ __device__ inline
#else
#define PSX_LAYOUT_HD inline
#endif

/* one launch of the audio front-end (audio_frontend_kernels.hip): n_out outputs of a stream, from the filter history and n_in
 * new source samples.  Indices are relative to the launch's first new sample; history sample h of channel c is y[h - (T - 1)]. */
#define PSXHIP_AFE_TILE 256                 /* outputs per tile = threads per workgroup */
typedef struct {
	const void *src[8];                 /* interleaved: src[0] only */
	int fmt, sch, dch;
	int bypass;                         /* equal rates: y copied, no filter, no history */
	int64_t n_in, n_out;                /* n_in <= 2^28 (the host cuts longer calls); n_out up to 16x that: indices are int64 */
	int64_t i0;                         /* input index of output 0 (>= -H) */
	int r0;                             /* (its absolute index * M) mod L */
	int L, M, P, T, H;
	const int16_t *coef;                /* [P][T] Q15 taps, device memory */
	int coef_lds;                       /* 1: the table is copied into LDS once per workgroup */
	int span;                           /* int16 per channel per copy in LDS: >= (L - 1 + (TILE - 1) M) / L + T, even */
	const int16_t *hist_in;             /* [dch][T - 1] */
	int16_t *hist_out;                  /* [dch][T - 1], written by the launch (the last tile) */
	int16_t *dst;                       /* [n_out][dch] */
	int16_t mix[8][8];                  /* [dst][src] Q14 */
} psxhip_afe_job_t;

// the header of every workgroup (Header of the kernel file, which asserts its size): the matrix as int32 [8][8], eight source pointers
constexpr int kAfeHeaderBytes = 320, kAfeHeaderDwords = kAfeHeaderBytes / 4;

// dwords of the coefficient table in LDS: P * T int16 (T is even), none when the kernel reads it from memory
PSX_LAYOUT_HD constexpr int afe_table_dwords(bool coef_lds, int P, int T) { return coef_lds ? (P * T) >> 1 : 0; }

// the dynamic LDS of a launch: a bypass launch takes the header alone
PSX_LAYOUT_HD size_t afe_lds_bytes(bool bypass, bool coef_lds, int P, int T, int dch, int span) {
    if (bypass) return kAfeHeaderBytes;
    return kAfeHeaderBytes + (size_t)afe_table_dwords(coef_lds, P, T) * 4 + (size_t)dch * 2 * span * 2;
}
