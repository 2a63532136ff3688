// psxhip_decode_internal.h -- glue between the decoder's C-ABI layer (psxhip_decode.cpp) and its kernels (mdec_decode_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/psxav_hip.h"

/* bumped with every change to the decoder's kernels: profiles/ is keyed by it */
#define PSXHIP_MDEC_DECODE_KERNEL_REV "mdec-dec-k1.0"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
	const uint8_t *d_bs;
	size_t bs_stride;
	const int32_t *d_sizes;             /* or NULL: uniform_size */
	int uniform_size;
	int n_frames, nblk, wrap;
	int16_t *d_levels;                  /* or NULL: parse only */
	psxhip_mdec_decoded_t *d_decoded;
} psxhip_mdec_parse_job_t;
hipError_t psxhip_mdec_parse_launch(const psxhip_mdec_parse_job_t *j, void *stream);

typedef struct {
	const int16_t *d_levels;
	const psxhip_mdec_decoded_t *d_decoded;
	uint8_t *d_frames;
	size_t frame_stride;
	int n_frames, width, height;
} psxhip_mdec_recon_job_t;
hipError_t psxhip_mdec_reconstruct_launch(const psxhip_mdec_recon_job_t *j, void *stream);

hipError_t psxhip_mdec_sse_launch(const uint8_t *d_a, const uint8_t *d_b, size_t frame_stride, int width, int height, int n_frames,
                                  unsigned long long *d_sse, void *stream);

#ifdef __cplusplus
}
#endif
