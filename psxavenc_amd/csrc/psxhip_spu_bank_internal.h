// psxhip_spu_bank_internal.h -- glue between the sound bank's host layer (psxhip_spu_bank.cpp) and its kernels (spu_bank_kernels.hip):
// the job structs and the launch functions.  The rows and tiles the jobs point at are the plan's (spu_bank_plan.h).  A launch function
// fills nothing but the launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spu_bank_plan.h"

/* bumped with every change to spu_bank_kernels.hip */
#define PSXHIP_SPU_BANK_KERNEL_REV "spubank-k1.0"

#ifdef __cplusplus
extern "C" {
#endif

/* spu_bank_frame_kernel: one wavefront per entry writes the entry's frame words and ORs its loop flags into the data blocks */
typedef struct {
	const psxhip_spu_bank_row_t *rows;      /* [n_entries], 16-byte aligned */
	int n_entries;
	uint8_t *out;                           /* the bank, 16-byte aligned */
} psxhip_spu_bank_frame_job_t;
hipError_t psxhip_spu_bank_frame_launch(const psxhip_spu_bank_frame_job_t *j, void *stream);

/* spu_bank_check_kernel: one 256-lane workgroup per tile; status[entry] (zero before the launch) takes PSXHIP_SPU_BANK_STATUS_* */
typedef struct {
	const psxhip_spu_bank_row_t *rows;
	const psxhip_spu_bank_tile_t *tiles;    /* [n_tiles] */
	int n_tiles;
	const uint8_t *bank;                    /* 16-byte aligned */
	int32_t *status;                        /* [n_entries] */
} psxhip_spu_bank_check_job_t;
hipError_t psxhip_spu_bank_check_launch(const psxhip_spu_bank_check_job_t *j, void *stream);

#ifdef __cplusplus
}
#endif
