// psxhip_spu_seam_internal.h -- glue between the sound bank's host layer (psxhip_spu_bank.cpp) and the seam kernels
// (spu_seam_kernels.hip; "psxhip SPU loop seam v1"): the job structs and the launch functions.  The tables the
// jobs point at are the plan's (spu_bank_plan.h).  A launch function fills nothing but the launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spu_bank_plan.h"

/* bumped with every change to spu_seam_kernels.hip or spu_seam_core.h */
#define PSXHIP_SPU_SEAM_KERNEL_REV "spuseam-k1.0"

#ifdef __cplusplus
extern "C" {
#endif

/* spu_seam_step_kernel: one lane per body chain of the seam chain table; spu_seam_step (spu_seam_core.h) with pass number k */
typedef struct {
	psxhip_adpcm_chain_t *chains;               /* the DEVICE table's body chains: [n_body] */
	psxhip_adpcm_state_t *states;               /* their state slots: [n_body] */
	const psxhip_adpcm_state_t *first_states;   /* slot 0 of the state table: the intros' end states */
	psxhip_adpcm_state_t *start;                /* [n_body] s_k */
	const int32_t *body_intro;                  /* [n_body] the intro's slot or -1 */
	const int32_t *body_entry;                  /* [n_body] */
	const int32_t *body_units;                  /* [n_body] the body's units, as the plan has them */
	int32_t *outcome;                           /* [n_entries] */
	int n_body;
	int k;                                      /* -1: arm; 0 .. passes - 1 */
	int passes;
} psxhip_spu_seam_step_job_t;
hipError_t psxhip_spu_seam_step_launch(const psxhip_spu_seam_step_job_t *j, void *stream);

/* spu_seam_report_kernel: one lane per entry; spu_seam_report_entry (spu_seam_core.h) */
typedef struct {
	const psxhip_spu_seam_row_t *rows;          /* [n_entries] */
	int n_entries;
	const uint8_t *bank;                        /* 16-byte aligned */
	const int16_t *pcm;                         /* or NULL */
	psxhip_spu_seam_t *seam;                    /* [n_entries] */
} psxhip_spu_seam_report_job_t;
hipError_t psxhip_spu_seam_report_launch(const psxhip_spu_seam_report_job_t *j, void *stream);

#ifdef __cplusplus
}
#endif
