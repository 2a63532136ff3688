// psxhip_disc_internal.h -- glue between the disc finisher's C-ABI layer (psxhip_disc.cpp) and its kernels (disc_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/psxav_hip.h"

/* bumped with every change to the finisher's kernels: profiles/ is keyed by it */
#define PSXHIP_DISC_KERNEL_REV "disc-k1.0"

#define PSXHIP_DISC_SECTORS_PER_GROUP 4     /* one wavefront per sector, four to a 256-thread workgroup */

#ifdef __cplusplus
extern "C" {
#endif

/* One finish launch; the whole job travels as kernel arguments (2.8 KiB), so the call uploads nothing.  Everything in it has been
 * checked by psxhip_disc.cpp: the kernel bounds nothing again but the source sector number. */
typedef struct {
	const uint8_t *base;
	int64_t stride;
	int32_t n_sectors;
	int32_t lead;               /* 2352 - sector_size: where the source's byte 0 lies in the raw sector (0, 16; 2048-byte sources: 24) */
	int32_t count;              /* slots of the period the source owns */
	int16_t file, channel;      /* -1: keep */
	uint32_t data_subheader;    /* 2048-byte sources: the subheader, little-endian */
	int32_t has_subheader;
} psxhip_disc_dev_source_t;

typedef struct {
	psxhip_disc_dev_source_t src[PSXHIP_DISC_MAX_SOURCES];
	int8_t slot_source[PSXHIP_DISC_MAX_PERIOD];
	uint8_t slot_rank[PSXHIP_DISC_MAX_PERIOD];
	int32_t period;
	int32_t start_lba;
	int64_t first_out, n_out;
	uint8_t *out;
} psxhip_disc_finish_job_t;

typedef struct {
	const uint8_t *image;
	int64_t n_sectors;
	int64_t start_lba;          /* -1: the MSF is only checked for being BCD */
	int32_t *status;            /* or NULL */
	psxhip_disc_summary_t *summary;   /* zero before the launch */
} psxhip_disc_check_job_t;

int psxhip_disc_tables(int device);
hipError_t psxhip_disc_finish_launch(const psxhip_disc_finish_job_t *j, int grid, void *stream);
hipError_t psxhip_disc_check_launch(const psxhip_disc_check_job_t *j, int grid, void *stream);

#ifdef __cplusplus
}
#endif
