// psxhip_disc_read_internal.h -- glue between the disc reader's C-ABI layer (psxhip_disc_read.cpp) and its kernels
// (disc_read_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/psxav_hip.h"

/* bumped with every change to the reader's kernels: profiles/ is keyed by it */
#define PSXHIP_DISC_READ_KERNEL_REV "disc-rd-k1.0"

#define PSXHIP_DISC_READ_SECTORS_PER_GROUP 4     /* classify, gather: one wavefront per sector, four to a 256-thread workgroup */
#define PSXHIP_DISC_READ_SPAN 1024               /* count, place: sectors per wavefront (one 64-thread workgroup) */

#ifdef __cplusplus
extern "C" {
#endif

/* One read; the whole job travels as kernel arguments (2.3 KiB), so the call uploads nothing.  Everything in it has been checked
 * by psxhip_disc_read.cpp. */
typedef struct {
	uint8_t *base;
	int64_t stride;
	int32_t capacity;
	int32_t lead4;              /* first dword of the raw sector that is written: 0 (2352), 4 (2336), 6 (2048) */
	int32_t size4;              /* dwords written */
	int32_t reserved;
} psxhip_disc_read_dev_track_t;

typedef struct {
	const uint8_t *image;
	int64_t n_sectors;
	int64_t first_group;        /* classify, gather: the launch's first workgroup (a launch has fewer than 2^32 threads) */
	int32_t n_tracks;
	int32_t n_spans;            /* ceil(n_sectors / PSXHIP_DISC_READ_SPAN) */
	psxhip_disc_read_sector_t *table;       /* the caller's, or the workspace's */
	int32_t *span_counts;       /* workspace [n_spans][64]: per span and track the count, then (prefix) the sectors before the span */
	int32_t *track_counts;
	psxhip_disc_read_summary_t *summary;    /* zero before the first launch */
	/* routing key of track t: file_number + 1 | (channel_number + 1) << 9 | submode_mask << 16 | submode_value << 24 */
	uint32_t key[PSXHIP_DISC_MAX_SOURCES];
	psxhip_disc_read_dev_track_t track[PSXHIP_DISC_MAX_SOURCES];
} psxhip_disc_read_job_t;

int psxhip_disc_read_tables(int device);
/* classify (repair, verdict, routing key, record) -> count -> prefix -> place (ordinals, dropped) -> gather, all on `stream` */
hipError_t psxhip_disc_read_launch(const psxhip_disc_read_job_t *j, void *stream);

#ifdef __cplusplus
}
#endif
