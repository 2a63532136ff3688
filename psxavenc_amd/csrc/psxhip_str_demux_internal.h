// psxhip_str_demux_internal.h -- glue between the STR reader's C-ABI layer (psxhip_str_demux.cpp) and its kernels
// (str_demux_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/psxav_hip.h"

/* bumped with every change to the reader's kernels: profiles/ is keyed by it */
#define PSXHIP_STR_DEMUX_KERNEL_REV "str-dmx-k1.0"

#define PSXHIP_STR_DEMUX_SCAN_BLOCK 256     /* sectors per workgroup of the scan and place passes */

#ifdef __cplusplus
extern "C" {
#endif

/* One demux call.  The workspace (all per stream, stream s at s * the per-stream count):
 *   d_rec      [n_sectors] x 4 words: what the scan pass read of each sector (kind, frame_index, chunk fields, audio rank in its block)
 *   d_table    [n_sectors] x psxhip_str_sector_t: the place pass's verdict, read by the gather pass
 *   d_blocks   [n_blocks] audio sectors per scan block, turned into their exclusive prefix sums by the prefix pass
 *   d_owner    [max_frames x chunk_cap] lowest position of a placeable sector per (row, chunk); all ones = none
 *   d_lead     [max_frames] (chunk_index != 0) << 31 | position, minimised; all ones = no sector in the row
 *   d_status   [max_frames] PSXHIP_STR_FRAME_* bits collected from the row's sectors
 *   d_min      [1] the smallest frame_index of a video sector; all ones = none
 * d_owner, d_lead and d_min start as all ones, d_status and the summaries as zero: the launch function sets them. */
typedef struct {
	int format, sector_size, sub_at, hdr_at;      /* sub_at < 0: no subheader */
	int audio_on, xa_file, xa_channel, video_id, width, height;
	int n_streams, n_sectors, n_blocks, max_frames, chunk_cap, xa_capacity;
	int64_t first_frame;
	const uint8_t *d_sectors;
	size_t in_stream_stride;
	uint8_t *d_bs;
	size_t bs_stride, bs_stream_stride;
	int32_t *d_bs_sizes;
	psxhip_str_frame_info_t *d_info;
	uint8_t *d_xa;
	size_t xa_stream_stride;
	psxhip_str_sector_t *d_user_table;            /* or NULL */
	psxhip_str_summary_t *d_summary;
	uint32_t *d_rec, *d_blocks, *d_owner, *d_lead, *d_status, *d_min;
	psxhip_str_sector_t *d_table;
} psxhip_str_demux_job_t;
int psxhip_str_demux_launch(int device, const psxhip_str_demux_job_t *j, void *stream);

#ifdef __cplusplus
}
#endif
