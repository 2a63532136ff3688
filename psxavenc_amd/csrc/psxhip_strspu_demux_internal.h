// psxhip_strspu_demux_internal.h -- glue between the STRSPU reader's C-ABI layer (psxhip_str_demux.cpp) and its kernels
// (strspu_demux_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/psxav_hip.h"
#include "strspu_chunk.h"

/* bumped with every change to the STRSPU reader's kernels: profiles/ is keyed by it */
#define PSXHIP_STRSPU_DEMUX_KERNEL_REV "strspu-dmx-k1.0"

#ifdef __cplusplus
extern "C" {
#endif

/* One de-interleave: chunk k of stream s lies at in + s * in_stream_stride + src * chunk_stride, src = src_chunk ?
 * src_chunk[s * src_stream_stride + k] : k, a negative src skips the chunk; block b of lane c goes to record (k B + b) * channels + c. */
typedef struct {
	const uint8_t *in;
	size_t in_stream_stride, chunk_stride, lane_offset;
	int blocks;                  /* B = lane_bytes / 16 */
	int channels, n_chunks;
	const int32_t *src_chunk;    /* or NULL */
	size_t src_stream_stride;    /* elements; 0: one table for every stream */
	uint8_t *units;
	size_t units_stream_stride;
	int vec16;                   /* every source block is 16-byte aligned: one 16-byte load instead of four dwords */
} psxhip_spu_deinterleave_job_t;
int psxhip_spu_deinterleave_launch(const psxhip_spu_deinterleave_job_t *j, int n_streams, void *stream);

/* The audio half of one STRSPU demux call, behind the video half on the same stream.  The workspace, per stream audio_capacity words
 * each: d_owner, the lowest position of a sector per chunk number (all ones = none; read as int32 it is the de-interleave's source
 * table), and d_count, the sectors per chunk number.  The launch function sets them. */
typedef struct {
	StrspuChunkRules rules;
	int n_streams, n_sectors, audio_capacity;
	const uint8_t *d_sectors;
	size_t in_stream_stride;
	uint8_t *d_units;
	size_t units_stream_stride;
	psxhip_strspu_chunk_info_t *d_chunk_info;
	psxhip_str_sector_t *d_user_table;            /* or NULL */
	psxhip_str_summary_t *d_summary;              /* the video half's: the audio sectors move from n_other to n_audio */
	psxhip_strspu_audio_summary_t *d_audio_summary;
	uint32_t *d_owner, *d_count;
} psxhip_strspu_demux_job_t;
int psxhip_strspu_demux_launch(int device, const psxhip_strspu_demux_job_t *j, void *stream);

#ifdef __cplusplus
}
#endif
