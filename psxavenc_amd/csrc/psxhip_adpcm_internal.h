// psxhip_adpcm_internal.h -- glue between the ADPCM / sector C-ABI layer (psxhip_adpcm_encode.cpp, psxhip_adpcm_decode.cpp,
// psxhip_audio_api.cpp, psxhip_str.cpp) and its kernels (adpcm_kernels.hip, adpcm_decode_kernels.hip, sector_kernels.hip, strspu_kernels.hip): the job
// struct every kernel takes, declared once, and the launch functions.  A launch function fills nothing but the launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/psxav_hip.h"

/* bumped with every change to the ADPCM decoder's kernels */
#define PSXHIP_ADPCM_DECODE_KERNEL_REV "adpcm-dec-k1.0"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- adpcm_kernels.hip: the encoder ---- */
/* adpcm_chains_kernel: every chain serially, four chains per wavefront */
typedef struct {
	const int16_t *samples;
	const psxhip_adpcm_chain_t *chains;
	const int32_t *unit_base;
	int n_chains;
	int filter_count;   /* 5 SPU, 4 XA */
	int range;          /* 12 (4-bit) or 8 (8-bit) */
	psxhip_adpcm_state_t *states;
	uint8_t *units;
} psxhip_adpcm_chain_job_t;
hipError_t psxhip_adpcm_chains_launch(const psxhip_adpcm_chain_job_t *j, void *stream);

/* adpcm_call_kernel: one launch for the reference's per-call pattern -- up to four chains, descriptors and start states in the
 * kernel arguments, samples read from device-visible (page-locked host) memory */
#define PSXHIP_ADPCM_CALL_STAGE_MAX 8192     /* int16 elements staged in LDS (an XA sector is 4032) */
typedef struct {
	const int16_t *samples;                 /* device-visible; chains' sample_offset counts from here */
	psxhip_adpcm_chain_t chains[4];
	psxhip_adpcm_state_t states_in[4];
	int32_t unit_base[4];
	int n_chains, filter_count, range;
	int stage_elems;                        /* > 0: copy this many elements into LDS first (multiple of 8, <= PSXHIP_ADPCM_CALL_STAGE_MAX) */
	psxhip_adpcm_state_t *states_out;       /* [n_chains] */
	uint8_t *units;                         /* unit records (PSXHIP_ADPCM_RECORD_SIZE(bits) apart), or NULL when spu_out is given */
	uint8_t *spu_out;                       /* packed 16-byte SPU blocks, or NULL */
} psxhip_adpcm_call_job_t;
hipError_t psxhip_adpcm_call_launch(const psxhip_adpcm_call_job_t *j, void *stream);

/* adpcm_chunks_kernel: chains cut along time, speculate (verify = 0) and verify passes */
typedef struct {
	const int16_t *samples;
	const psxhip_adpcm_chain_t *chains;
	const int32_t *unit_base;        /* record index of each chain's unit 0 */
	const int64_t *state_base;       /* index into unit_states of each chain's unit 0 */
	const int32_t *chunk_chain;      /* [n_chunks] chain of each chunk */
	const int32_t *chunk_first;      /* [n_chunks] first unit (chain-local) of each chunk */
	int n_chunks, chunk_units, warmup_units;
	int filter_count, range;
	const psxhip_adpcm_state_t *chain_states;   /* start state of every chain (the truth as far as it is known) */
	const int32_t *lead_units;                  /* [n_chains] units available BEFORE the chain's first unit for guessing
	                                             *            its start state (0: start from chain_states as given) */
	const uint8_t *start_known;                 /* [n_chains] 0: chain_states[c] is not known yet, keep the guess */
	psxhip_adpcm_state_t *unit_states;          /* state after every unit */
	psxhip_adpcm_state_t *start_used;           /* [n_chunks] state each chunk was last encoded from */
	uint8_t *units;
	int *changed;                    /* verify: set to 1 when any chunk had to be re-encoded (device memory, one word per pass) */
	const int *changed_before;       /* verify: the previous pass's word, NULL for the first pass of a batch -- a pass whose
	                                  * predecessor changed nothing has nothing to do (the fixpoint was reached) and returns at once */
} psxhip_adpcm_chunk_job_t;
hipError_t psxhip_adpcm_chunks_launch(const psxhip_adpcm_chunk_job_t *j, int verify, void *stream);
/* states[c] = the state after chain c's last unit (chains without units keep theirs) */
hipError_t psxhip_adpcm_final_states_launch(const psxhip_adpcm_chain_t *chains, const int64_t *state_base, int n_chains,
                                            const psxhip_adpcm_state_t *unit_states, psxhip_adpcm_state_t *states, void *stream);
hipError_t psxhip_spu_pack_launch(const uint8_t *units, int n_blocks, uint8_t *out, void *stream);

/* ---- adpcm_beam_kernels.hip: the encoder with a delayed decision inside the unit ("psxhip ADPCM beam v1") ---- */
/* bumped with every change to adpcm_beam_kernels.hip */
#define PSXHIP_ADPCM_BEAM_KERNEL_REV "adpcm-beam-k1.0"
/* adpcm_beam_chains_kernel: every chain serially, four chains per wavefront */
typedef struct {
	psxhip_adpcm_chain_job_t job;
	int beam;                        /* 1 .. 4 */
	uint32_t *unit_err;              /* optional: the winner's e per record index */
} psxhip_adpcm_beam_chain_job_t;
hipError_t psxhip_adpcm_beam_chains_launch(const psxhip_adpcm_beam_chain_job_t *j, void *stream);
/* adpcm_beam_chunks_kernel: the tables and words of adpcm_chunks_kernel, four chunks per wavefront */
typedef struct {
	psxhip_adpcm_chunk_job_t job;
	int beam;
	uint32_t *unit_err;              /* optional */
} psxhip_adpcm_beam_chunk_job_t;
hipError_t psxhip_adpcm_beam_chunks_launch(const psxhip_adpcm_beam_chunk_job_t *j, int verify, void *stream);

/* ---- adpcm_decode_kernels.hip: the decoder ---- */
/* adpcm_decode_kernel: serial per chain, or chunks of chains (speculate, verify passes) */
typedef struct {
	const uint8_t *units;
	const psxhip_adpcm_chain_t *chains;
	const int32_t *unit_base;
	int n_items;                         /* work items: chains, or chunks when chunk_chain is given */
	int filter_count;
	psxhip_adpcm_state_t *states;        /* [n_chains] serial: read and updated; chunked: the start state of every chain's first chunk */
	int16_t *samples;
	uint8_t *unit_flags;                 /* optional: one byte per record index */
	int16_t *tail;                       /* optional: 28 samples per chain, the unit sample_limit cuts */
	const int32_t *chunk_chain;          /* [n_items] chain of each chunk; NULL: one work item per chain */
	const int32_t *chunk_first;          /* [n_items] first unit (chain-local) of each chunk */
	const int32_t *chunk_pred;           /* [n_items] the chunk in front of it in its chain (-1: the chain's first).  The two chains of an
	                                      *           interleaved stereo pair alternate chunk by chunk, so that L and R of the same stretch of
	                                      *           time are neighbouring lanes (see the write-out) */
	int chunk_units, warmup_units;
	unsigned long long *start_used;      /* [n_items] state each chunk was last decoded from (pack_state) */
	unsigned long long *chunk_end;       /* [n_items] state behind each chunk's last unit -- kept here, not read back from PCM that
	                                      *           sample_limit may have kept from being stored */
	int *changed;                        /* verify: set to 1 when any chunk was decoded again */
	const int *changed_before;           /* verify: the previous pass's word (NULL: first pass of a batch); 0 there = nothing to do */
} psxhip_adpcm_decode_job_t;
hipError_t psxhip_adpcm_decode_launch(const psxhip_adpcm_decode_job_t *j, int verify, int bits, void *stream);
hipError_t psxhip_adpcm_decode_final_launch(const int32_t *last_chunk, const unsigned long long *chunk_end, int n_chains,
                                            psxhip_adpcm_state_t *states, void *stream);

/* adpcm_sse_kernel: one lane per unit, one chain per blockIdx.x, `slices` workgroups stride over a chain's units */
typedef struct {
	const int16_t *a;
	const int16_t *b;
	const int16_t *a_tail;               /* optional: 28 samples per chain, what the decoder computed for the unit sample_limit cuts */
	const psxhip_adpcm_chain_t *chains;
	const int32_t *unit_base;            /* needed with unit_sse only */
	unsigned long long *unit_sse;        /* optional: one sum per record index */
	unsigned long long *chain_sums;      /* optional: [n_chains][2] = sum (a - b)^2, sum b^2 (zero before the launch) */
} psxhip_adpcm_sse_job_t;
hipError_t psxhip_adpcm_sse_launch(const psxhip_adpcm_sse_job_t *j, int n_chains, int slices, void *stream);

/* ---- sector_kernels.hip: unit records <-> XA sectors, the STR muxer's video sectors ---- */
/* builds the EDC tables and uploads them, once per device; PSXHIP_OK, or the error with its text set */
int psxhip_sector_tables(int device);

/* xa_assemble_kernel: one workgroup per sector, blockIdx.y walks n_streams streams of the same layout */
typedef struct {
	const uint8_t *units;
	int n_sectors, format, stereo, frequency, bits, file_number, channel_number, first_lba;
	const uint8_t *eof_flags;   /* optional: eof_flags[s] != 0 sets the EOF submode bit (adpcm.c:334-340) */
	uint32_t eof_bits;          /* ... or, without eof_flags, bit s for the first 32 sectors (the per-sector call: nothing to upload) */
	uint8_t *out;
	/* muxed streams (psxhip_str_encode_device): sector s goes to slot dst_sector[s] of the output -- its address (the header's time
	 * code, cdrom.c:61-65) is first_lba + that slot, like encode_file_str's sector counter (filefmt.c:450-503) -- and blockIdx.y
	 * walks independent streams with the same layout */
	const int32_t *dst_sector;  /* optional [n_sectors] */
	size_t units_stream_stride; /* bytes between the streams' unit records */
	size_t out_stream_stride;   /* bytes between the streams' outputs */
} psxhip_xa_job_t;
hipError_t psxhip_xa_assemble_launch(const psxhip_xa_job_t *j, int n_streams, void *stream);

/* str_video_sector_kernel: video sectors of muxed STR streams (tab[i]: see the kernel) */
typedef struct {
	const uint8_t *bs;                      /* the frames' bitstreams, bs_stride apart, the streams' bs_stream_stride apart */
	size_t bs_stride, bs_stream_stride;
	const psxhip_mdec_result_t *res;        /* [streams][frames_per_stream] */
	int frames_per_stream;
	const int4 *tab;
	int n_entries;
	int format;                             /* 6 STR, 7 STRCD, 9 STRV (format_t, args.h:45-58) */
	int sector_size;
	int xa_file, xa_channel, video_id, width, height;
	uint8_t *out;
	size_t out_stream_stride;
} psxhip_str_video_job_t;
hipError_t psxhip_str_video_sectors_launch(const psxhip_str_video_job_t *j, int n_streams, void *stream);

/* xa_disassemble_kernel: the inverse of xa_assemble_kernel, one workgroup per sector */
typedef struct {
	const uint8_t *sectors;
	int n_sectors, format, stereo, frequency, bits;
	uint8_t *units;
	int32_t *status;        /* optional */
	uint32_t eof_edc_delta; /* EDC of an all-zero span with 0x80 at sector bytes 18 and 22 */
} psxhip_xa_dis_job_t;
hipError_t psxhip_xa_disassemble_launch(const psxhip_xa_dis_job_t *j, void *stream);

/* ---- strspu_kernels.hip: the audio sectors of a muxed STRSPU stream ("psxhip STRSPU v1") ---- */
/* bumped with every change to strspu_kernels.hip */
#define PSXHIP_STRSPU_KERNEL_REV "strspu-k1.0"
/* strspu_audio_sector_kernel: one 128-lane workgroup per 2048-byte sector, one lane per 16 bytes: two for the chunk header, 126 for
 * the SPU blocks.  Record (u * channels + c) of a stream's units is unit u of channel c's chain (fill_interleaved_chains); the stream
 * holds n_sectors * 126 records, 16 bytes apart, 16-byte aligned.  Sector k goes to slot dst_sector[k] of its stream's output;
 * n_sectors is the K of the format: the last sector carries the trap block and the "last chunk" flag */
typedef struct {
	const uint8_t *units;
	int n_sectors, channels, frequency;
	uint32_t options;           /* strspu_options of psxhip_str_settings_t */
	uint8_t *out;               /* 4-byte aligned */
	const int32_t *dst_sector;  /* optional [n_sectors] */
	size_t units_stream_stride; /* bytes between the streams' unit records (a multiple of 16) */
	size_t out_stream_stride;   /* bytes between the streams' outputs (a multiple of 4) */
} psxhip_strspu_job_t;
hipError_t psxhip_strspu_audio_sectors_launch(const psxhip_strspu_job_t *j, int n_streams, void *stream);

#ifdef __cplusplus
}
#endif
