// spu_bank_plan.h -- what the sound bank ("psxhip SPU bank v1"; include/psxav_hip.h, psxhip_spu_bank_*) derives
// from its settings and entry list alone: what it refuses, with which text and in which order, where every file lies, the row per
// entry the kernels read, the chain table the ADPCM encoder and decoder run under, the check kernel's tiles, whether the encode is
// serial or cut along time, and the seam tables of "psxhip SPU loop seam v1" (DESIGN.md section 24).  Arithmetic and refusals only (no HIP), like reader_plan.h and str_plan.h: spu_bank_plan.cpp builds with
// a host compiler alone and links against nothing but psxhip_set_error (tests/test_spu_bank_plan_cpu.py does so, under the host
// sanitizers); psxhip_spu_bank.cpp only executes the plan.  The file framing itself is spu_file_layout.h's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/psxav_hip.h"

/* One entry as the kernels see it (spu_bank_kernels.hip).  A bank is counted in 16-byte words: a block, a third of a header.  The
 * entry's words that are NOT data blocks, in file order, are its "frame words": header_words + dummy in front of the data blocks,
 * then everything from the first word behind them to end_word (the trap block when `trap`, the file's padding, the gap up to the
 * next file or to the bank's end). */
typedef struct {
	int32_t first_word;         /* the file's offset / 16 */
	int32_t header_words;       /* 3 (VAG) or 0 */
	int32_t dummy;              /* 1: a leading zero block */
	int32_t data_blocks;
	int32_t trap;               /* 1: the block behind the data is the trap block */
	int32_t end_word;           /* the next file's first word, or total / 16 */
	int32_t loop_start_block;   /* the data block whose byte 1 takes LOOP_START, or -1 */
	int32_t loop_repeat;        /* 1: LOOP_REPEAT into byte 1 of the last data block (there is one) */
	uint32_t header[12];        /* VAG: the 48 header bytes as they lie */
} psxhip_spu_bank_row_t;

/* One workgroup's share of spu_bank_check_kernel: part 0 = frame words [first, first + count) of the entry, part 1 = its data
 * blocks [first, first + count) */
typedef struct {
	int32_t entry, part, first, count;
} psxhip_spu_bank_tile_t;

/* One entry as the seam report sees it ("psxhip SPU loop seam v1"; spu_seam_kernels.hip) */
typedef struct {
	int64_t pcm_offset;         /* the entry's first sample in the PCM buffer */
	int32_t samples;
	int32_t first_block;        /* record index of the first data block */
	int32_t data_blocks;        /* D */
	int32_t seam_block;         /* S, or -1 */
} psxhip_spu_seam_row_t;

#ifdef __cplusplus
#pragma GCC visibility push(hidden)

constexpr int kSpuBankTile = 4096;          // words or blocks per tile at the most

struct SpuBankPlan {
    psxhip_spu_bank_settings_t settings;
    int n = 0;
    int64_t total = 0;                                  // bytes
    std::vector<int64_t> offsets, sizes;                // [n]
    std::vector<psxhip_spu_bank_row_t> rows;            // [n]
    // entry i's chain: its samples in the PCM buffer, its data blocks as records of the bank (encode and decode alike); an entry
    // without samples keeps its place with n_units = 0, which the chain kernels pass over (adpcm_kernels.hip: the unit loop runs
    // to the wavefront's longest chain and masks the rest)
    std::vector<psxhip_adpcm_chain_t> chains;           // [n]
    std::vector<int32_t> unit_base;                     // [n] record index of the first data block
    std::vector<psxhip_spu_bank_tile_t> tiles;
    int64_t pcm_elements = 0;                           // max over entries of pcm_offset + samples
    int64_t total_units = 0;
    int max_units = 0;                                  // the longest entry's
    bool chunked = false;                               // max_units >= the threshold given

    // "psxhip SPU loop seam v1": the seam block per entry (-1: none) and the report's rows
    std::vector<int32_t> seam_block;                    // [n]
    std::vector<psxhip_spu_seam_row_t> seam_rows;       // [n]
    // mode STEADY's chain table, in place over the bank like `chains`.  First, in entry order, what is encoded once from a zero
    // state: the intro (units 0 .. S-1) of every entry with S > 0 and the whole chain of every entry without a seam block; behind
    // them, in entry order, the body (units S .. D-1) of every entry with a seam block.  A chain's state slot is its index.
    std::vector<psxhip_adpcm_chain_t> seam_chains;      // [seam_first + seam_body]
    std::vector<int32_t> seam_unit_base;                // likewise
    int seam_first = 0, seam_body = 0;
    std::vector<int32_t> seam_body_entry;               // [seam_body] the entry a body chain belongs to
    std::vector<int32_t> seam_body_intro;               // [seam_body] the state slot of its intro chain, or -1: S = 0, s_0 = (0, 0)
};

// the one-file settings entry e amounts to
psxhip_spu_file_settings_t spu_bank_file_settings(const psxhip_spu_bank_settings_t* s, const psxhip_spu_bank_entry_t* e);
// PSXHIP_OK, or PSXHIP_EINVAL with the text set.  chunked_threshold: psxhip_adpcm_chunked_threshold(n), the caller's to ask
int spu_bank_plan_build(const psxhip_spu_bank_settings_t* s, const psxhip_spu_bank_entry_t* entries, int n, int chunked_threshold,
                        SpuBankPlan* p);
// the seam block of an entry with `data_blocks` data blocks, or -1 (the rule is stated in include/psxav_hip.h)
int64_t spu_bank_seam_block(const psxhip_spu_file_settings_t* f, int64_t data_blocks);
// the frame words of a row
static inline int64_t spu_bank_frame_words(const psxhip_spu_bank_row_t& r) {
    return (int64_t)r.header_words + r.dummy + ((int64_t)r.end_word - ((int64_t)r.first_word + r.header_words + r.dummy + r.data_blocks));
}

#pragma GCC visibility pop
#endif
