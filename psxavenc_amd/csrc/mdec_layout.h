// mdec_layout.h -- the LDS working sets of the MDEC encoder's two kernels, and the constants they rest on: what the frame kernel
// (mdec_kernels.hip) and the split kernel (mdec_split.inc) carve their LDS by, and what the host's plan (mdec_plan.cpp) sizes
// geometries, grids and workspaces by.  Constants and arithmetic only: the kernels and a host compiler read the same text (PSX_LAYOUT_HD: the
// pattern of mdec_search.h), so the two sides cannot drift apart.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bs_vlc_lut.h"

#if defined(__HIPCC__)
#define PSX_LAYOUT_HD __host__ __device__ inline
#else
#define PSX_LAYOUT_HD inline
#endif


// Two workgroup shapes: 12 wavefronts at 6 per SIMD (two frames per CU; 80 VGPRs) when two groups' LDS fits one CU,
// otherwise 16 wavefronts at 4 per SIMD (one frame per CU; 128 VGPRs) -- large frames / large budgets.
constexpr int kWavesSmall = 12, kOccSmall = 6;
constexpr int kWavesLarge = 16, kOccLarge = 4;
constexpr int kTileStride = 72;   // int16 per block in the transpose tile: 6 blocks land on disjoint LDS banks
constexpr int kZStride = 64;      // int16 per block in the coefficient tile: column-pass lane t stores its 8 outputs at bytes 16 t
constexpr int kPilotMax = 4;      // scales evaluated per pilot round
constexpr int kMaxTiles = 16;     // image tiles of 2048 dwords: budgets up to 128 KiB
constexpr uint32_t kNoMb = 0xFFFFu;   // pass order entry without a macroblock (the last round of tickets may be partial)

// scalars[] slots (LDS, per workgroup).  [0, S_KEEP0) are per-frame: cleared when a frame ends; [S_KEEP0, S_COUNT) live across frames.
enum {
    S_DC_BITS = 0,      // v3: sum of the DC code lengths
    S_STG_NEXT,         // staging bump allocator (dwords)
    S_FOREIGN,          // the hint this frame started with came from somewhere else than its neighbour in time (the group's previous run, the previous launch): its value, 0 if none -- what the trust policy learns from when the answer is known
    S_CNT_F,            // count pass: sum of AC code lengths
    S_CNT_D,            // count pass: sum of refinement deficits
    S_EMIT_BITS,        // emit pass: sum of macroblock stream lengths
    S_EMIT_D,           // emit pass: sum of refinement deficits
    S_NNZ,              // emit pass: non-zero AC coefficients
    S_PASS_COUNT,       // next pass: count scale
    S_PASS_EMIT,        // next pass: emit scale
    S_DONE,             // search finished
    S_RESULT,           // chosen scale (64 = nothing fits)
    S_TOTAL_BITS,       // bits of the staged stream incl. the end-of-frame code
    S_PILOT_N,          // scales in this pilot round (0 = pilot finished)
    S_PILOT_GUESS,
    S_PILOT_LO,
    S_PILOT_HI,
    S_CK_DONE,          // checkpoint: macroblocks finished so far in this pass
    S_MB_NEXT,          // pass tickets: next macroblock ticket to hand out
    S_CK_WAVES,         // checkpoint: wavefronts whose sums up to the quarter mark are in
    S_ABORT,            // checkpoint verdict: new guess | pass number << 8 (a verdict of an earlier pass is stale, not reset)
    S_ABORTS_LEFT,      // checkpoints still allowed for this frame
    S_RETRY,            // this frame came from the retry queue: the scale to start from (0: a fresh frame; -1: the queue is empty)
    S_DEFER,            // 1: the frame goes to the retry queue instead of into another pass here; 2: it starts over from the pilot (S_REPILOT)
    S_PILOTED,          // the pilot has run for this frame (its guess is a measurement, not somebody else's answer)
    S_CNT_BOUND,        // the pass (its number) whose count is a lower bound, not a total: counting stopped at its checkpoint (kStopCount)
    S_SEARCH,           // MdecSearch (14 ints)
    S_PILOT_SCALE0 = S_SEARCH + 14,    // [kPilotMax]
    S_PILOT_BITS0 = S_PILOT_SCALE0 + kPilotMax,   // [kPilotMax]
    S_TILE_FIRST0 = S_PILOT_BITS0 + kPilotMax,    // [kMaxTiles + 1] first macroblock whose stream starts in image tile t (see the merge)
    S_KEEP0 = S_TILE_FIRST0 + kMaxTiles + 1,
    S_FRAME = S_KEEP0,  // the frame TICKET in hand (ticket t is frame t), kNoTicket when no fresh one is left
    S_FIDX,             // index of the frame being encoded (the ticket's frame, or a frame taken from the retry queue)
    S_RUN_LEFT,         // always 0: a ticket is one frame.  It stays, with end_of_frame's `left > 0` arm and hand_on's term: read from LDS the compiler cannot fold it, and every form of the kernel without it spilled more in the 12-wavefront v3 shapes than tests/test_kernel_resources.py allows (NOTEBOOK, mdec-k3.8)
    S_PUSHED,           // the previous fresh frame of this group was handed on (see hand_on: whose hint the next frame starts from)
    S_QUEUE,            // drawn with the last frame's end when no fresh ticket is left: >= 0 the queue slot to take, -1 nothing will come, <= -2 wait for slot -2 - x
    S_HINT,             // the previous frame's answer in this group (0 = none): the pilot starts from it
    S_HINT_BUDGET,      // ... and its budget
    S_HINT_FRAME,       // ... and its index: the hint is the neighbour's answer when that is this frame's index - 1 (inside a run), foreign otherwise
    S_SHARED_HINT,      // answer | budget << 8 of the previous launch's last frame (by index)
    S_NEXT_DRAW,        // thread 0's ticket for the frame after this one, parked here over the passes (it is a register from the draw to the start of the next frame's passes: the atomic's round trip hides behind a frame's work, and the passes have no register to spare)
    S_REPILOT,          // the first pass, started from a hint, was stopped with a verdict FAR from the hint (a scene cut): the verdict.  The frame starts over from the pilot: one more turn of the frame loop for the same frame (taken back to 0 once the pilot has read it)
    S_DISTRUST,         // foreign hints are not trusted: frames without a neighbour's answer run the pilot (trust policy, below): bit 0 the launches before this one found them wrong more than one time in four, bits 8.. this group's foreign hints that failed in a row
    S_F_TRIED,          // foreign hints this group could judge (the frame's answer became known here)
    S_F_WRONG,          // ... and how many of them were not the answer
    S_P_TRIED,          // frames of this group whose first pass started from the PILOT's guess
    S_P_WRONG,          // ... and how many of those guesses were not the answer
    S_COUNT
};
static_assert((S_SEARCH % 2) == 0, "MdecSearch is read and written as 64-bit pairs");

constexpr int kWaveTileBytes = ((6 * kTileStride * 2 + 6 * kZStride * 2) + 15) / 16 * 16;   // transpose tile + coefficient tile
static_assert(kWaveTileBytes >= 384 * 4, "the per-wave code list (384 entries) aliases the tiles");

PSX_LAYOUT_HD int dc_chunks(int nmb) { return 2 * ((nmb + 63) >> 6) + ((4 * nmb + 63) >> 6); }

// LDS layout: everything whose size is known at compile time (given the workgroup shape) comes FIRST, at constant offsets --
// the compiler folds those addresses into the instructions' offset fields, where run-time offsets each took a scalar register
// (sixteen base addresses in a kernel that spills a hundred scalar registers) -- then the arrays sized by the geometry.
PSX_LAYOUT_HD constexpr size_t lds_fixed_bytes(int waves) {
    size_t b = 0;
    b += (size_t)S_COUNT * 4;             // scalars
    b += BS_LUT_SIZE * 2;                 // ac_len16
    b = (b + 3) & ~(size_t)3;
    b += BS_LUT_SIZE * 4;                 // ac_code
    b += 32;                              // dc tables
    b = (b + 15) & ~(size_t)15;
    b += 2 * 64 * 16 + 2 * 64;            // per-lane constant tables, scan-position table, quant matrix
    b += (size_t)waves * kWaveTileBytes;  // tiles
    return (b + 15) & ~(size_t)15;
}
PSX_LAYOUT_HD size_t lds_bytes(int nmb, int out_words, int stg_words, int waves) {
    size_t b = lds_fixed_bytes(waves);
    b += (size_t)out_words * 4;
    b += (size_t)stg_words * 4;
    b += (size_t)nmb * 4;         // rec
    b += (size_t)nmb * 4;         // mb_off
    b += (size_t)dc_chunks(nmb) * 16;   // dc_fn
    b += (size_t)nmb * 6 * 2;     // dcv
    return (b + 15) & ~(size_t)15;
}

// ---- the split kernel (mdec_split.inc)
constexpr int kSplitWaves = 16, kSplitThreads = kSplitWaves * 64;
constexpr int kSplitRound = 16;              // scales evaluated per round (eight in a first round that has a low hint)
constexpr int kSplitRounds = 5;              // 8 + 4 x 16 >= 63
// a macroblock's stream is at most 6 x (DC code <= 24 bits + 63 escapes + end of block) bits, + the end-of-frame code, + slack
constexpr int kSplitMbMaxBits = 6 * (24 + 63 * 22 + 2);
constexpr int kSplitWbufWords = (kSplitMbMaxBits + 10 + 31) / 32 + 2;
static_assert(kSplitWbufWords * 4 >= 6 * kTileStride * 2, "a wavefront's transpose tile fits its stream buffer");
constexpr unsigned long long kSplitPatience = 20000000ull;    // ticks of the 100 MHz wall clock a rendezvous waits: 0.2 s (default)

PSX_LAYOUT_HD int split_dc_chunks(int nmb) { return 2 * ((nmb + 511) >> 9) + ((4 * nmb + 511) >> 9); }
PSX_LAYOUT_HD size_t split_lds_bytes(int codec, int M, int nmb) {
    size_t b = 0;
    b += 96 * 4;                                        // scalars
    b += (BS_LUT_SIZE * 2 + 15) & ~15;                  // ac_len16
    b += (BS_LUT_SIZE * 4 + 15) & ~15;                  // ac_code
    b += (size_t)M * 6 * 64 * 2;                        // coefficients, scan order
    b += (size_t)M * kSplitRound * 4;                   // macroblock bits per scale of the round
    b += (size_t)M * 8 * 2;                             // quantised DC of the segment's blocks
    b += (size_t)kSplitWaves * kSplitWbufWords * 4;     // per-wavefront stream buffers (the transpose tiles alias them)
    if (codec != 0) {
        b += ((size_t)nmb * 6 * 2 + 15) & ~15;          // the frame's DC terms / deltas
        b += (size_t)split_dc_chunks(nmb) * 16;         // chain scan
    }
    return (b + 15) & ~(size_t)15;
}
