// spu_bank_kernels.hip -- the framing of a sound bank on the device for MI355X (gfx950), hand-written HIP ("psxhip SPU bank v1",
// DESIGN.md section 23; the file rule is encode_file_spu's, filefmt.c:212-293, as spu_file_layout.h states it).  The ADPCM encoder
// has written every entry's data blocks where they belong; spu_bank_frame_kernel writes everything else -- header, leading dummy
// block, trap block, padding and the gap up to the next file -- and ORs the loop flags into the data blocks; spu_bank_check_kernel
// is its inverse and reports per entry what is not as the rule has it.  Both read one row per entry that the plan built
// (spu_bank_plan.h).  No LDS, no tables: 16-byte loads and stores, one atomic OR per wavefront that has something to report.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/psxav_audio.h"
#include "psxhip_spu_bank_internal.h"
#include "wave_ops.h"

namespace {

// Frame word i of an entry (spu_bank_plan.h): the bank word it is, what the rule puts there, and the status bit that judges it
struct FrameWord {
    int word;
    int bit;
    uint4 want;
};

__device__ __forceinline__ FrameWord frame_word(const psxhip_spu_bank_row_t* row, int i) {
    const int header_words = row->header_words, head = header_words + row->dummy;
    FrameWord f;
    f.want = make_uint4(0u, 0u, 0u, 0u);
    if (i < head) {
        f.word = row->first_word + i;
        f.bit = i < header_words ? PSXHIP_SPU_BANK_STATUS_HEADER : PSXHIP_SPU_BANK_STATUS_DUMMY;
        if (i < header_words) f.want = ((const uint4*)row->header)[i];
    } else {                                                            // behind the data blocks: trap, padding, gap
        const bool trap = row->trap && i == head;
        f.word = row->first_word + row->data_blocks + i;
        f.bit = trap ? PSXHIP_SPU_BANK_STATUS_TRAP : PSXHIP_SPU_BANK_STATUS_PADDING;
        if (trap) f.want.x = (uint32_t)PSX_AUDIO_SPU_LOOP_TRAP << 8;    // byte 1, the rest zero (filefmt.c:271-278)
    }
    return f;
}

__device__ __forceinline__ int frame_word_count(const psxhip_spu_bank_row_t* row) {
    return row->end_word - row->first_word - row->data_blocks;
}

__global__ __launch_bounds__(64) void spu_bank_frame_kernel(const psxhip_spu_bank_frame_job_t job) {
    const int lane = (int)threadIdx.x;
    const psxhip_spu_bank_row_t* row = job.rows + blockIdx.x;
    const int count = frame_word_count(row);
    uint4* out = (uint4*)job.out;
    for (int i = lane; i < count; i += 64) {
        const FrameWord f = frame_word(row, i);
        out[f.word] = f.want;
    }
    // the loop flags, into byte 1 of blocks the encoder wrote with a zero there (filefmt.c:251-254): one lane, in order -- both may
    // fall into the same block
    if (lane == 0) {
        uint8_t* data = job.out + 16ll * (row->first_word + row->header_words + row->dummy);
        const int start = row->loop_start_block;
        if (start >= 0) data[16ll * start + 1] |= (uint8_t)PSX_AUDIO_SPU_LOOP_START;
        if (row->loop_repeat) data[16ll * (row->data_blocks - 1) + 1] |= (uint8_t)PSX_AUDIO_SPU_LOOP_REPEAT;
    }
}

__global__ __launch_bounds__(256) void spu_bank_check_kernel(const psxhip_spu_bank_check_job_t job) {
    const psxhip_spu_bank_tile_t tile = job.tiles[blockIdx.x];
    const psxhip_spu_bank_row_t* row = job.rows + tile.entry;
    int bits = 0;
    if (tile.part == 0) {
        const uint4* bank = (const uint4*)job.bank;
        for (int k = (int)threadIdx.x; k < tile.count; k += 256) {
            const FrameWord f = frame_word(row, tile.first + k);
            const uint4 v = bank[f.word];
            if (v.x != f.want.x || v.y != f.want.y || v.z != f.want.z || v.w != f.want.w) bits |= f.bit;
        }
    } else {
        const uint8_t* data = job.bank + 16ll * (row->first_word + row->header_words + row->dummy);
        const int start = row->loop_start_block, last = row->loop_repeat ? row->data_blocks - 1 : -1;
        for (int k = (int)threadIdx.x; k < tile.count; k += 256) {
            const int b = tile.first + k;
            const int want = (b == start ? (int)PSX_AUDIO_SPU_LOOP_START : 0) | (b == last ? (int)PSX_AUDIO_SPU_LOOP_REPEAT : 0);
            if ((int)data[16ll * b + 1] != want) bits |= PSXHIP_SPU_BANK_STATUS_FLAGS;
        }
    }
    // a wavefront's bits, one ballot each; one atomic per wavefront that found something
    int found = 0;
#pragma unroll
    for (int bit = 1; bit <= PSXHIP_SPU_BANK_STATUS_PADDING; bit <<= 1)
        if (wave::ballot((bits & bit) != 0)) found |= bit;
    if (wave::lane_id() == 0 && found) atomicOr(&job.status[tile.entry], found);
}

}  // namespace

extern "C" hipError_t psxhip_spu_bank_frame_launch(const psxhip_spu_bank_frame_job_t* j, void* stream) {
    hipLaunchKernelGGL(spu_bank_frame_kernel, dim3((unsigned)j->n_entries), dim3(64), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}

extern "C" hipError_t psxhip_spu_bank_check_launch(const psxhip_spu_bank_check_job_t* j, void* stream) {
    hipLaunchKernelGGL(spu_bank_check_kernel, dim3((unsigned)j->n_tiles), dim3(256), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}
