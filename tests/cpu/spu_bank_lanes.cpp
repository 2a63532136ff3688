// tests/cpu/spu_bank_lanes.cpp -- TEST INFRASTRUCTURE: runs the text of psxavenc_amd/csrc/spu_bank_kernels.hip on the CPU under
// -fsanitize=address,undefined (tests/test_spu_bank_lanes_cpu.py), behind the wavefront model of the stand-in tests/cpu/hip_lanes
// (the check kernel reduces a wavefront's bits with wave_ops.h).  The rows and tiles the kernels read are built by the plan module's
// own text (spu_bank_plan.cpp).  A record is one launch of the frame kernel (kind 0) or of the check kernel (kind 1) through its
// launch function.  A program, not a library.
//
//   spu_bank_lanes <in> <out> <order: 0 ascending, 1 descending, 2 shuffled> [seed]
// in:  records of 8 int32 {kind, format, alignment, no_leading_dummy, bank_alignment, n, guard, fill}; n x psxhip_spu_bank_entry_t;
//      the bank's `total` bytes (kind 0: what the encoder left in a buffer of `fill`; kind 1: the bank to check)
// out: kind 0: guard + total + guard bytes, the guards having held `fill`; kind 1: n int32 of status, zeroed before the launch
// The rows and the tiles are heap blocks of their own that end with their last element; so is the bank of kind 1, which is only
// read.  `guard` is a multiple of 16.
#define HIP_LANES_WAVES 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip_lanes/psxhip_api_standin.h"

#include "../../psxavenc_amd/csrc/spu_bank_kernels.hip"
#include "../../psxavenc_amd/csrc/spu_bank_plan.cpp"

namespace {
void* block16(size_t bytes) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 16)) exit(4);
    return p;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    hip_lanes::order = atoi(argv[3]);
    if (argc > 4) hip_lanes::seed = strtoull(argv[4], nullptr, 10);
    int32_t head[8];
    while (fread(head, sizeof head, 1, in) == 1) {
        const int kind = head[0], n = head[5], guard = head[6], fill = head[7];
        const psxhip_spu_bank_settings_t s = {head[1], head[2], head[3], head[4], 0};
        if (kind < 0 || kind > 1 || n < 1 || n > 65535 || guard < 0 || guard % 16) return 3;
        std::vector<psxhip_spu_bank_entry_t> entries((size_t)n);
        if (fread(entries.data(), sizeof(psxhip_spu_bank_entry_t), (size_t)n, in) != (size_t)n) return 4;
        SpuBankPlan p;
        if (spu_bank_plan_build(&s, entries.data(), n, 0x7FFFFFFF, &p)) {
            fprintf(stderr, "the plan refused the bank: %s\n", psxhip_last_error());
            return 6;
        }
        const size_t total = (size_t)p.total, row_bytes = sizeof(psxhip_spu_bank_row_t) * (size_t)n;
        auto* rows = (psxhip_spu_bank_row_t*)block16(row_bytes);
        memcpy(rows, p.rows.data(), row_bytes);
        if (kind == 0) {
            uint8_t* all = (uint8_t*)block16(total + 2 * (size_t)guard);
            memset(all, fill, total + 2 * (size_t)guard);
            if (total && fread(all + guard, 1, total, in) != total) return 4;
            psxhip_spu_bank_frame_job_t job = {rows, n, all + guard};
            if (psxhip_spu_bank_frame_launch(&job, nullptr) != hipSuccess) return 6;
            if (fwrite(all, 1, total + 2 * (size_t)guard, out) != total + 2 * (size_t)guard) return 5;
            free(all);
        } else {
            uint8_t* bank = (uint8_t*)block16(total);
            if (total && fread(bank, 1, total, in) != total) return 4;
            const size_t tile_bytes = sizeof(psxhip_spu_bank_tile_t) * p.tiles.size();
            auto* tiles = (psxhip_spu_bank_tile_t*)block16(tile_bytes);
            memcpy(tiles, p.tiles.data(), tile_bytes);
            auto* status = (int32_t*)block16(sizeof(int32_t) * (size_t)n);
            memset(status, 0, sizeof(int32_t) * (size_t)n);
            psxhip_spu_bank_check_job_t job = {rows, tiles, (int)p.tiles.size(), bank, status};
            if (job.n_tiles && psxhip_spu_bank_check_launch(&job, nullptr) != hipSuccess) return 6;
            if (fwrite(status, sizeof(int32_t), (size_t)n, out) != (size_t)n) return 5;
            free(status);
            free(tiles);
            free(bank);
        }
        free(rows);
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
