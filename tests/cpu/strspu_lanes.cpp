// tests/cpu/strspu_lanes.cpp -- TEST INFRASTRUCTURE: runs the text of psxavenc_amd/csrc/strspu_kernels.hip itself, lane by lane, on
// the CPU under -fsanitize=address,undefined (tests/test_strspu_lanes_cpu.py), behind the stand-in
// tests/cpu/hip_lanes/hip/hip_runtime.h.  The kernel loads a 16-byte record in every lane and selects afterwards -- the header lanes
// and the leading dummy block drop what they loaded -- so a record index outside the stream's units changes no output byte; here
// it is a sanitizer report.  A program, not a library.
//
//   strspu_lanes <in> <out> <order: 0 ascending, 1 descending, 2 shuffled> [seed]
// in:  records of eleven int32 {n_sectors, channels, frequency, options, n_streams, units_stream_stride, has_slots, n_slots,
//      out_stream_stride, out_offset, fill}, then n_sectors int32 of destination slots when has_slots, then
//      n_streams * units_stream_stride bytes of unit records
// out: per record the whole destination, (n_streams - 1) * out_stream_stride + n_slots * 2048 bytes, which held `fill` before
// The units are one heap block that ends with the last record include/psxav_hip.h promises the call reads: a channel has
// U = n_sectors * 126 / channels - 1 units (one more with PSXHIP_STRSPU_NO_LEADING_DUMMY), "records behind them are not read", so
// the block is (n_streams - 1) * units_stream_stride + U * channels * 16 bytes.  The destination is a block of its own of the size
// above, out_offset bytes (4: it is promised 4-byte alignment and no more) into an allocation whose first bytes must keep `fill`.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../psxavenc_amd/csrc/strspu_kernels.hip"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    hip_lanes::order = atoi(argv[3]);
    if (argc > 4) hip_lanes::seed = strtoull(argv[4], nullptr, 10);
    int32_t head[11];
    while (fread(head, sizeof head, 1, in) == 1) {
        psxhip_strspu_job_t j;
        memset(&j, 0, sizeof j);
        j.n_sectors = head[0]; j.channels = head[1]; j.frequency = head[2]; j.options = (uint32_t)head[3];
        const int S = head[4], has_slots = head[6], n_slots = head[7], fill = head[10], K = j.n_sectors;
        j.units_stream_stride = (size_t)head[5]; j.out_stream_stride = (size_t)head[8];
        const size_t offset = (size_t)head[9];
        // the rules of psxhip_strspu_audio_sectors_device
        if (K < 1 || S < 1 || S > 65535 || (j.channels != 1 && j.channels != 2) || j.frequency <= 0 || n_slots < K) return 3;
        if ((j.options & ~(uint32_t)(PSXHIP_STRSPU_ID_MASK | PSXHIP_STRSPU_LOOP | PSXHIP_STRSPU_NO_LEADING_DUMMY)) || (j.units_stream_stride & 15) ||
            ((j.out_stream_stride | offset) & 3))
            return 3;
        if (S > 1 && (j.units_stream_stride < (size_t)K * 126 * 16 || (!has_slots && j.out_stream_stride < (size_t)K * 2048))) return 3;
        const size_t U = (size_t)K * (126 / j.channels) - ((j.options & PSXHIP_STRSPU_NO_LEADING_DUMMY) ? 0 : 1);
        const size_t units_size = (size_t)(S - 1) * j.units_stream_stride + U * j.channels * 16;
        const size_t dst_size = (size_t)(S - 1) * j.out_stream_stride + (size_t)n_slots * 2048;
        int32_t* slots = has_slots ? (int32_t*)malloc((size_t)K * sizeof(int32_t)) : nullptr;
        uint8_t* all = (uint8_t*)malloc((size_t)S * j.units_stream_stride);
        uint8_t* units = (uint8_t*)malloc(units_size);
        uint8_t* block = (uint8_t*)malloc(offset + dst_size);
        if (!all || !units || !block || (has_slots && !slots)) return 4;
        if (has_slots && fread(slots, sizeof(int32_t), (size_t)K, in) != (size_t)K) return 4;
        for (int k = 0; has_slots && k < K; k++)
            if (slots[k] < 0 || slots[k] >= n_slots) return 3;
        if (fread(all, 1, (size_t)S * j.units_stream_stride, in) != (size_t)S * j.units_stream_stride) return 4;
        if (units_size > (size_t)S * j.units_stream_stride) return 3;
        memcpy(units, all, units_size);
        free(all);
        memset(block, fill, offset + dst_size);
        j.units = units; j.out = block + offset; j.dst_sector = slots;
        if (psxhip_strspu_audio_sectors_launch(&j, S, nullptr) != hipSuccess) return 6;
        for (size_t i = 0; i < offset; i++)
            if (block[i] != (uint8_t)fill) return 7;
        if (fwrite(block + offset, 1, dst_size, out) != dst_size) return 5;
        free(slots);
        free(units);
        free(block);
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
