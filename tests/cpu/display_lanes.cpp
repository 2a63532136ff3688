// tests/cpu/display_lanes.cpp -- TEST INFRASTRUCTURE: runs the text of psxavenc_amd/csrc/display_kernels.hip itself, lane by lane,
// on the CPU under -fsanitize=address,undefined (tests/test_display_lanes_cpu.py), behind the stand-in
// tests/cpu/hip_lanes/hip/hip_runtime.h.  What display_sim.cpp cannot see is here: which addresses a lane touches -- the dwords left
// and right of its own that chroma_hmix loads, the rows above and below, the tail of the last workgroup.  A program, not a library.
//
//   display_lanes <in> <out> <order: 0 ascending, 1 descending, 2 shuffled> [seed]
// in:  records of display_sim.cpp's five int32 {width, height, n_frames, out_format, options} and six more {frame_stride, dst_pitch,
//      dst_stride, dst_offset, has_records, fill}, then n_frames decoder records of four int32 when has_records, then
//      n_frames * frame_stride bytes (NV21 frames, frame_stride apart)
// out: per record the whole destination, (n_frames - 1) * dst_stride + (height - 1) * dst_pitch + row bytes, which held `fill` before
// The frames are one heap block of (n_frames - 1) * frame_stride + width * height * 3 / 2 bytes and the destination one of the size
// above: the smallest psxhip_display_check accepts, so that a read or a store outside either is the sanitizer's to report.  With
// dst_offset (4, 8, 12: a destination that is 4-byte aligned and no more) the block is that much longer in front; those bytes must
// still hold `fill` afterwards.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../psxavenc_amd/csrc/display_kernels.hip"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    hip_lanes::order = atoi(argv[3]);
    if (argc > 4) hip_lanes::seed = strtoull(argv[4], nullptr, 10);
    int32_t head[11];
    while (fread(head, sizeof head, 1, in) == 1) {
        psxhip_display_job_t j = {};
        j.width = head[0]; j.height = head[1]; j.n_frames = head[2]; j.out_format = head[3]; j.options = (uint32_t)head[4];
        j.frame_stride = (size_t)head[5]; j.dst_pitch = (size_t)head[6]; j.dst_stride = (size_t)head[7];
        const size_t offset = (size_t)head[8];
        const int has_records = head[9], fill = head[10], n = j.n_frames;
        // the rules of psxhip_display_check
        const size_t row = (size_t)disp_row_bytes(j.out_format, j.width);
        if (j.width < 16 || j.height < 16 || j.width > 1024 || j.height > 1024 || (j.width & 15) || (j.height & 15) || n < 1 || !row) return 3;
        if ((j.options & ~7u) || (j.out_format != PSXHIP_OUT_RGB555 && (j.options & (PSXHIP_DISPLAY_DITHER | PSXHIP_DISPLAY_MASK_BIT)))) return 3;
        const size_t frame_bytes = (size_t)j.width * j.height * 3 / 2, picture = (size_t)(j.height - 1) * j.dst_pitch + row;
        if ((j.frame_stride & 3) || j.frame_stride < frame_bytes || ((j.dst_pitch | j.dst_stride | offset) & 3) || j.dst_pitch < row || j.dst_stride < picture) return 3;
        const size_t src_size = (size_t)(n - 1) * j.frame_stride + frame_bytes, dst_size = (size_t)(n - 1) * j.dst_stride + picture;
        psxhip_mdec_decoded_t* records = has_records ? (psxhip_mdec_decoded_t*)malloc((size_t)n * sizeof(psxhip_mdec_decoded_t)) : nullptr;
        uint8_t* all = (uint8_t*)malloc((size_t)n * j.frame_stride);
        uint8_t* frames = (uint8_t*)malloc(src_size);
        uint8_t* block = (uint8_t*)malloc(offset + dst_size);
        if (!all || !frames || !block || (has_records && !records)) return 4;
        if (has_records && fread(records, sizeof(psxhip_mdec_decoded_t), (size_t)n, in) != (size_t)n) return 4;
        if (fread(all, 1, (size_t)n * j.frame_stride, in) != (size_t)n * j.frame_stride) return 4;
        memcpy(frames, all, src_size);
        free(all);
        memset(block, fill, offset + dst_size);
        j.d_frames = frames; j.d_decoded = records; j.d_dst = block + offset;
        if (psxhip_display_launch(&j, nullptr) != hipSuccess) return 6;
        for (size_t i = 0; i < offset; i++)
            if (block[i] != (uint8_t)fill) return 7;
        if (fwrite(block + offset, 1, dst_size, out) != dst_size) return 5;
        free(records);
        free(frames);
        free(block);
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
