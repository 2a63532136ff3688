// tests/cpu/ingest_lanes.cpp -- TEST INFRASTRUCTURE: runs the text of psxavenc_amd/csrc/ingest_kernels.hip itself, lane by lane, on
// the CPU under -fsanitize=address,undefined (tests/test_ingest_lanes_cpu.py), behind the stand-in tests/cpu/hip_lanes/hip/hip_runtime.h.
// What ingest_sim.cpp cannot see is here: which addresses a lane touches -- fetch<> and store<> choosing whole dwords or bytes, the
// clamped neighbours of the bilinear mix, the ragged tail of a workgroup.  A program, not a library.
//
//   ingest_lanes <in> <out> <order: 0 ascending, 1 descending, 2 shuffled> [seed]
// in:  records of ingest_sim.cpp's 21 int32 {src_format, width, height, offset and pitch of planes 0, 1, 2, cy, rv, gu, gv, bu, yoff,
//      coff, out_format, options, n_pictures, src_stride, picture_bytes} and four more {n_out, out_stride, has_index, fill}, then
//      n_out int32 of index when has_index, then n_pictures * src_stride bytes
// out: per record the whole destination, (n_out - 1) * out_stride + output bytes, which held `fill` in every byte before the call
// The source is one heap block of (n_pictures - 1) * src_stride + the picture's bytes, the destination one of the size above and the
// index one of n_out words: the smallest the argument rules of psxhip_ingest_convert_device accept, so that a read or a store one
// byte outside any of them -- one whose value is masked away included -- is the sanitizer's to report, and so is a whole-dword access
// at an address that is no multiple of four.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../psxavenc_amd/csrc/ingest_kernels.hip"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    hip_lanes::order = atoi(argv[3]);
    if (argc > 4) hip_lanes::seed = strtoull(argv[4], nullptr, 10);
    int32_t head[25];
    while (fread(head, sizeof head, 1, in) == 1) {
        psxhip_ingest_job_t j = {};
        IngestDesc& d = j.d;
        d.f = ingest_format(head[0]);
        d.w = head[1]; d.h = head[2];
        if (d.f.layout < 0 || d.w < 1 || d.h < 1) return 3;
        size_t src_bytes = 0;                                  // psxhip_ingest_source_bytes: to the end of the last plane
        for (int p = 0; p < d.f.planes; p++) {
            d.off[p] = (uint32_t)head[3 + 2 * p];
            d.pitch[p] = (uint32_t)head[4 + 2 * p];
            const size_t row = ing_row_bytes(d, p), end = d.off[p] + (size_t)(ing_plane_rows(d, p) - 1) * d.pitch[p] + row;
            if (d.pitch[p] < row || (d.f.bytes == 2 && ((d.off[p] | d.pitch[p]) & 1))) return 3;
            if (end > src_bytes) src_bytes = end;
        }
        d.cy = head[9]; d.rv = head[10]; d.gu = head[11]; d.gv = head[12]; d.bu = head[13]; d.yoff = head[14]; d.coff = head[15];
        j.out_format = head[16];
        d.bilinear = (head[17] & ING_CHROMA_BILINEAR) ? 1 : 0;
        const int n = head[18], n_out = head[21], has_index = head[23], fill = head[24];
        const size_t stride = (size_t)head[19], out_stride = (size_t)head[22];
        const size_t out_bytes = j.out_format == ING_OUT_RGB24 ? (size_t)d.w * d.h * 3 : (size_t)d.w * d.h * 3 / 2;
        // the rules of psxhip_ingest_create and ingest_check; the statement's layout gives the same picture bytes
        if (j.out_format == ING_OUT_YUV420P && (((d.w | d.h) & 1) || d.f.layout == ING_RGB)) return 3;
        if (d.f.layout == ING_PACKED422 && (d.w & 1)) return 3;
        if ((size_t)head[20] != src_bytes || n < 1 || n_out < 1 || stride < src_bytes || out_stride < out_bytes) return 3;
        if (d.f.bytes == 2 && (stride & 1)) return 3;
        const size_t src_size = (size_t)(n - 1) * stride + src_bytes, dst_size = (size_t)(n_out - 1) * out_stride + out_bytes;
        int32_t* index = has_index ? (int32_t*)malloc((size_t)n_out * sizeof(int32_t)) : nullptr;
        uint8_t* all = (uint8_t*)malloc((size_t)n * stride);
        uint8_t* src = (uint8_t*)malloc(src_size);
        uint8_t* dst = (uint8_t*)malloc(dst_size);
        if (!all || !src || !dst || (has_index && !index)) return 4;
        if (has_index && fread(index, sizeof(int32_t), (size_t)n_out, in) != (size_t)n_out) return 4;
        if (fread(all, 1, (size_t)n * stride, in) != (size_t)n * stride) return 4;
        memcpy(src, all, src_size);
        free(all);
        memset(dst, fill, dst_size);
        j.d_src = src; j.src_stride = stride; j.n_src = n; j.d_src_index = index; j.first = 0; j.n_out = n_out;
        j.d_out = dst; j.out_stride = out_stride;
        if (psxhip_ingest_launch(&j, nullptr) != hipSuccess) return 6;
        if (fwrite(dst, 1, dst_size, out) != dst_size) return 5;
        free(index);
        free(src);
        free(dst);
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
