// tests/cpu/synth_lanes.cpp -- TEST INFRASTRUCTURE: runs the text of psxavenc_amd/csrc/synth_kernels.hip itself, lane by lane, on the
// CPU under -fsanitize=address,undefined (tests/test_synth_lanes_cpu.py), behind the stand-in tests/cpu/hip_lanes/hip/hip_runtime.h:
// the index arithmetic of the two generators -- which frame and dword, which sample, and where the last workgroup stops -- over heap
// blocks of exactly the bytes a call owns.  A program, not a library.
//
//   synth_lanes <in> <out> <order: 0 ascending, 1 descending, 2 shuffled> [seed]
// in:  records of nine int32, either {0, width, height, seed, first_frame, n_frames, noise_amp, frame_stride, fill}
//      or {1, seed, chain, first_sample low word, high word, n, kind, pitch, fill}
// out: per record the whole destination, which held `fill` in every byte before: (n_frames - 1) * frame_stride + width * height * 3 / 2
//      bytes, or (n - 1) * pitch + 1 samples of 16 bits
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../psxavenc_amd/csrc/synth_kernels.hip"

// what the entry points call besides their kernels (psxhip_api.cpp's, which need a device): the error text goes to stderr, which
// the test wants empty
extern "C" void psxhip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
int psxhip_ensure_device(int) { return PSXHIP_OK; }

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    hip_lanes::order = atoi(argv[3]);
    if (argc > 4) hip_lanes::seed = strtoull(argv[4], nullptr, 10);
    int32_t head[9];
    while (fread(head, sizeof head, 1, in) == 1) {
        const int fill = head[8];
        size_t size;
        uint8_t* block;
        if (head[0] == 0) {
            const int w = head[1], h = head[2], n = head[5];
            const size_t stride = (size_t)head[7];
            if (w < 16 || h < 16 || n < 1 || stride < (size_t)w * h * 3 / 2) return 3;
            size = (size_t)(n - 1) * stride + (size_t)w * h * 3 / 2;
            if (!(block = (uint8_t*)malloc(size))) return 4;
            memset(block, fill, size);
            if (psxhip_synth_frames_device(0, block, stride, w, h, (uint32_t)head[3], (uint32_t)head[4], n, head[6], nullptr) != PSXHIP_OK) return 6;
        } else {
            const int64_t first = (int64_t)(((uint64_t)(uint32_t)head[4] << 32) | (uint32_t)head[3]), n = head[5];
            const int pitch = head[7];
            if (n < 1 || pitch < 1) return 3;
            size = ((size_t)(n - 1) * pitch + 1) * sizeof(int16_t);
            if (!(block = (uint8_t*)malloc(size))) return 4;
            memset(block, fill, size);
            if (psxhip_synth_pcm_device(0, (int16_t*)block, (uint32_t)head[1], (uint32_t)head[2], first, n, head[6], pitch, nullptr) != PSXHIP_OK) return 6;
        }
        if (fwrite(block, 1, size, out) != size) return 5;
        free(block);
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
