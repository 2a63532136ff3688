// tests/cpu/display_sim.cpp -- TEST INFRASTRUCTURE: drives psxavenc_amd/csrc/display_core.h (the arithmetic of one pixel that the
// display kernel runs) on the CPU under -fsanitize=address,undefined.  A program, not a library: a sanitized shared object cannot
// be loaded into an unsanitized Python.
//
//   display_sim <in> <out>
// in:  records of int32 {width, height, n_frames, out_format, options} followed by n_frames * width * height * 3 / 2 bytes (NV21)
// out: per record n_frames * height * row bytes, pictures back to back
// Every frame is copied into a heap block of exactly its size and every picture written into one of exactly its size, so that a
// read or a store one byte outside either is the sanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../psxavenc_amd/csrc/display_core.h"

static void convert(const uint8_t* frame, int w, int h, int fmt, uint32_t options, uint8_t* out) {
    const bool bilinear = (options & DISP_CHROMA_BILINEAR) != 0;
    const int row = disp_row_bytes(fmt, w);
    for (int y = 0; y < h; y++) {
        uint8_t* o = out + (size_t)y * row;
        for (int x = 0; x < w; x++) {
            const DispRgb c = disp_pixel(frame, w, h, x, y, bilinear);
            if (fmt == DISP_RGB555) {
                const uint32_t p = disp_pack555(c, (options & DISP_DITHER) ? disp_dither(x, y) : 0, (options & DISP_MASK_BIT) ? 1 : 0);
                o[2 * x] = (uint8_t)(p & 255u);
                o[2 * x + 1] = (uint8_t)(p >> 8);
            } else {
                const int bytes = fmt == DISP_RGB24 ? 3 : 4;
                o[bytes * x] = (uint8_t)c.r;
                o[bytes * x + 1] = (uint8_t)c.g;
                o[bytes * x + 2] = (uint8_t)c.b;
                if (bytes == 4) o[bytes * x + 3] = 255;
            }
        }
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t head[5];
    while (fread(head, sizeof head, 1, in) == 1) {
        const int w = head[0], h = head[1], n = head[2], fmt = head[3];
        const uint32_t options = (uint32_t)head[4];
        const int row = disp_row_bytes(fmt, w);
        if (w < 16 || h < 16 || w > 1024 || h > 1024 || (w & 15) || (h & 15) || n < 0 || !row) return 3;
        const size_t frame_bytes = (size_t)w * h * 3 / 2, picture_bytes = (size_t)h * row;
        for (int i = 0; i < n; i++) {
            uint8_t* frame = (uint8_t*)malloc(frame_bytes);
            uint8_t* picture = (uint8_t*)malloc(picture_bytes);
            if (!frame || !picture || fread(frame, 1, frame_bytes, in) != frame_bytes) return 4;
            convert(frame, w, h, fmt, options, picture);
            if (fwrite(picture, 1, picture_bytes, out) != picture_bytes) return 5;
            free(frame);
            free(picture);
        }
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
