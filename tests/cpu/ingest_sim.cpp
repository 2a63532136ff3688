// tests/cpu/ingest_sim.cpp -- TEST INFRASTRUCTURE: drives psxavenc_amd/csrc/ingest_core.h (the arithmetic of one sample that the
// ingest kernel runs) on the CPU under -fsanitize=address,undefined.  A program, not a library: a sanitized shared object cannot
// be loaded into an unsanitized Python.
//
//   ingest_sim <in> <out>
// in:  records of 21 int32 {src_format, width, height, offset and pitch of planes 0, 1, 2, cy, rv, gu, gv, bu, yoff, coff,
//      out_format, options, n_pictures, src_stride, picture_bytes} followed by n_pictures * src_stride bytes
// out: per record n_pictures output pictures back to back (RGB24: 3 w h bytes; YUV420P: w h 3 / 2)
// Every picture is copied into a heap block of exactly picture_bytes (its first byte to the end of its last plane) and every output
// written into one of exactly its size, so that a read or a store one byte outside either is the sanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../psxavenc_amd/csrc/ingest_core.h"

static void convert(const IngestDesc& d, const uint8_t* pic, int out_format, uint8_t* out) {
    if (out_format == ING_OUT_RGB24) {
        for (int y = 0; y < d.h; y++)
            for (int x = 0; x < d.w; x++)
                for (int c = 0; c < 3; c++) out[((size_t)y * d.w + x) * 3 + c] = (uint8_t)ingest_pixel(d, pic, out_format, c, x, y);
        return;
    }
    uint8_t* o = out;
    for (int plane = 0; plane < 3; plane++) {
        const int w = plane ? d.w / 2 : d.w, h = plane ? d.h / 2 : d.h;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) *o++ = (uint8_t)ingest_pixel(d, pic, out_format, plane, x, y);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t head[21];
    while (fread(head, sizeof head, 1, in) == 1) {
        IngestDesc d = {};
        d.f = ingest_format(head[0]);
        d.w = head[1]; d.h = head[2];
        for (int p = 0; p < 3; p++) {
            d.off[p] = (uint32_t)head[3 + 2 * p];
            d.pitch[p] = (uint32_t)head[4 + 2 * p];
        }
        d.cy = head[9]; d.rv = head[10]; d.gu = head[11]; d.gv = head[12]; d.bu = head[13]; d.yoff = head[14]; d.coff = head[15];
        const int out_format = head[16], n = head[18];
        d.bilinear = (head[17] & ING_CHROMA_BILINEAR) ? 1 : 0;
        const size_t stride = (size_t)head[19], pic_bytes = (size_t)head[20];
        if (d.f.layout < 0 || d.w < 1 || d.h < 1 || n < 0 || pic_bytes > stride) return 3;
        if (out_format == ING_OUT_YUV420P && (((d.w | d.h) & 1) || d.f.layout == ING_RGB)) return 3;
        const size_t out_bytes = out_format == ING_OUT_RGB24 ? (size_t)d.w * d.h * 3 : (size_t)d.w * d.h * 3 / 2;
        uint8_t* slot = (uint8_t*)malloc(stride);
        for (int i = 0; i < n; i++) {
            uint8_t* pic = (uint8_t*)malloc(pic_bytes);
            uint8_t* o = (uint8_t*)malloc(out_bytes);
            if (!slot || !pic || !o || fread(slot, 1, stride, in) != stride) return 4;
            memcpy(pic, slot, pic_bytes);
            convert(d, pic, out_format, o);
            if (fwrite(o, 1, out_bytes, out) != out_bytes) return 5;
            free(pic);
            free(o);
        }
        free(slot);
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
