// tests/cpu/decode_sim.cpp -- TEST INFRASTRUCTURE: drives psxavenc_amd/csrc/mdec_parse.h (the bitstream reader the decode
// kernel runs) on the CPU, one peek per step, under -fsanitize=address,undefined.  A program, not a library: a sanitized
// shared object cannot be loaded into an unsanitized Python.
//
//   decode_sim <in> <out> [windowed]
// windowed: the kernel's schedule instead of one peek per step -- 64 "lanes" fetch and classify the 64 bit offsets of a window, a
// walk then steps through the offsets where codes start, and the block lives in 64 per-lane values stored at its end.
// in:  records of int32 {width, height, size, dc_wrap, want_levels} followed by `size` bytes
// out: per record int32 {status, quant_scale, version, bits_consumed}, then blocks * 64 int16 levels when want_levels and status 0
// Every frame is copied into a heap block of exactly `size` bytes and its levels into one of exactly blocks * 64 int16, so that a
// read or a store one byte outside either is the sanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../psxavenc_amd/csrc/mdec_parse.h"

static int decode(int w, int h, const uint8_t* bs, int size, int16_t* levels, int wrap, int32_t out[4]) {
    const int nblk = (w / 16) * (h / 16) * 6;
    MdecParse st;
    uint32_t hdr[2] = {0, 0};
    if (size >= 8) memcpy(hdr, bs, 8);
    out[0] = mdec_parse_begin(st, hdr[0], hdr[1], size, nblk, wrap);
    out[1] = st.quant_scale;
    out[2] = st.version;
    out[3] = 0;
    if (out[0]) return out[0];
    const uint8_t* payload = bs + 8;
    int16_t block[64];
    long steps = 0;
    const long max_steps = (long)nblk * 66 + 2;          // DC + at most 63 coefficients + end of block, per block; the end code
    while (st.phase != MDEC_PHASE_DONE) {
        if (++steps > max_steps) return out[0] = -100;   // the reader did not terminate
        const uint32_t v = mdec_parse_peek32(payload, st.nbytes, st.pos);
        const MdecSym s = mdec_parse_step(st, v, bs_dec_ac[mdec_parse_ac_index(v)],
                                           bs_dec_dc_luma[mdec_parse_dc_index(v)] | (uint32_t)bs_dec_dc_chroma[mdec_parse_dc_index(v)] << 8);
        if (s.kind == MDEC_SYM_ERROR) return out[0] = st.status;
        if (s.kind == MDEC_SYM_DC) {
            memset(block, 0, sizeof block);
            block[0] = (int16_t)s.level;
        } else if (s.kind == MDEC_SYM_AC) {
            block[s.k] = (int16_t)s.level;
        } else if (s.kind == MDEC_SYM_EOB) {
            memcpy(levels + (size_t)s.blk * 64, block, sizeof block);
        }
    }
    out[3] = (int32_t)st.pos;
    return 0;
}

// mdec_parse_kernel (psxavenc_amd/csrc/mdec_decode_kernels.hip) with the lanes as arrays
static int decode_windowed(int w, int h, const uint8_t* bs, int size, int16_t* levels, int wrap, int32_t out[4]) {
    const int nblk = (w / 16) * (h / 16) * 6;
    MdecParse st;
    uint32_t hdr[2] = {0, 0};
    if (size >= 8) memcpy(hdr, bs, 8);
    mdec_parse_begin(st, hdr[0], hdr[1], size, nblk, wrap);
    const uint8_t* payload = bs + 8;
    const bool v3 = st.version == 3;
    int lv[64] = {0};
    long windows = 0;
    while (st.status == MDEC_PARSE_OK && st.phase != MDEC_PHASE_DONE) {
        if (++windows > (long)nblk * 66 + 2) { st.status = -100; break; }
        const uint32_t base = st.pos;
        uint32_t v_lane[64], e_lane[64];
        for (int lane = 0; lane < 64; lane++) {
            v_lane[lane] = mdec_parse_peek32(payload, st.nbytes, base + (uint32_t)lane);
            e_lane[lane] = bs_dec_ac[mdec_parse_ac_index(v_lane[lane])];
            if (v3) e_lane[lane] |= (uint32_t)(bs_dec_dc_luma[mdec_parse_dc_index(v_lane[lane])] | (bs_dec_dc_chroma[mdec_parse_dc_index(v_lane[lane])] << 8)) << 16;
        }
        while (st.status == MDEC_PARSE_OK && st.phase != MDEC_PHASE_DONE && st.pos - base < 64u) {
            const int at = (int)(st.pos - base);
            const MdecSym s = mdec_parse_step(st, v_lane[at], e_lane[at] & 0xFFFFu, e_lane[at] >> 16);
            for (int lane = 0; lane < 64; lane++) {
                if (s.kind == MDEC_SYM_DC) lv[lane] = lane == 0 ? s.level : 0;
                else if (s.kind == MDEC_SYM_AC) lv[lane] = lane == s.k ? s.level : lv[lane];
                else if (s.kind == MDEC_SYM_EOB) levels[(size_t)s.blk * 64 + lane] = (int16_t)lv[lane];
            }
        }
    }
    out[0] = st.status;
    out[1] = st.quant_scale;
    out[2] = st.version;
    out[3] = st.status == MDEC_PARSE_OK ? (int32_t)st.pos : 0;
    return out[0];
}

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) return 2;
    const bool windowed = argc == 4;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t rec[5];
    while (fread(rec, sizeof rec, 1, in) == 1) {
        const int w = rec[0], h = rec[1], size = rec[2];
        if (w < 16 || h < 16 || w > 1024 || h > 1024 || size < 0) return 3;
        const size_t nlev = (size_t)(w / 16) * (h / 16) * 6 * 64;
        uint8_t* bs = (uint8_t*)malloc(size ? size : 1);
        int16_t* levels = (int16_t*)malloc(nlev * sizeof(int16_t));
        if (!bs || !levels) return 4;
        if (size && fread(bs, 1, size, in) != (size_t)size) return 3;
        int32_t res[4];
        (windowed ? decode_windowed : decode)(w, h, bs, size, levels, rec[3], res);
        fwrite(res, sizeof res, 1, out);
        if (rec[4] && res[0] == 0) fwrite(levels, sizeof(int16_t), nlev, out);
        free(bs);
        free(levels);
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
