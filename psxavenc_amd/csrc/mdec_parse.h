// mdec_parse.h -- the BS v2 / v3 bitstream reader: header, DC, AC, end code, one syntax element per step.
//
// What the encoder writes (psxavenc/mdec.c:321-333 word order, :441-510 block syntax, :647-651,710 end codes, :738-754 header),
// read back:
//   header   8 bytes: uncompressed size, 0x3800, quant scale, version (2 or 3), each a little-endian 16-bit word
//   payload  little-endian 16-bit words, most significant bit first; per block (Cr, Cb, Y0..Y3 of each macroblock)
//              DC   v2: 10 bits, two's complement; 0x1FF here = the frame ended early
//                   v3: size-class prefix (luma / chroma book), then a sign bit and m magnitude bits; the value is a
//                       delta in steps of 4 on the component's last DC, wrapped to 10 bits when the context says so
//              AC   table code + sign bit | 000001 + 6-bit run + 10-bit level | 10 = end of block
//            then the end code, 10 bits: 0x1FF (v2) or 0x3FF (v3)
//
// Bits past the frame's last byte read as 0 and no byte past it is fetched, so arbitrary bytes are safe: a frame of zeros past
// its end stops at the first AC position (sixteen zero bits start no code), every step consumes at least two bits, and a
// coefficient position past 63 is an error, not a store.
//
// Plain C++ with no device dependencies: the kernel (mdec_decode_kernels.hip) runs mdec_parse_step() with the stream's bits
// handed over by v_readlane, the CPU test (tests/test_mdec_parse_cpu.py through tests/cpu/decode_sim.cpp) runs the same text
// with mdec_parse_peek32() per step, under the host sanitizers.
#pragma once
#include <stdint.h>

#include "bs_vlc_decode.h"

#ifndef PSX_HD
#if defined(__HIPCC__)
#define PSX_HD __host__ __device__ __forceinline__
#else
#define PSX_HD inline
#endif
#endif

// per-frame status (psxhip_mdec_decoded_t.status, include/psxav_hip.h: PSXHIP_DEC_*)
enum {
    MDEC_PARSE_OK = 0,
    MDEC_PARSE_EHEADER = -1,      // fewer than 8 bytes, or bytes 2..3 are not 00 38
    MDEC_PARSE_EVERSION = -2,     // version neither 2 nor 3
    MDEC_PARSE_EPREMATURE = -3,   // v2: the end code where a block's DC belongs
    MDEC_PARSE_EDC = -4,          // v3: no DC size class starts with these bits
    MDEC_PARSE_EAC = -5,          // no AC code starts with these bits
    MDEC_PARSE_EOVERRUN = -6,     // a run leads past coefficient 63
    MDEC_PARSE_EENDCODE = -7,     // the blocks are not followed by the end code
    MDEC_PARSE_ETRUNCATED = -8    // the end code lies past the frame's last byte
};

enum { MDEC_PHASE_DC = 0, MDEC_PHASE_AC = 1, MDEC_PHASE_END = 2, MDEC_PHASE_DONE = 3 };
enum { MDEC_SYM_DC = 0, MDEC_SYM_AC = 1, MDEC_SYM_EOB = 2, MDEC_SYM_END = 3, MDEC_SYM_ERROR = 4 };

// A frame can carry at most 6 * 4096 blocks (1024x1024) of at most 16 + 63 * 22 + 2 bits, plus the end code: under 4.4 MB.
// Payload bytes past this many are never reached, so capping the count changes no result and keeps bit positions in 32 bits.
#define MDEC_PARSE_MAX_PAYLOAD (8u << 20)

struct MdecParse {
    uint32_t nbytes;          // payload bytes that may be read (frame size - 8, capped)
    uint32_t pos;             // bit position in the payload
    int32_t nblk, blk;        // blocks of the frame; the block being read
    int32_t k;                // last coefficient position written in this block
    int32_t phase;
    int32_t version, wrap;
    int32_t quant_scale;
    int32_t dc_cr, dc_cb, dc_y;   // v3: last DC per component
    int32_t status;
};

struct MdecSym {
    int32_t kind;             // MDEC_SYM_*
    int32_t k;                // AC: coefficient position 1..63 (DC: 0)
    int32_t level;
    int32_t blk;              // EOB: the block that ended
};

// The 32 bits that start at bit `pos` of the payload, first bit in bit 31.  A 16-bit word that is not wholly inside the nbytes reads
// as 0.  That covers the odd byte a frame of odd size ends with: it is the low byte of a word, i.e. the word's bits 8..15 in stream
// order, and those lie past the frame's last bit (8 * nbytes) -- while the word's first eight bits would come from the byte after
// the frame.  The three words are fetched from indices clamped to the last whole word, so every load is inside the frame and none
// waits for a bounds branch, and masked afterwards.  `payload` is 2-byte aligned.
PSX_HD uint32_t mdec_parse_peek32(const uint8_t* payload, uint32_t nbytes, uint32_t pos) {
    if (nbytes < 2u) return 0u;
    const uint32_t last = (nbytes >> 1) - 1u, w = pos >> 4;
    const uint16_t* words = (const uint16_t*)payload;
    const uint32_t a = words[w < last ? w : last], b = words[w + 1u < last ? w + 1u : last], c = words[w + 2u < last ? w + 2u : last];
    const uint64_t x = ((uint64_t)(w <= last ? a : 0u) << 32) | ((uint64_t)(w + 1u <= last ? b : 0u) << 16) | (uint64_t)(w + 2u <= last ? c : 0u);
    return (uint32_t)(x >> (16u - (pos & 15u)));
}

// index into bs_dec_ac for the 32 bits `v` that start at an AC position
PSX_HD uint32_t mdec_parse_ac_index(uint32_t v) {
    const uint32_t t = v >> 16;
    return t < 0x400u ? t : 1024u + (t >> 8);
}

// Header check.  hdr0 / hdr1: the frame's first two little-endian dwords (anything when size < 8: they are not looked at), `size`
// the frame's byte count.  Returns the status; quant scale and version are set once the magic holds, as the specification leaves them.
PSX_HD int mdec_parse_begin(MdecParse& st, uint32_t hdr0, uint32_t hdr1, int64_t size, int nblk, int wrap) {
    st.nbytes = 0; st.pos = 0; st.nblk = nblk; st.blk = 0; st.k = 0;
    st.phase = MDEC_PHASE_DC; st.version = 0; st.wrap = wrap; st.quant_scale = 0;
    st.dc_cr = st.dc_cb = st.dc_y = 0;
    st.status = MDEC_PARSE_OK;
    if (size < 8 || (hdr0 >> 16) != 0x3800u) return st.status = MDEC_PARSE_EHEADER;
    st.quant_scale = (int32_t)(hdr1 & 0xFFFFu);
    st.version = (int32_t)(hdr1 >> 16);
    if (st.version != 2 && st.version != 3) return st.status = MDEC_PARSE_EVERSION;
    const int64_t n = size - 8;
    st.nbytes = n > (int64_t)MDEC_PARSE_MAX_PAYLOAD ? MDEC_PARSE_MAX_PAYLOAD : (uint32_t)n;
    if (nblk == 0) st.phase = MDEC_PHASE_END;
    return MDEC_PARSE_OK;
}

// the v3 DC tables' entries for the 32 bits `v` that start at a DC position: luma | chroma << 8
PSX_HD uint32_t mdec_parse_dc_index(uint32_t v) { return v >> 24; }

PSX_HD int mdec_parse_sext10(uint32_t v) { return (int)(v & 0x3FFu) - (int)((v & 0x200u) << 1); }

// Reads the syntax element at st.pos.  v: the 32 bits from st.pos on (mdec_parse_peek32); ac: bs_dec_ac[mdec_parse_ac_index(v)];
// dc: bs_dec_dc_luma[i] | bs_dec_dc_chroma[i] << 8, i = mdec_parse_dc_index(v) (v3 only) -- looked up by the caller: the kernel
// does it for 64 positions at a time.  Advances st.  On an error st.status is set, kind is MDEC_SYM_ERROR and nothing may be stored.
PSX_HD MdecSym mdec_parse_step(MdecParse& st, uint32_t v, uint32_t ac, uint32_t dc) {
    MdecSym s;
    s.kind = MDEC_SYM_ERROR; s.k = 0; s.level = 0; s.blk = st.blk;
    if (st.phase == MDEC_PHASE_DC) {
        if (st.version == 2) {
            const uint32_t x = v >> 22;
            if (x == 0x1FFu) { st.status = MDEC_PARSE_EPREMATURE; return s; }
            s.level = mdec_parse_sext10(x);
            st.pos += 10;
        } else {
            const int comp = st.blk % 6;
            const uint32_t e = comp < 2 ? dc >> 8 : dc & 0xFFu;
            if (e == 0) { st.status = MDEC_PARSE_EDC; return s; }
            const uint32_t plen = e & 15u, cls = e >> 4;
            int delta = 0;
            uint32_t bits = plen;
            if (cls) {
                const uint32_t m = cls - 1u;                              // plen + 1 + m <= 16
                const uint32_t positive = (v >> (31u - plen)) & 1u;
                const int j = (int)((v >> (31u - plen - m)) & ((1u << m) - 1u));
                delta = positive ? j + (1 << m) : j - ((2 << m) - 1);
                bits = plen + 1u + m;
            }
            const int cr = st.dc_cr, cb = st.dc_cb, yy = st.dc_y;
            int dc = (comp == 0 ? cr : comp == 1 ? cb : yy) + delta * 4;
            if (st.wrap) dc = ((dc + 512) & 0x3FF) - 512;                 // the decoder-side 10-bit wrap of v3dc
            st.dc_cr = comp == 0 ? dc : cr;                               // (all three written: selects of values, which stay in
            st.dc_cb = comp == 1 ? dc : cb;                               // registers, not a store through a selected address)
            st.dc_y = comp >= 2 ? dc : yy;
            s.level = (int16_t)dc;
            st.pos += bits;
        }
        st.k = 0;
        st.phase = MDEC_PHASE_AC;
        s.kind = MDEC_SYM_DC;
        return s;
    }
    if (st.phase == MDEC_PHASE_AC) {
        if (ac == 0) { st.status = MDEC_PARSE_EAC; return s; }
        const uint32_t len = ac & 31u, mag = ac >> 10;
        int run, level;
        if (mag == 0) {
            if (len == BS_DEC_AC_EOB_BITS) {
                st.pos += BS_DEC_AC_EOB_BITS;
                st.blk++;
                st.phase = st.blk == st.nblk ? MDEC_PHASE_END : MDEC_PHASE_DC;
                s.kind = MDEC_SYM_EOB;
                return s;
            }
            run = (int)((v >> 20) & 63u);
            level = mdec_parse_sext10(v >> 10);
            st.pos += BS_DEC_AC_ESCAPE_BITS + 16;
        } else {
            run = (int)((ac >> 5) & 31u);
            level = ((v >> (31u - len)) & 1u) ? -(int)mag : (int)mag;
            st.pos += len + 1u;
        }
        st.k += run + 1;
        if (st.k > 63) { st.status = MDEC_PARSE_EOVERRUN; return s; }
        s.kind = MDEC_SYM_AC;
        s.k = st.k;
        s.level = level;
        return s;
    }
    // MDEC_PHASE_END
    if ((v >> 22) != (st.version == 2 ? 0x1FFu : 0x3FFu)) { st.status = MDEC_PARSE_EENDCODE; return s; }
    st.pos += 10;
    if (st.pos > 8u * st.nbytes) { st.status = MDEC_PARSE_ETRUNCATED; return s; }
    st.phase = MDEC_PHASE_DONE;
    s.kind = MDEC_SYM_END;
    return s;
}
