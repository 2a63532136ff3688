// mdec_shed_core.h -- the rule "psxhip MDEC shed v1"  in plain C++ for host and device: the exact integer FDCT as a
// straightforward statement, the quantiser, the shed predicate, what one shed step changes at one position of one block (bits,
// distortion, count), the step choice, the acceptance, and the codes of a refined row.  No HIP in here: mdec_shed_kernels.hip runs
// this text one lane per zig-zag position with the neighbour masks from wave ballots, tests/cpu/mdec_shed_check.cpp runs it under the
// host sanitizers with the masks from a loop.  The numpy statement is tests/mdec_shed_ref.py.
//
// A frame whose plain encode chose scale N is tried at M = N - 1.  Shed step t = 1 .. 63 K names a magnitude class m = 1 + (t - 1) / 63
// and a position p = 64 - ((t - 1) % 63 + 1): it zeroes every AC level with |lv| <= m - 1, and those with |lv| <= m at positions
// z >= p.  Going from step t - 1 to t changes only position p of a block, and only when |lv[p]| == m: its code goes, and the code of
// the next survivor above it now carries the longer run.  So every step's bits, distortion and count are the step before plus a sum
// over blocks that each lane (position) keeps for itself: 63 sums per class and frame.
#pragma once
#include <stdint.h>

#include "bs_vlc_lut.h"

// SHED_DEVICE: defined by the kernel file, which keeps copies of the tables of bs_vlc_lut.h in device memory (shed_dev_*); everybody
// else -- a host compiler, the host layer -- gets host functions over the tables themselves
#if defined(__HIPCC__) && defined(SHED_DEVICE)
#define SHED_HD __host__ __device__ inline
#else
#define SHED_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__) && defined(SHED_DEVICE)
#define SHED_TAB(name) shed_dev_##name
#else
#define SHED_TAB(name) bs_##name
#endif

#define PSXHIP_MDEC_SHED_KERNEL_REV "mdec-shed-k1.0"

constexpr int kShedMaxMagnitude = 3;      // K: magnitude classes a call may ask for
constexpr int kShedClassSteps = 63;       // shed steps per class: one per AC position, 63 down to 1

// Per-frame accumulators: kShedRows rows of 64 int64, one column per zig-zag position (column 0 stays 0); a row's meaning is the sum
// over its columns, except for the three delta rows per class, whose columns are the steps' own
enum {
    SHED_D_PLAIN = 0,       // sum (F - R_N)^2
    SHED_D_BASE,            // sum (F - R_M)^2: D_shed at step 0
    SHED_BITS0,             // AC code bits at scale M, nothing shed
    SHED_NNZ0,              // non-zero AC levels at scale M
    SHED_DBITS,             // [3] change of the AC bits at step (m, column)
    SHED_DCNT = SHED_DBITS + kShedMaxMagnitude,     // [3] levels zeroed at that step
    SHED_DDIST = SHED_DCNT + kShedMaxMagnitude,     // [3] change of the distortion: F^2 - (F - R)^2
    kShedRows = SHED_DDIST + kShedMaxMagnitude
};

// ---------------------------------------------------------------- the FDCT: jfdctint "islow" for 8-bit samples, 4 extra bits after the rows
// (the arithmetic psxhip_mdec_fdct_host and the oracle's mdec_coefs must both equal; every result is an int16 between and after the passes)
SHED_HD int32_t shed_descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

SHED_HD void shed_fdct_1d(int16_t* p, int stride, bool columns) {
    const int32_t d0 = p[0], d1 = p[stride], d2 = p[2 * stride], d3 = p[3 * stride];
    const int32_t d4 = p[4 * stride], d5 = p[5 * stride], d6 = p[6 * stride], d7 = p[7 * stride];
    const int32_t s07 = d0 + d7, s16 = d1 + d6, s25 = d2 + d5, s34 = d3 + d4;
    const int32_t e0 = s07 + s34, e3 = s07 - s34, e1 = s16 + s25, e2 = s16 - s25;
    int32_t o0 = d3 - d4, o1 = d2 - d5, o2 = d1 - d6, o3 = d0 - d7;
    const int shift = columns ? 13 + 4 : 13 - 4;
    if (columns) {
        p[0] = (int16_t)shed_descale(e0 + e1, 4);
        p[4 * stride] = (int16_t)shed_descale(e0 - e1, 4);
    } else {
        p[0] = (int16_t)((e0 + e1) * 16);
        p[4 * stride] = (int16_t)((e0 - e1) * 16);
    }
    const int32_t r = (e2 + e3) * 4433;
    p[2 * stride] = (int16_t)shed_descale(r + e3 * 6270, shift);
    p[6 * stride] = (int16_t)shed_descale(r - e2 * 15137, shift);
    int32_t z1 = o0 + o3, z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const int32_t z5 = (z3 + z4) * 9633;
    o0 *= 2446;
    o1 *= 16819;
    o2 *= 25172;
    o3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    p[7 * stride] = (int16_t)shed_descale(o0 + z1 + z3, shift);
    p[5 * stride] = (int16_t)shed_descale(o1 + z2 + z4, shift);
    p[3 * stride] = (int16_t)shed_descale(o2 + z2 + z3, shift);
    p[stride] = (int16_t)shed_descale(o3 + z1 + z4, shift);
}

// one 8x8 block of level-shifted samples (-128..127, raster order), in place
SHED_HD void shed_fdct8x8(int16_t* blk) {
    for (int r = 0; r < 8; r++) shed_fdct_1d(blk + 8 * r, 1, false);
    for (int c = 0; c < 8; c++) shed_fdct_1d(blk + c, 8, true);
}

// ---------------------------------------------------------------- quantiser
// DIVIDE_ROUNDED (mdec.c:438): n / d rounded half away from zero, d > 0
SHED_HD int shed_div_rounded(int n, int d) { return n >= 0 ? (2 * n + d) / (2 * d) : -((-2 * n + d) / (2 * d)); }
// ... and the level range (mdec.c:260-267): 0x1FF stays free for the v2 end code
SHED_HD int shed_quant(int f, int qs) {
    const int v = shed_div_rounded(f, qs);
    return v < -0x200 ? -0x200 : (v > 0x1FE ? 0x1FE : v);
}
SHED_HD int shed_dc_level(int f0) { return shed_quant(f0, SHED_TAB(quant_zz)[0] * 8); }
// the AC level at zig-zag position z (1..63) and scale s
SHED_HD int shed_ac_level(int f, int z, int s) { return shed_quant(f, SHED_TAB(quant_zz)[z] * s); }
SHED_HD int64_t shed_sq(int64_t x) { return x * x; }
// what zeroing a level reconstructed as r does to the block's squared error
SHED_HD int64_t shed_dist_gain(int f, int r) { return shed_sq(f) - shed_sq((int64_t)f - r); }

// ---------------------------------------------------------------- codes
SHED_HD int shed_lut_index(int run, int alevel) { return (alevel > BS_LUT_MAX_LEVEL ? BS_LUT_MAX_LEVEL + 1 : alevel) * BS_LUT_W + run; }
// bits of (run, level): the table code with its sign, or the 22-bit escape
SHED_HD int shed_len(int run, int alevel) { return SHED_TAB(ac_len16_lut)[shed_lut_index(run, alevel)] & 0xFF; }
// bits << 24 | code
SHED_HD uint32_t shed_ac_code(int run, int level) {
    const int a = level < 0 ? -level : level;
    const uint32_t e = SHED_TAB(ac_code_lut)[shed_lut_index(run, a)];
    if ((e >> 24) == BS_ESCAPE_BITS) return (uint32_t)BS_ESCAPE_BITS << 24 | 1u << 16 | (uint32_t)run << 10 | ((uint32_t)level & 0x3FF);
    return (e & 0xFF000000u) | (e & 0x1FFFEu) | (level < 0 ? 1u : 0u);
}
// The DC code of a block: bits << 24 | code.  comp: 0 Cr, 1 Cb, 2 Y; *last: the component's running DC (v3), updated.
// A v3 delta the code books do not carry (|delta| > 255; the reference reads uninitialised memory there) comes back as 0.
SHED_HD uint32_t shed_dc_code(int codec, int comp, int dc, int* last) {
    if (codec == 0) return 10u << 24 | ((uint32_t)dc & 0x3FF);
    int delta = shed_div_rounded(dc - *last, 4);
    *last = (int16_t)(*last + delta * 4);
    if (codec == 2) delta = delta < -0x80 ? delta + 0x100 : (delta > 0x80 ? delta - 0x100 : delta);
    const bool luma = comp == 2;
    if (delta == 0) return luma ? (uint32_t)BS_DC_LUMA_ZERO_LEN << 24 | BS_DC_LUMA_ZERO_CODE : (uint32_t)BS_DC_CHROMA_ZERO_LEN << 24 | BS_DC_CHROMA_ZERO_CODE;
    const int a = delta < 0 ? -delta : delta;
    int m = 0;
    while ((2 << m) <= a) m++;
    if (m > 7) return 0;
    const uint32_t prefix = luma ? SHED_TAB(dc_luma_prefix)[m] : SHED_TAB(dc_chroma_prefix)[m];
    const int plen = luma ? SHED_TAB(dc_luma_plen)[m] : SHED_TAB(dc_chroma_plen)[m];
    const uint32_t tail = delta > 0 ? (1u << m | (uint32_t)(delta - (1 << m))) : (uint32_t)(delta + (2 << m) - 1);
    return (uint32_t)(plen + 1 + m) << 24 | prefix << (m + 1) | tail;
}

// ---------------------------------------------------------------- shed steps
SHED_HD void shed_step_class(int t, int* m, int* p) {
    *m = 1 + (t - 1) / kShedClassSteps;
    *p = 64 - ((t - 1) % kShedClassSteps + 1);
}
// is the level of magnitude a at position z gone at step t (t = 0: nothing is)
SHED_HD bool shed_gone(int a, int z, int t) {
    if (t == 0) return false;
    int m, p;
    shed_step_class(t, &m, &p);
    return a <= m - 1 || (a <= m && z >= p);
}
// Position z between its neighbours.  below: the positions that stand before z when it is looked at (bit 0, the DC, clear), above:
// those after it.  *run: zeros between z and the nearest of `below` (or the DC); returns the nearest of `above`, 0 when there is none
SHED_HD int shed_neighbours(int z, uint64_t below, uint64_t above, int* run) {
    const uint64_t lo = below & ((1ull << z) - 1);
    const int prev = lo ? 63 - __builtin_clzll(lo) : 0;
    *run = z - prev - 1;
    const uint64_t hi = z < 63 ? above & ~((2ull << z) - 1) : 0;
    return hi ? __builtin_ctzll(hi) : 0;
}
// what the AC bits change by when the level of magnitude m at z goes: run zeros below it, the next survivor (magnitude a_next) at
// `next` above it (0: none)
SHED_HD int shed_bit_delta(int z, int m, int run, int next, int a_next) {
    if (!next) return -shed_len(run, m);
    const int run2 = next - z - 1;
    return shed_len(run + 1 + run2, a_next) - shed_len(run, m) - shed_len(run2, a_next);
}

// ---------------------------------------------------------------- fit, choice, acceptance
// the bytes a stream of `bits` bits takes with its header, before the round-up to 4, and the encoder's own fit rule
SHED_HD int64_t shed_need(int64_t bits) { return 8 + 2 * ((bits + 15) / 16); }
SHED_HD bool shed_fits(int64_t bits, int b) { return shed_need(bits) <= b - (b & 1); }
SHED_HD bool shed_frame_eligible(int quant_scale) { return quant_scale > 1 && quant_scale < 64; }

struct ShedDecision {
    int32_t step;           // t* when refined, else 0
    int32_t count;          // levels zeroed when refined, else 0
    int64_t d_plain, d_shed;        // when some step fits, else 0
    int64_t bits;           // the refined stream's bits, the end code included
    int32_t nnz;            // its non-zero AC levels
    int32_t refined;
};
// acc: the frame's kShedRows x 64 sums; dc_bits: its DC codes' bits; first fit over t = 1 .. 63 K, then D_shed < D_plain
SHED_HD ShedDecision shed_decide(const int64_t* acc, int64_t dc_bits, int n_blocks, int b, int K) {
    ShedDecision d = {0, 0, 0, 0, 0, 0, 0};
    int64_t d_plain = 0, dist = 0, bits = dc_bits + 2 * (int64_t)n_blocks + 10, nnz = 0, count = 0;
    for (int z = 1; z < 64; z++) {
        d_plain += acc[SHED_D_PLAIN * 64 + z];
        dist += acc[SHED_D_BASE * 64 + z];
        bits += acc[SHED_BITS0 * 64 + z];
        nnz += acc[SHED_NNZ0 * 64 + z];
    }
    for (int t = 1; t <= kShedClassSteps * K; t++) {
        int m, p;
        shed_step_class(t, &m, &p);
        bits += acc[(SHED_DBITS + m - 1) * 64 + p];
        count += acc[(SHED_DCNT + m - 1) * 64 + p];
        dist += acc[(SHED_DDIST + m - 1) * 64 + p];
        if (!shed_fits(bits, b)) continue;
        d.d_plain = d_plain;
        d.d_shed = dist;
        if (dist < d_plain) {
            d.step = t;
            d.count = (int32_t)count;
            d.bits = bits;
            d.nnz = (int32_t)(nnz - count);
            d.refined = 1;
        }
        break;
    }
    return d;
}
// what encode_frame_bs leaves for such a stream (mdec.c:497,507,719-736)
SHED_HD void shed_result(const ShedDecision& d, int n_blocks, int M, int32_t out[4]) {
    const int hwords = (d.nnz + 2 * n_blocks + 2 + 0x3F) & ~0x3F;
    out[0] = M;
    out[1] = (int32_t)((shed_need(d.bits) + 3) & ~(int64_t)3);
    out[2] = (hwords + 1) >> 1;
    out[3] = hwords;
}

// ---------------------------------------------------------------- the row
// `len` bits of `code` at bit `pos` of the payload (bit 0 = the top bit of the halfword at byte 8): up to three 16-bit words, each
// OR-ed into the row through sink.or16(halfword index from byte 0, value).  The words are stored low byte first.
template <class Sink>
SHED_HD void shed_put(Sink& sink, int64_t pos, int len, uint32_t code) {
    const int hw = (int)(pos >> 4), sh = 48 - (int)(pos & 15) - len;
    const uint64_t v = (uint64_t)(code & ((1u << len) - 1u)) << sh;
    for (int j = 0; j < 3; j++) {
        const uint32_t w = (uint32_t)(v >> (32 - 16 * j)) & 0xFFFFu;
        if (w) sink.or16(4 + hw + j, w);
    }
}
template <class Sink>
SHED_HD void shed_put_header(Sink& sink, int codec, int M, int blocks_used) {
    sink.or16(0, (uint32_t)blocks_used & 0xFFFFu);
    sink.or16(1, 0x3800u);
    sink.or16(2, (uint32_t)M);
    sink.or16(3, codec == 0 ? 2u : 3u);
}
SHED_HD uint32_t shed_end_code(int codec) { return codec == 0 ? 0x1FFu : 0x3FFu; }

// ---------------------------------------------------------------- host statement of a whole frame (tests/cpu/mdec_shed_check.cpp)
#if !defined(__HIP_DEVICE_COMPILE__)
// one block's 64 coefficients in zig-zag order into the frame's sums: what the analyse kernel does with one lane per position
inline void shed_analyse_block_host(const int16_t* fz, int M, int N, int64_t* acc) {
    int lv[64], a[64];
    lv[0] = a[0] = 0;
    for (int z = 1; z < 64; z++) {
        lv[z] = shed_ac_level(fz[z], z, M);
        a[z] = lv[z] < 0 ? -lv[z] : lv[z];
        const int q = bs_quant_zz[z];
        acc[SHED_D_PLAIN * 64 + z] += shed_sq((int64_t)fz[z] - shed_ac_level(fz[z], z, N) * q * N);
        acc[SHED_D_BASE * 64 + z] += shed_sq((int64_t)fz[z] - lv[z] * q * M);
    }
    uint64_t ge[kShedMaxMagnitude + 2] = {0};            // ge[m]: positions with |lv| >= m
    for (int m = 1; m <= kShedMaxMagnitude + 1; m++)
        for (int z = 1; z < 64; z++)
            if (a[z] >= m) ge[m] |= 1ull << z;
    for (int z = 1; z < 64; z++) {
        if (!a[z]) continue;
        int run;
        shed_neighbours(z, ge[1], 0, &run);
        acc[SHED_BITS0 * 64 + z] += shed_len(run, a[z]);
        acc[SHED_NNZ0 * 64 + z] += 1;
        const int m = a[z];
        if (m > kShedMaxMagnitude) continue;
        const int next = shed_neighbours(z, ge[m], ge[m + 1], &run);
        acc[(SHED_DBITS + m - 1) * 64 + z] += shed_bit_delta(z, m, run, next, a[next]);
        acc[(SHED_DCNT + m - 1) * 64 + z] += 1;
        acc[(SHED_DDIST + m - 1) * 64 + z] += shed_dist_gain(fz[z], lv[z] * bs_quant_zz[z] * M);
    }
}

struct ShedHostSink {
    uint8_t* row;
    void or16(int hw, uint32_t v) {
        row[2 * hw] |= (uint8_t)v;
        row[2 * hw + 1] |= (uint8_t)(v >> 8);
    }
};
// the refined frame's row: b bytes, zeroed here.  fz: n_blocks x 64 coefficients in zig-zag order, blocks in the encoder's order
inline void shed_emit_row_host(int codec, const int16_t* fz, int n_blocks, int M, const ShedDecision& d, int b, uint8_t* row) {
    for (int i = 0; i < b; i++) row[i] = 0;
    ShedHostSink sink = {row};
    int32_t res[4];
    shed_result(d, n_blocks, M, res);
    shed_put_header(sink, codec, M, res[2]);
    int last[3] = {0, 0, 0};
    int64_t pos = 0;
    for (int blk = 0; blk < n_blocks; blk++) {
        const int16_t* f = fz + (size_t)blk * 64;
        const int comp = blk % 6 < 2 ? blk % 6 : 2;
        const uint32_t dc = shed_dc_code(codec, comp, shed_dc_level(f[0]), &last[comp]);
        shed_put(sink, pos, (int)(dc >> 24), dc & 0xFFFFFF);
        pos += dc >> 24;
        int run = 0;
        for (int z = 1; z < 64; z++) {
            const int lv = shed_ac_level(f[z], z, M);
            if (lv == 0 || shed_gone(lv < 0 ? -lv : lv, z, d.step)) {
                run++;
                continue;
            }
            const uint32_t c = shed_ac_code(run, lv);
            shed_put(sink, pos, (int)(c >> 24), c & 0xFFFFFF);
            pos += c >> 24;
            run = 0;
        }
        shed_put(sink, pos, 2, 2);
        pos += 2;
    }
    shed_put(sink, pos, 10, shed_end_code(codec));
}
#endif
