// adpcm_beam_core.h -- "psxhip ADPCM beam v1"  as plain C++ for host and device: one step of the slots of one
// (filter, shift) candidate, the pool order, the selection, the trace back through the kept decisions and the record's words.  The
// kernels (adpcm_beam_kernels.hip) compile this text; tests/cpu/adpcm_beam_sim.cpp runs the same text on the CPU under the host
// sanitizers, against tests/adpcm_beam_ref.py.
//
// Integers only; >> is arithmetic.  A candidate holds up to B <= 4 slots (e, p1, p2); slot 0 is the anchor, the reference's greedy
// path (libpsxav/adpcm.c:81-140).  Per sample x every live slot, in rising slot order, gives its children d = 0, -1, +1:
//   pv = (k1 p1 + k2 p2 + 32) >> 6;  q0 = clamp((((x - pv) << s) + (1 << (R - 1))) >> R, lo, hi);  q = q0 + d, dropped outside lo..hi
//   y = clamp(((q 2^R) >> s) + pv, -32768, 32767);  e' = min(e + (y - x)^2, 2^32 - 1)
// The d = 0 child of slot 0 is the next slot 0.  All others, in that order, are the pool: the next slots 1 .. B-1 are its B-1
// smallest e', the smallest first, ties to the earlier child.  What is kept per step is one byte of code per slot and two bits of
// parent slot for slots 1 .. 3; the winner's 28 codes are read back from those once per unit.
#pragma once
#include <stdint.h>

#ifndef PSXHIP_HD
#if defined(__HIPCC__)
#define PSXHIP_HD __host__ __device__ __forceinline__
#else
#define PSXHIP_HD inline
#endif
#endif

enum { PSXHIP_ADPCM_BEAM_MAX = 4 };

struct BeamCand {
    int k1, k2, shift, range, lo, hi, half, up;
};

// taps in 1/64 units (adpcm.c:36-37)
PSXHIP_HD BeamCand beam_cand(int f, int shift, int range) {
    BeamCand c;
    c.k1 = f == 0 ? 0 : f == 1 ? 60 : f == 2 ? 115 : f == 3 ? 98 : 122;
    c.k2 = f == 0 ? 0 : f == 1 ? 0 : f == 2 ? -52 : f == 3 ? -55 : -60;
    c.shift = shift;
    c.range = range;
    c.lo = -0x8000 >> range;
    c.hi = 0x7FFF >> range;
    c.half = 1 << (range - 1);
    c.up = range - shift;            // (q 2^R) >> s = q 2^(R - s): s <= R
    return c;
}

PSXHIP_HD int beam_predict(const BeamCand& c, int p1, int p2) { return (c.k1 * p1 + c.k2 * p2 + 32) >> 6; }

// find_min_shift (adpcm.c:39-79) for one filter: the history continues with RAW samples.  The two while loops in closed form, as
// adpcm_kernels.hip has them: rs = clamp(bit_length(max(hi, ~lo)) - (15 - range), 0, range).  xs[i * stride] is sample i.
PSXHIP_HD int beam_min_shift(const int* xs, int stride, int p1, int p2, int f, int range) {
    const BeamCand c = beam_cand(f, 0, range);
    int lo = 0, hi = 0;
    for (int i = 0; i < 28; i++) {
        const int x = xs[i * stride];
        const int r = x - beam_predict(c, p1, p2);
        lo = r < lo ? r : lo;
        hi = r > hi ? r : hi;
        p2 = p1;
        p1 = x;
    }
    const int widest = hi > ~lo ? hi : ~lo;
    int rs = (widest > 0 ? 32 - __builtin_clz((unsigned)widest) : 0) - (15 - range);
    rs = rs < 0 ? 0 : (rs > range ? range : rs);
    return range - rs;
}

// The slots of one candidate.  The pool's survivors fill the slots from 1 on, so the live slots are 0 .. n_live - 1; a slot that is
// not live holds zeros.  (Counts, not a flag per slot and place: flags live in scalar register pairs on the device, and a dozen of
// them across the step loop spilled.)
struct BeamSlots {
    uint32_t e[4];
    int p1[4], p2[4];
    int n_live;
};

PSXHIP_HD void beam_start(BeamSlots& s, int p1, int p2) {
    for (int j = 0; j < 4; j++) {
        s.e[j] = 0;
        s.p1[j] = j == 0 ? p1 : 0;
        s.p2[j] = j == 0 ? p2 : 0;
    }
    s.n_live = 1;
}

// The pool's three smallest so far, the smallest first.  tag = y << 16 | parent slot << 8 | (q & 255).
struct BeamTop {
    uint32_t e0, e1, e2, t0, t1, t2;
    int n;                 // places filled, from place 0 on
};

// a strict < against what is there: a child never passes an earlier one of the same error (the list is sorted with the empty places
// last, so "before place 0" implies "before place 1" implies "before place 2")
PSXHIP_HD void beam_insert(BeamTop& t, bool ok, uint32_t e, uint32_t tag) {
    const bool l0 = ok && (t.n < 1 || e < t.e0);
    const bool l1 = ok && (t.n < 2 || e < t.e1);
    const bool l2 = ok && (t.n < 3 || e < t.e2);
    t.e2 = l1 ? t.e1 : (l2 ? e : t.e2);
    t.t2 = l1 ? t.t1 : (l2 ? tag : t.t2);
    t.e1 = l0 ? t.e0 : (l1 ? e : t.e1);
    t.t1 = l0 ? t.t0 : (l1 ? tag : t.t1);
    t.e0 = l0 ? e : t.e0;
    t.t0 = l0 ? tag : t.t0;
    t.n += (ok && t.n < 3) ? 1 : 0;
}

// One sample for all slots.  codes: the new slots' codes, one byte each (the low 8 bits of q); parents: the slot each of the new slots
// 1 .. 3 came from, two bits each from bit 0 on.
PSXHIP_HD void beam_step(const BeamCand& c, int beam, int x, BeamSlots& s, uint32_t& codes, uint32_t& parents) {
    BeamTop top = {0, 0, 0, 0, 0, 0, 0};
    uint32_t anchor_e = 0;
    int anchor_y = 0, anchor_q = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (j > 0 && j >= beam) continue;          // no such slot at this width (the same for every lane: a branch, not a mask)
        const int pv = beam_predict(c, s.p1[j], s.p2[j]);
        int q0 = ((int)((uint32_t)(x - pv) << c.shift) + c.half) >> c.range;       // |x - pv| < 2^17, shift <= 12
        q0 = q0 < c.lo ? c.lo : (q0 > c.hi ? c.hi : q0);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int q = q0 + (k == 0 ? 0 : (k == 1 ? -1 : 1));
            const bool ok = j < s.n_live && q >= c.lo && q <= c.hi;
            int y = q * (1 << c.up) + pv;
            y = y > 0x7FFF ? 0x7FFF : (y < -0x8000 ? -0x8000 : y);
            const uint32_t err = (uint32_t)(y - x);                                // |y - x| <= 65535: the square fits 32 bits
            const uint32_t sq = err * err;
            uint32_t e = s.e[j] + sq;
            e = e < sq ? 0xFFFFFFFFu : e;
            if (j == 0 && k == 0) {
                anchor_e = e;
                anchor_y = y;
                anchor_q = q;
            } else {
                beam_insert(top, ok, e, ((uint32_t)y << 16) | ((uint32_t)j << 8) | ((uint32_t)q & 0xFFu));
            }
        }
    }
    const int o0 = s.p1[0], o1 = s.p1[1], o2 = s.p1[2], o3 = s.p1[3];
    s.e[0] = anchor_e;
    s.p2[0] = o0;
    s.p1[0] = anchor_y;
    codes = (uint32_t)anchor_q & 0xFFu;
    parents = 0;
    s.n_live = 1 + (top.n < beam - 1 ? top.n : beam - 1);
#pragma unroll
    for (int j = 1; j < 4; j++) {
        const bool full = j < s.n_live;
        const uint32_t tag = full ? (j == 1 ? top.t0 : (j == 2 ? top.t1 : top.t2)) : 0u;
        const int par = (int)((tag >> 8) & 3u);
        s.e[j] = full ? (j == 1 ? top.e0 : (j == 2 ? top.e1 : top.e2)) : 0u;
        s.p1[j] = (int)tag >> 16;
        s.p2[j] = !full ? 0 : (par == 0 ? o0 : (par == 1 ? o1 : (par == 2 ? o2 : o3)));
        codes |= (tag & 0xFFu) << (8 * j);
        parents |= (uint32_t)par << (2 * (j - 1));
    }
}

// One candidate on 28 samples xs[i * stride] from (p1, p2).  What every step kept goes to codes_hist[i * hist_stride] and
// parents_hist[i * hist_stride].  Returns the result's e; slot is the result's, (np1, np2) its state (y[27], y[26]).
PSXHIP_HD uint32_t beam_candidate(const BeamCand& c, int beam, const int* xs, int stride, int p1, int p2, uint32_t* codes_hist,
                                  uint8_t* parents_hist, int hist_stride, int& slot, int& np1, int& np2) {
    BeamSlots s;
    beam_start(s, p1, p2);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 0; i < 28; i++) {
        uint32_t codes, parents;
        beam_step(c, beam, xs[i * stride], s, codes, parents);
        codes_hist[i * hist_stride] = codes;
        parents_hist[i * hist_stride] = (uint8_t)parents;
    }
    // the live slot with the smallest e, ties to the lowest slot
    slot = 0;
    uint32_t e = s.e[0];
    np1 = s.p1[0];
    np2 = s.p2[0];
#pragma unroll
    for (int j = 1; j < 4; j++)
        if (j < s.n_live && s.e[j] < e) {
            slot = j;
            e = s.e[j];
            np1 = s.p1[j];
            np2 = s.p2[j];
        }
    return e;
}

// the 28 codes of the path that ends in `slot`, four to a word, one per byte (the low 8 bits of q)
PSXHIP_HD void beam_trace_back(const uint32_t* codes_hist, const uint8_t* parents_hist, int hist_stride, int slot, uint32_t pk[7]) {
#pragma unroll
    for (int w = 0; w < 7; w++) pk[w] = 0;
#pragma unroll
    for (int i = 27; i >= 0; i--) {
        const uint32_t c = (codes_hist[i * hist_stride] >> (8 * slot)) & 0xFFu;
        pk[i >> 2] |= c << (8 * (i & 3));
        slot = slot == 0 ? 0 : (int)((parents_hist[i * hist_stride] >> (2 * (slot - 1))) & 3u);
    }
}

// the record's words (PSXHIP_ADPCM_RECORD_SIZE(bits)).  4-bit codes: 4 words in the layout of an SPU block -- header, 0, fourteen bytes of
// two codes each, the even sample low.  8-bit codes: 8 words -- header, three zero bytes, the 28 codes.  (Two functions: one array
// filled on either side of a branch went through the stack on the device.)
PSXHIP_HD void beam_record4(uint32_t header, const uint32_t pk[7], uint32_t rec[4]) {
    uint32_t h[7];
#pragma unroll
    for (int w = 0; w < 7; w++) {
        const uint32_t c = pk[w] & 0x0F0F0F0Fu;
        const uint32_t t = c | (c >> 4);
        h[w] = (t & 0xFFu) | ((t >> 8) & 0xFF00u);
    }
    rec[0] = (header & 0xFFu) | (h[0] << 16);
    rec[1] = h[1] | (h[2] << 16);
    rec[2] = h[3] | (h[4] << 16);
    rec[3] = h[5] | (h[6] << 16);
}
PSXHIP_HD void beam_record8(uint32_t header, const uint32_t pk[7], uint32_t rec[8]) {
    rec[0] = header & 0xFFu;
#pragma unroll
    for (int w = 0; w < 7; w++) rec[1 + w] = pk[w];
}

// One sound unit, candidate after candidate in the reference's loop order (adpcm.c:158-183), the first strict minimum wins: what the
// kernels spread over a row of lanes.  Host code (the CPU check and nothing else calls it).
struct BeamUnit {
    uint32_t header, e;
    int p1, p2, slot;
    uint32_t rec[8];
};

inline BeamUnit beam_encode_unit(const int* xs, int p1, int p2, int filter_count, int range, int beam) {
    BeamUnit u = {0, 0, p1, p2, 0, {0, 0, 0, 0, 0, 0, 0, 0}};
    bool have = false;
    uint32_t codes_hist[28];
    uint8_t parents_hist[28];
    for (int f = 0; f < filter_count; f++) {
        const int m = beam_min_shift(xs, 1, p1, p2, f, range);
        for (int sh = (m - 1 < 0 ? 0 : m - 1); sh <= (m + 1 > range ? range : m + 1); sh++) {
            int slot, np1, np2;
            const uint32_t e = beam_candidate(beam_cand(f, sh, range), beam, xs, 1, p1, p2, codes_hist, parents_hist, 1, slot, np1, np2);
            if (have && !(e < u.e)) continue;
            have = true;
            u.e = e;
            u.header = (uint32_t)((sh & 15) | (f << 4));
            u.p1 = np1;
            u.p2 = np2;
            u.slot = slot;
            uint32_t pk[7];
            beam_trace_back(codes_hist, parents_hist, 1, slot, pk);
            if (range == 12) beam_record4(u.header, pk, u.rec);
            else beam_record8(u.header, pk, u.rec);
        }
    }
    return u;
}
