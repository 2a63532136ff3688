// spu_seam_core.h -- "psxhip SPU loop seam v1" (include/psxav_hip.h) as plain C++ for host and device: the
// step between two body passes of mode STEADY, and the seam report of one entry.  The kernels (spu_seam_kernels.hip) compile this
// text and add nothing but the lane-to-entry mapping.  The unit arithmetic is the decoder's (adpcm_decode_core.h).  Integers only.
#pragma once
#include <hip/hip_runtime.h>        // uint4: a block is one 16-byte load
#include <stdint.h>

#include "adpcm_decode_core.h"
#include "spu_bank_plan.h"

// ---- the step.  Body chain j of the seam chain table (spu_bank_plan.h): `chain` its row of the DEVICE table, whose n_units the step
// sets to 0 once the entry is fixed so that later body launches pass over it; `state` its state slot, which the body launch has just
// carried from s_k to e_k; `start` holds s_k; s0 is the intro's end state ((0, 0) without an intro).
//   k = -1  arms the entry before pass 0: s_0 into state and start, the chain's units restored, the outcome P.
//   k >= 0  compares: e_k == s_k records k and retires the chain; else s_{k+1} = e_k, and after the last pass s_0 goes back into the
//           state for the one launch that restores pass 0's blocks.
PSXHIP_HD void spu_seam_step(int k, int passes, psxhip_adpcm_state_t s0, int units, psxhip_adpcm_chain_t* chain, psxhip_adpcm_state_t* state,
                             psxhip_adpcm_state_t* start, int32_t* outcome) {
    if (k < 0) {
        *state = s0;
        *start = s0;
        chain->n_units = units;
        *outcome = passes;
        return;
    }
    if (chain->n_units == 0) return;            // fixed at an earlier pass
    const psxhip_adpcm_state_t e = *state, s = *start;
    if (e.prev1 == s.prev1 && e.prev2 == s.prev2) {
        *outcome = k;
        chain->n_units = 0;
    } else if (k + 1 < passes) {
        *start = e;
    } else {
        *state = s0;
    }
}

// ---- the report
struct SpuSeamPair {        // a decoder state
    int p1, p2;
};

// the PCM sample i of an entry, zero past `samples`
PSXHIP_HD int spu_seam_pcm(const psxhip_spu_seam_row_t& r, const int16_t* pcm, int64_t i) {
    return i < (int64_t)r.samples ? (int)pcm[r.pcm_offset + i] : 0;
}

// One entry, serially.  The first loop is pass 1: it keeps the state in front of the seam block, the end state b and, with PCM, the
// body's error.  The second loop runs pass 2 (from b) beside pass 1 (from the kept state) over the same block, loaded once, and ends
// where the two states coincide: from there the passes are the same samples, so neither the difference nor pass2_err - pass1_err
// changes any more.  At its end the states are equal exactly when b2 == b (pass 1's state behind the last unit IS b).
PSXHIP_HD void spu_seam_report_entry(const psxhip_spu_seam_row_t& r, const uint8_t* bank, const int16_t* pcm, psxhip_spu_seam_t* out) {
    psxhip_spu_seam_t s;
    s.seam_block = r.seam_block;
    s.first_units = 0;
    s.first_peak = 0;
    s.settled = 0;
    s.first_sse = 0;
    s.pass1_err = 0;
    s.pass2_err = 0;
    if (r.seam_block < 0) {
        *out = s;
        return;
    }
    const uint4* blocks = (const uint4*)bank + r.first_block;
    const int D = r.data_blocks, S = r.seam_block;
    SpuSeamPair a = {0, 0}, at = {0, 0};
    uint64_t err1 = 0;
    for (int u = 0; u < D; u++) {
        if (u == S) at = a;
        const uint4 v = blocks[u];

        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const AdpcmDecHeader h = adpcm_dec_header(w[0] & 0xFFu, 5, 12);
        const bool tally = pcm != nullptr && u >= S;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 28; i++) {
            const int d = adpcm_dec_sample(adpcm_dec_code<4>(w, i), 12, h, a.p1, a.p2);
            a.p2 = a.p1;
            a.p1 = d;
            if (tally) {
                const int64_t e = d - spu_seam_pcm(r, pcm, (int64_t)u * 28 + i);
                err1 += (uint64_t)(e * e);
            }
        }
    }
    SpuSeamPair b = a;          // pass 2's state; `at` is pass 1's
    int k = 0, peak = 0;
    uint64_t sse = 0;
    int64_t delta = 0;          // pass2_err - pass1_err so far
    while (k < D - S && (at.p1 != b.p1 || at.p2 != b.p2)) {
        const uint4 v = blocks[S + k];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const AdpcmDecHeader h = adpcm_dec_header(w[0] & 0xFFu, 5, 12);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 28; i++) {
            const int code = adpcm_dec_code<4>(w, i);
            const int y1 = adpcm_dec_sample(code, 12, h, at.p1, at.p2);
            const int y2 = adpcm_dec_sample(code, 12, h, b.p1, b.p2);
            at.p2 = at.p1;
            at.p1 = y1;
            b.p2 = b.p1;
            b.p1 = y2;
            const int64_t d = y2 - y1;
            const int ad = (int)(d < 0 ? -d : d);
            peak = ad > peak ? ad : peak;
            sse += (uint64_t)(d * d);
            if (pcm != nullptr) {
                const int64_t x = spu_seam_pcm(r, pcm, (int64_t)(S + k) * 28 + i);
                delta += (y2 - x) * (y2 - x) - (y1 - x) * (y1 - x);
            }
        }
        k++;
    }
    s.first_units = k;
    s.first_peak = peak;
    s.settled = at.p1 == b.p1 && at.p2 == b.p2 ? 1 : 0;
    s.first_sse = sse;
    s.pass1_err = err1;
    s.pass2_err = (uint64_t)((int64_t)err1 + delta);
    *out = s;
}
