// tests/cpu/search_bound_sim.cpp -- TEST INFRASTRUCTURE: drives psxavenc_amd/csrc/mdec_search.h the way the frame kernel does since
// mdec-k3.9: a pass that counts at p - 1 and emits at p may stop counting at its checkpoint, and what it then reports for p - 1 is a
// lower bound for all scales <= p - 1 (mdec_search_note_bound), not an evaluation.  A stand-alone program: reads records of int32
//     limit_bits, fixed_bits, guess, seed, tb[64], fb[64]       (tb[s]: total bits at scale s, fb[s]: tb - deficit, a valid bound)
// from stdin and prints per record "answer passes bounds proved diverged plain_answer plain_passes" -- answer 64 = nothing fits, < 0 an
// error of the search.  In a (p - 1, p) pass the count is replaced, with probability one half (a generator seeded per record), by a
// bound drawn evenly from [0, fb[p - 1]]; `proved` of the `bounds` exceeded the limit.  `diverged`: bounds after which the search's
// state can differ from that of a search that counts everything -- the bound proved (no model point at p - 1), or it did not but the
// emit scale's own evaluation proved p - 1 as well (nothing left to count, and again no model point).  The plain_ figures are the
// same record run without any bound.
#include <stdint.h>
#include <stdio.h>

#include "../../psxavenc_amd/csrc/mdec_search.h"

static uint32_t next_u32(uint64_t& state) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}

static int run(const int* tb, const int* fb, int limit_bits, int fixed_bits, int guess, uint64_t rng, bool sample, int* passes, int* bounds, int* proved, int* diverged) {
    MdecSearch st;
    mdec_search_init(st);
    int n = 0, nb = 0, np = 0, nd = 0, bounded = 0;       // bounded: the scale the last pass reported a bound for (0: none)
    for (;;) {
        MdecPass p = (limit_bits < fixed_bits) ? MdecPass{0, 0, 1}
                     : bounded ? mdec_search_next_after_bound(st, bounded, guess, limit_bits, fixed_bits) : mdec_search_next(st, guess, limit_bits, fixed_bits);
        bounded = 0;
        bool bound_proved = false;
        if (p.done) break;
        if (++n > 200) return -1;
        if (p.count_scale < 0 || p.count_scale > 63 || p.emit_scale < 0 || p.emit_scale > 63) return -3;
        if (p.count_scale == 0 && p.emit_scale == 0) return -4;
        if (p.count_scale) {
            const bool sampled = sample && p.emit_scale == p.count_scale + 1 && (next_u32(rng) & 1u);
            if (sampled) {
                const int top = fb[p.count_scale] > 0 ? fb[p.count_scale] : 0;
                mdec_search_note_bound(st, p.count_scale, (int)(next_u32(rng) % (uint32_t)(top + 1)), limit_bits);
                nb++;
                bound_proved = st.lo >= p.count_scale;
                if (bound_proved) { np++; nd++; }
                bounded = p.count_scale;
            } else {
                mdec_search_note(st, p.count_scale, tb[p.count_scale], fb[p.count_scale], limit_bits);
            }
        }
        if (p.emit_scale) {
            mdec_search_note(st, p.emit_scale, tb[p.emit_scale], fb[p.emit_scale], limit_bits);
            st.staged = p.emit_scale;
        }
        if (bounded && !bound_proved && st.lo >= bounded) nd++;       // the emit scale's evaluation proved the counted scale too
    }
    *passes = n;
    *bounds = nb;
    *proved = np;
    *diverged = nd;
    if (st.best < 64 && st.staged != st.best) return -2;
    return st.best;
}

int main() {
    int rec[4 + 128];
    while (fread(rec, sizeof(int), 4 + 128, stdin) == 4 + 128) {
        int passes = 0, bounds = 0, proved = 0, diverged = 0, p0 = 0, b0 = 0, v0 = 0, d0 = 0;
        const uint64_t seed = (uint64_t)(uint32_t)rec[3] * 2654435761ull + 1ull;
        const int r = run(rec + 4, rec + 4 + 64, rec[0], rec[1], rec[2], seed, true, &passes, &bounds, &proved, &diverged);
        const int r0 = run(rec + 4, rec + 4 + 64, rec[0], rec[1], rec[2], seed, false, &p0, &b0, &v0, &d0);
        printf("%d %d %d %d %d %d %d\n", r, passes, bounds, proved, diverged, r0, p0);
    }
    return 0;
}
