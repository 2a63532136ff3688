// adpcm_decode_sim.cpp -- psxavenc_amd/csrc/adpcm_decode_core.h on the CPU (built with -fsanitize=address,undefined by
// tests/test_adpcm_decode_core_cpu.py): the unit step and code unpacking the kernels compile, and the chunk / verify schedule of
// adpcm_decode_kernel as a host model -- every chunk's assumed start, decode again from the truth until the stored end state is met,
// passes to the fixpoint.
//
// usage: adpcm_decode_sim IN OUT.  IN is a sequence of cases: int32 {bits, filter_count, n_units, p1, p2, chunk_units, warmup_units,
// sample_limit} + n_units records.  chunk_units 0 = serial.  OUT per case: int32 {p1, p2, passes} + 28 n_units int16 samples +
// n_units flag bytes.  Samples at index >= sample_limit are decoded but left 0x7777, as the kernel leaves them unstored.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../psxavenc_amd/csrc/adpcm_decode_core.h"

namespace {

struct State {
    int p1, p2;
    bool operator==(const State& o) const { return p1 == o.p1 && p2 == o.p2; }
    bool operator!=(const State& o) const { return !(*this == o); }
};

struct Case {
    int bits, filter_count, n_units, limit;
    std::vector<uint8_t> rec;
    std::vector<int16_t> pcm;
    std::vector<uint8_t> flags;

    int rec_bytes() const { return bits == 4 ? 16 : 32; }

    // decode unit u from s; store what lies below the limit
    void unit(int u, State& s, bool store) {
        uint32_t w[8], out[14];
        memcpy(w, rec.data() + (size_t)u * rec_bytes(), (size_t)rec_bytes());
        const int f = bits == 4 ? adpcm_dec_unit<4>(w, filter_count, s.p1, s.p2, out) : adpcm_dec_unit<8>(w, filter_count, s.p1, s.p2, out);
        if (!store) return;
        flags[u] = (uint8_t)f;
        for (int i = 0; i < 28; i++)
            if ((long long)u * 28 + i < limit) pcm[(size_t)u * 28 + i] = (int16_t)(uint16_t)(out[i >> 1] >> (16 * (i & 1)));
    }
};

int run_serial(Case& c, State& s) {
    for (int u = 0; u < c.n_units; u++) c.unit(u, s, true);
    return 0;
}

int run_chunked(Case& c, State& s, int chunk_units, int warmup_units) {
    const int n_chunks = (c.n_units + chunk_units - 1) / chunk_units;
    std::vector<State> used((size_t)n_chunks), end((size_t)n_chunks);
    // speculate: every chunk at once, all but the first from a guess
    for (int k = 0; k < n_chunks; k++) {
        const int first = k * chunk_units, count = c.n_units - first < chunk_units ? c.n_units - first : chunk_units;
        State t = {0, 0};
        if (first == 0) t = s;
        const int warm = first ? adpcm_dec_warm(first, warmup_units) : 0;
        for (int u = first - warm; u < first; u++) c.unit(u, t, false);
        used[k] = t;
        for (int u = first; u < first + count; u++) c.unit(u, t, true);
        end[k] = t;
    }
    int passes = 0;
    for (bool changed = true; changed;) {
        changed = false;
        passes++;
        const std::vector<State> seen = end;          // a pass reads its predecessors' ends as they were when it started
        for (int k = 1; k < n_chunks; k++) {
            if (used[k] == seen[k - 1]) continue;
            changed = true;
            used[k] = seen[k - 1];
            const int first = k * chunk_units, count = c.n_units - first < chunk_units ? c.n_units - first : chunk_units;
            State t = used[k];
            bool running = true;
            for (int u = first; u < first + count && running; u++) {
                State old = {0, 0};
                const bool stored = adpcm_dec_unit_stored(u, c.limit);
                if (stored) old = {c.pcm[(size_t)u * 28 + 27], c.pcm[(size_t)u * 28 + 26]};
                c.unit(u, t, true);
                if (stored && old == t) running = false;
            }
            if (running) end[k] = t;
        }
    }
    if (n_chunks) s = end[(size_t)n_chunks - 1];
    return passes;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t head[8];
    while (fread(head, sizeof head, 1, in) == 1) {
        Case c;
        c.bits = head[0]; c.filter_count = head[1]; c.n_units = head[2]; c.limit = head[7];
        if ((c.bits != 4 && c.bits != 8) || c.n_units < 0 || head[5] < 0) return 3;
        c.rec.resize((size_t)c.n_units * c.rec_bytes());
        if (!c.rec.empty() && fread(c.rec.data(), c.rec.size(), 1, in) != 1) return 3;
        c.pcm.assign((size_t)c.n_units * 28, 0x7777);
        c.flags.assign((size_t)c.n_units, 0);
        State s = {head[3], head[4]};
        const int passes = head[5] > 0 ? run_chunked(c, s, head[5], head[6]) : run_serial(c, s);
        const int32_t res[3] = {s.p1, s.p2, passes};
        fwrite(res, sizeof res, 1, out);
        if (c.n_units) {
            fwrite(c.pcm.data(), sizeof(int16_t), c.pcm.size(), out);
            fwrite(c.flags.data(), 1, c.flags.size(), out);
        }
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}
