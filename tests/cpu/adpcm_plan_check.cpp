// adpcm_plan_check.cpp -- runs a table of calls through psxavenc_amd/csrc/adpcm_plan.cpp and prints what the plans derive, for
// tests/test_adpcm_plan_cpu.py to compare with its restatements and with the recorded refusals (tests/golden/adpcm_plan_parent.json).
// Built from adpcm_plan.cpp and this file alone, with a host compiler and the host sanitizers: every case is arithmetic, so a call
// may name made-up addresses without anything being read through them.
//
//   adpcm_plan_check <calls>
// calls: one call a line, "<kind> <k> <k numbers>".  The kinds named after entry points take the entry point's arguments in its own
//        order (pointers as addresses; the device, the stream and the session's handle pointer left out; decchunked with the chain
//        table behind them, 5 numbers a chain) and call the plan functions in the order the entry point calls them.  The other kinds
//        ask one plan function; each says below what it takes.
// out:   a line of constants, then per call "<kind> : <rc> | <error text>" for a refusal; "<kind> : 0 | early <v>" where the entry point
//        returns v before it asks for the device, "<kind> : 0 | device" where it goes on to the device; "<kind> : 0 | <numbers>" for
//        the other kinds.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../psxavenc_amd/csrc/adpcm_plan.h"

// the error sink: the one symbol the plan module links against
static char g_error[512];
extern "C" void psxhip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

typedef long long ll;
typedef uintptr_t up;

template <class T> static void print_list(const std::vector<T>& v) {
    printf(" |");
    for (const T& x : v) printf(" %lld", (ll)x);
}

// what an entry point answers behind its plan: a refusal, a value at once, or the device
static void answer(const char* kind, int rc, bool early = false, int value = 0) {
    if (rc) printf("%s : %d | %s\n", kind, rc, g_error);
    else if (early) printf("%s : 0 | early %d\n", kind, value);
    else printf("%s : 0 | device\n", kind);
}

static int session_create(const ll* a) {        // d_samples, chains, unit_base, lead_units, n_chains, filter_count, bits, d_units, chunk_units, warmup_units
    return adpcm_session_create_check((up)a[0], a[1] != 0, a[2] != 0, (up)a[7], (int)a[4], (int)a[5], (int)a[6], (int)a[8], (int)a[9]);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    printf("const %d %zu %zu %zu %d %zu %zu %d\n", kAdpcmCallStageMax, kAdpcmCallIn, kAdpcmCallOut, kAdpcmCallStates, kAdpcmVerifyBatchMax,
           sizeof(psxhip_adpcm_chain_t), sizeof(psxhip_adpcm_state_t), PSXHIP_ADPCM_RECORD_BYTES);
    char kind[32];
    int k;
    while (fscanf(in, "%31s %d", kind, &k) == 2) {
        if (k < 0 || k > 100000) return 3;
        std::vector<ll> a((size_t)k);
        for (ll& v : a)
            if (fscanf(in, "%lld", &v) != 1) return 3;
        g_error[0] = 0;
        const std::string name = kind;
        // ---- the entry points
        if (name == "enc" && k == 8) {                  // d_samples, d_chains, d_unit_base, n_chains, filter_count, bits, d_states, d_units
            answer(kind, adpcm_encode_chains_check(kEncodeChains, (up)a[0], (up)a[1], (up)a[2], (up)a[6], (up)a[7], (int)a[3], (int)a[4], (int)a[5], 0, 0));
        } else if (name == "encbeam" && k == 10) {      // ..., bits, beam, d_states, d_units, d_unit_err
            answer(kind, adpcm_encode_chains_check(kBeamEncodeChains, (up)a[0], (up)a[1], (up)a[2], (up)a[7], (up)a[8], (int)a[3], (int)a[4], (int)a[5],
                                                   (int)a[6], (up)a[9]));
        } else if (name == "session" && k == 10) {
            answer(kind, session_create(a.data()));
        } else if (name == "setbeam" && k == 3) {       // session, beam, speculated (the last is the session's own, not an argument)
            answer(kind, adpcm_session_beam_check(a[0] != 0, (int)a[1], a[2] != 0));
        } else if ((name == "chunked" && k == 11) || (name == "chunkedbeam" && k == 12)) {
            // d_samples, chains, unit_base, n_chains, filter_count, bits, d_states, d_units, [beam,] chunk_units, warmup_units, max_passes
            const bool beam = name == "chunkedbeam";
            const int rc = adpcm_encode_chunked_check(beam, beam ? (int)a[8] : 0, (up)a[6]);
            if (rc || a[3] == 0) {
                answer(kind, rc, true, 0);
                continue;
            }
            const ll* t = a.data() + (beam ? 9 : 8);
            const ll s[10] = {a[0], a[1], a[2], 0, a[3], a[4], a[5], a[7], t[0], t[1]};
            answer(kind, session_create(s));
        } else if (name == "pack" && k == 3) {          // d_units, n_blocks, d_out
            answer(kind, spu_pack_check((up)a[0], (int)a[1], (up)a[2]));
        } else if (name == "scatter" && k == 16) {
            // d_units, n_sectors, format, stereo, frequency, bits, file, channel, first_lba, d_eof_flags, eof_bits, d_out, d_dst_sector, n_streams, strides
            answer(kind, xa_assemble_check((up)a[0], (up)a[11], (int)a[1], (int)a[13], (int)a[2], (int)a[5], (size_t)a[14], (size_t)a[15]));
        } else if (name == "dec" && k == 10) {          // d_units, d_chains, d_unit_base, n_chains, filter_count, bits, d_states, d_samples, d_unit_flags, d_tail
            answer(kind, adpcm_decode_chains_check(false, (up)a[0], a[1] != 0, a[2] != 0, (up)a[6], (up)a[7], (up)a[9], (int)a[3], (int)a[4], (int)a[5]));
        } else if (name == "decchunked" && k >= 13 && (k - 13) % 5 == 0) {
            // ... the same ten, chunk_units, warmup_units, max_passes; then the chain table (none: `chains` is only an address)
            int rc = adpcm_decode_chains_check(true, (up)a[0], a[1] != 0, a[2] != 0, (up)a[6], (up)a[7], (up)a[9], (int)a[3], (int)a[4], (int)a[5]);
            std::vector<psxhip_adpcm_chain_t> chains((size_t)(k - 13) / 5);
            for (size_t c = 0; c < chains.size(); c++) {
                const ll* v = a.data() + 13 + 5 * c;
                chains[c] = {(int64_t)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4]};
            }
            ll total = 0;
            if (!rc && (ll)chains.size() < a[3]) return 3;      // an accepted call's table is read
            if (!rc) rc = adpcm_decode_chunked_chains_check(chains.data(), (int)a[3], &total);
            answer(kind, rc);
        } else if (name == "sse" && k == 8) {           // d_a, d_a_tail, d_b, d_chains, n_chains, d_unit_sse, d_unit_base, d_chain_sums
            answer(kind, adpcm_sse_check((up)a[0], (up)a[1], (up)a[2], (up)a[3], (int)a[4], (up)a[5], (up)a[6], (up)a[7]));
        } else if (name == "dis" && k == 8) {           // d_sectors, n_sectors, format, stereo, frequency, bits, d_units, d_sector_status
            answer(kind, xa_disassemble_check((up)a[0], (int)a[1], (int)a[2], (int)a[5], (up)a[6], (up)a[7]));
        } else if ((name == "spuhost" && k == 8) || (name == "spuhostbeam" && k == 9)) {
            // samples, n_streams, stream_stride, pitch, samples_per_stream, states, out, out_stride[, beam]
            int rc = k == 9 ? adpcm_host_beam_check("spu_encode_streams_host_beam", (int)a[8]) : 0;
            SpuEncodeShape p = SpuEncodeShape();
            if (!rc) rc = spu_encode_shape(a[0] && a[5] && a[6], (int)a[1], (int64_t)a[2], (int)a[3], (int)a[4], (int64_t)a[7], &p);
            answer(kind, rc, p.empty, p.bytes);
        } else if ((name == "xahost" && k == 15) || (name == "xahostbeam" && k == 16)) {
            // format, stereo, frequency, bits, file, channel, samples, n_streams, stream_stride, samples_per_stream, lbas, states, out, out_stride, finalize[, beam]
            int rc = k == 16 ? adpcm_host_beam_check("xa_encode_streams_host_beam", (int)a[15]) : 0;
            XaEncodeShape p = XaEncodeShape();
            if (!rc) rc = xa_encode_shape(a[6] && a[11] && a[12], (int)a[0], (int)a[1], (int)a[3], (int)a[7], (int64_t)a[8], (int)a[9], (int64_t)a[13], &p);
            answer(kind, rc, p.empty, p.bytes);
        }
        // ---- one plan function each
        else if (name == "threshold" && k == 1) {       // n_chains
            printf("%s : 0 | %d\n", kind, adpcm_chunked_threshold((int)a[0]));
        } else if (name == "route" && k == 2) {         // units_per_chain, n_chains
            printf("%s : 0 | %d\n", kind, (int)adpcm_route_chunked((int)a[0], (int)a[1]));
        } else if (name == "spufast" && k == 5) {       // beam, n_streams, n_units, stage_max, out_max
            printf("%s : 0 | %d\n", kind, (int)spu_call_fast_path((int)a[0], (int)a[1], (int)a[2], (size_t)a[3], (size_t)a[4]));
        } else if (name == "xafast" && k == 7) {        // beam, n_streams, sectors, per, bytes, stage_max, out_max
            printf("%s : 0 | %d\n", kind, (int)xa_call_fast_path((int)a[0], (int)a[1], (int)a[2], (size_t)a[3], (size_t)a[4], (size_t)a[5], (size_t)a[6]));
        } else if (name == "chunking" && k == 3) {      // total_units, rows, n_cu
            const AdpcmChunking c = adpcm_chunking(a[0], (int)a[1], (int)a[2]);
            printf("%s : 0 | %d %d\n", kind, c.chunk_units, c.warmup_units);
        } else if (name == "decchunking" && k == 2) {   // total_units, n_cu
            printf("%s : 0 | %d\n", kind, adpcm_decode_chunking(a[0], (int)a[1]));
        } else if (name == "sessionplan" && k >= 2 && (k - 2) % 2 == 0) {       // chunk_units, has lead_units; then n_units and lead_units per chain
            const size_t n = (size_t)(k - 2) / 2;
            std::vector<psxhip_adpcm_chain_t> chains(n);
            std::vector<int32_t> lead(n);
            for (size_t c = 0; c < n; c++) {
                chains[c] = {0, 1, 0, (int)a[2 + 2 * c], 1};
                lead[c] = (int32_t)a[3 + 2 * c];
            }
            AdpcmSessionPlan p;
            adpcm_session_plan(chains.data(), a[1] ? lead.data() : nullptr, (int)n, (int)a[0], &p);
            printf("%s : 0 | %lld %d | %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", kind, (ll)p.total_units, p.n_chunks, p.o_chains, p.o_base, p.o_sbase,
                   p.o_lead, p.o_cstates, p.o_final, p.o_known, p.o_flags, p.o_cchain, p.o_cfirst, p.o_used, p.o_ustates, p.bytes);
            print_list(p.state_base);
            print_list(p.chunk_chain);
            print_list(p.chunk_first);
            print_list(p.lead);
            printf("\n");
        } else if (name == "decodeplan" && k >= 1 && (k - 1) % 3 == 0) {        // chunk_units; then sample_offset, pitch and n_units per chain
            const size_t n = (size_t)(k - 1) / 3;
            std::vector<psxhip_adpcm_chain_t> chains(n);
            for (size_t c = 0; c < n; c++) chains[c] = {(int64_t)a[1 + 3 * c], (int)a[2 + 3 * c], 0, (int)a[3 + 3 * c], 1};
            AdpcmDecodePlan p;
            const int rc = adpcm_decode_plan(chains.data(), (int)n, (int)a[0], &p);
            if (rc) {
                answer(kind, rc);
                continue;
            }
            printf("%s : 0 | %zu | %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", kind, p.n_chunks, p.o_chains, p.o_base, p.o_cc, p.o_cf, p.o_cp, p.o_last, p.o_used,
                   p.o_end, p.o_flags, p.bytes);
            print_list(p.chunk_chain);
            print_list(p.chunk_first);
            print_list(p.chunk_pred);
            print_list(p.last_chunk);
            printf("\n");
        } else if (name == "spushape" && k == 5) {      // n_streams, stream_stride, pitch, samples_per_stream, out_stride
            SpuEncodeShape p;
            const int rc = spu_encode_shape(true, (int)a[0], (int64_t)a[1], (int)a[2], (int)a[3], (int64_t)a[4], &p);
            if (rc) {
                answer(kind, rc);
                continue;
            }
            printf("%s : 0 | %d %d %d %lld %lld %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", kind, p.n_units, p.bytes, (int)p.empty, (ll)p.stream_stride, (ll)p.out_stride,
                   p.per, p.readable, p.row, p.sample_bytes, p.chain_bytes, p.base_bytes, p.state_bytes, p.unit_bytes, p.out_bytes);
        } else if (name == "xashape" && k >= 9) {
            // format, stereo, bits, n_streams, stream_stride, samples_per_stream, out_stride, finalize, has eof_flags; then the flags
            XaEncodeShape p;
            const int rc = xa_encode_shape(true, (int)a[0], (int)a[1], (int)a[2], (int)a[3], (int64_t)a[4], (int)a[5], (int64_t)a[6], &p);
            if (rc) {
                answer(kind, rc);
                continue;
            }
            printf("%s : 0 | %d %d %d %d %d %d %d %lld %lld %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", kind, p.xa.channels, p.groups, p.sectors, p.bytes, (int)p.empty,
                   p.units_per_stream, p.units_per_chain, (ll)p.stream_stride, (ll)p.out_stride, p.per, p.row, p.n_chains, p.sample_bytes, p.chain_bytes,
                   p.base_bytes, p.state_bytes, p.unit_bytes, p.out_bytes, p.eof_bytes);
            if (!p.empty) {
                std::vector<uint8_t> flags(a.begin() + 9, a.end());
                if (a[8] && flags.size() != (size_t)a[3] * p.sectors) return 3;
                printf(" | %u", xa_encode_eof_bits(p.sectors, a[8] ? flags.data() : nullptr, (int)a[7]));
                print_list(xa_encode_eof_table((int)a[3], p.sectors, a[8] ? flags.data() : nullptr, (int)a[7]));
            }
            printf("\n");
        } else {
            return 3;
        }
    }
    fclose(in);
    return 0;
}
