// reader_plan_check.cpp -- runs a table of calls through psxavenc_amd/csrc/reader_plan.cpp and prints what the plans derive, for
// tests/test_reader_plan_cpu.py to compare with its restatements and with the recorded refusals (tests/golden/reader_plan_parent.json).
// Built from reader_plan.cpp, str_plan.cpp and this file alone, with a host compiler and the host sanitizers: every case is arithmetic,
// so a call may name huge counts and made-up addresses without anything being allocated or read.
//
//   reader_plan_check <calls>
// calls: one call a line, "<kind> <has settings> <the 16 words of psxhip_str_settings_t> <k> <k numbers>", the numbers being the entry
//        point's arguments in its own order (pointers as addresses, the handle and the stream left out)
// out:   a line of constants, then per call "<kind> : <rc> | <error text>" or "<kind> : 0 | <the plan's numbers>"; each kind below
//        says which.  The plan functions are called in the order the entry point calls them.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../psxavenc_amd/csrc/adpcm_plan.h"          // (the spustreams and xastreams kinds: StreamsHostShape, inline)
#include "../../psxavenc_amd/csrc/reader_plan.h"

// the error sink: the one symbol the plan modules link against
static char g_error[512];
extern "C" void psxhip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

typedef long long ll;

static bool refused(const char* kind, int rc) {
    if (rc) printf("%s : %d | %s\n", kind, rc, g_error);
    return rc != 0;
}

// the video half, as psxhip_str_demux_device plans it: a[0 .. 15]
static int demux(const psxhip_str_settings_t* s, const ll* a, StrDemuxPlan* p) {
    const StrDemuxCall c = {s, (int)a[0], (uintptr_t)a[1], (size_t)a[2], (int)a[3], (int64_t)a[4], (int)a[5], (uintptr_t)a[6], (size_t)a[7],
                            (size_t)a[8], (uintptr_t)a[9], (uintptr_t)a[10], (uintptr_t)a[11], (int)a[12], (size_t)a[13], (uintptr_t)a[14],
                            (uintptr_t)a[15]};
    return plan_str_demux(c, p);
}

static void print_demux(const StrDemuxPlan& p) {
    printf(" %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu", p.sector_size, p.sub_at, p.hdr_at, p.chunk_cap, p.n_blocks, p.o_rec, p.o_table, p.o_blocks,
           p.o_owner, p.o_lead, p.o_min, p.o_status, p.ws_bytes);
}

// a _host reader's plan, then the return-value rules for summary counts around the capacity: "| count taken value [chains]" each
static void print_read(const ReadHostPlan& p) {
    printf(" %d %zu %zu %d %d %zu %zu %d %d %d %zu %d %d %d %zu %zu %zu %zu |", (int)p.spu, p.n, p.mf, p.sector_size, p.chunks, p.bs_stride, p.frame_bytes,
           p.dec_key[0], p.dec_key[1], p.dec_key[2], p.audio_cap, p.ch, p.d, p.B, p.src_item, p.unit_item, p.info_item, p.pcm_item);
    printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", p.o_sec, p.o_bs, p.o_sizes, p.o_info, p.o_dec, p.o_sum, p.o_asum, p.o_src, p.o_units,
           p.o_ainfo, p.o_states, p.o_pcm, p.o_px, p.reserve);
    const ll cap = (ll)p.audio_cap;
    for (ll count : {0ll, cap - 1, cap, cap + 1, cap + 7}) {
        if (count < 0) continue;
        const size_t taken = read_items_taken(p, (int32_t)std::min(count, 0x7FFFFFFFll));
        if (!p.spu) {
            printf(" | %lld %zu %d", count, taken, xa_read_returns(p, taken));
            continue;
        }
        const int n_units = strspu_read_units(p, taken);
        printf(" | %lld %zu %d", count, taken, 28 * n_units);
        psxhip_adpcm_chain_t chains[2];
        int32_t unit_base[2];
        if (n_units) strspu_read_chains(chains, unit_base, p.ch, p.d, n_units);
        for (int c = 0; n_units && c < p.ch; c++)
            printf(" %lld %d %d %d %d %d", (ll)chains[c].sample_offset, chains[c].pitch, chains[c].sample_limit, chains[c].n_units, chains[c].unit_stride,
                   unit_base[c]);
    }
}

static void print_shape(const StreamsHostShape& p) {
    printf(" %d %d %d %zu %zu %lld %lld %zu %zu %zu %zu %zu %zu %zu", p.channels, p.units_per_stream, p.per_channel, p.per, p.in_bytes, (ll)p.in_stride,
           (ll)p.out_stride, p.n_chains, p.total_sectors, p.src_bytes, p.unit_bytes, p.state_bytes, p.sample_bytes, p.status_bytes);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    printf("const %d %d %zu %zu %zu %zu %zu %zu %zu\n", kStrDemuxScanBlock, kStrspuMaxChunks, sizeof(psxhip_str_sector_t), sizeof(psxhip_str_frame_info_t),
           sizeof(psxhip_mdec_decoded_t), sizeof(psxhip_str_summary_t), sizeof(psxhip_strspu_audio_summary_t), sizeof(psxhip_strspu_chunk_info_t),
           sizeof(psxhip_adpcm_state_t));
    char kind[32];
    int has_settings;
    while (fscanf(in, "%31s %d", kind, &has_settings) == 2) {
        int32_t words[16];
        static_assert(sizeof(psxhip_str_settings_t) == sizeof words, "the settings are 16 words");
        for (int32_t& w : words)
            if (fscanf(in, "%d", &w) != 1) return 3;
        psxhip_str_settings_t settings;
        memcpy(&settings, words, sizeof settings);
        const psxhip_str_settings_t* s = has_settings ? &settings : nullptr;
        int k;
        if (fscanf(in, "%d", &k) != 1 || k < 0 || k > 32) return 3;
        std::vector<ll> a((size_t)k);
        for (ll& v : a)
            if (fscanf(in, "%lld", &v) != 1) return 3;
        g_error[0] = 0;
        const std::string name = kind;
        if (name == "demux" && k == 16) {
            StrDemuxPlan p;
            if (refused(kind, demux(s, a.data(), &p))) continue;
            printf("%s : 0 |", kind);
            print_demux(p);
        } else if (name == "strspu" && k == 18) {
            // n_streams, d_sectors, in_stride, n, first, max_frames, d_bs, bs_stride, bs_stream, d_sizes, d_info, d_units, capacity,
            // units_stream, d_chunk_info, d_table, d_summary, d_audio_summary
            StrspuDemuxPlan p;
            if (refused(kind, plan_strspu_demux(s, (int)a[0], (uintptr_t)a[11], (int)a[12], (size_t)a[13], (uintptr_t)a[14], (uintptr_t)a[17], &p))) continue;
            const psxhip_str_settings_t v = strv_settings_of(s);
            const ll video[16] = {a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], 0, 0, 0, a[15], a[16]};
            StrDemuxPlan pv;
            if (refused(kind, demux(&v, video, &pv))) continue;
            printf("%s : 0 | %d %u %d %d %u %zu %zu |", kind, p.rules.ch, p.rules.id, p.rules.d, p.rules.loop, p.rules.frequency, p.words, p.ws_bytes);
            print_demux(pv);
        } else if (name == "deint" && k == 11) {
            SpuDeinterleavePlan p;
            if (refused(kind, plan_spu_deinterleave((uintptr_t)a[0], (int)a[1], (size_t)a[2], (size_t)a[3], (size_t)a[4], (int)a[5], (uintptr_t)a[6], (int)a[7],
                                                    (size_t)a[8], (uintptr_t)a[9], (size_t)a[10], &p)))
                continue;
            printf("%s : 0 | %zu %zu %d", kind, p.blocks, p.records, (int)p.vec16);
        } else if ((name == "read" && k == 11) || (name == "readspu" && k == 12)) {
            // sectors, n, first, max_frames, frames, info, decoded, pcm, pcm_capacity, status / chunk records, summary[, audio summary]
            const ReadHostCall c = {s, (int)a[1], (int)a[3], (int64_t)a[8], a[0] != 0, a[4] != 0, a[5] != 0, a[6] != 0, a[7] != 0, a[10] != 0};
            ReadHostPlan p;
            if (refused(kind, plan_read_host(name == "readspu", c, &p))) continue;
            printf("%s : 0 |", kind);
            print_read(p);
        } else if (name == "spustreams" && k == 7) {
            // blocks, n_streams, in_stride, n_blocks, states, samples, out_stride
            StreamsHostShape p;
            if (refused(kind, spu_streams_host_shape((int)a[1], (int64_t)a[2], (int)a[3], a[0] && a[4] && a[5], (int64_t)a[6], &p))) continue;
            printf("%s : 0 |", kind);
            print_shape(p);
        } else if (name == "xastreams" && k == 12) {
            // format, stereo, frequency, bits, sectors, n_streams, in_stride, n_sectors, states, samples, out_stride, status
            StreamsHostShape p;
            if (refused(kind, xa_streams_host_shape((int)a[0], (int)a[1], (int)a[3], (int)a[5], (int64_t)a[6], (int)a[7], a[4] && a[8] && a[9], (int64_t)a[10], &p)))
                continue;
            printf("%s : 0 |", kind);
            print_shape(p);
        } else {
            return 3;
        }
        printf("\n");
    }
    fclose(in);
    return 0;
}
