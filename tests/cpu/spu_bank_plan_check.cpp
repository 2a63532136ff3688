// spu_bank_plan_check.cpp -- runs a table of banks through psxavenc_amd/csrc/spu_bank_plan.cpp and prints what the plan derives, for
// tests/test_spu_bank_plan_cpu.py to compare with its restatement and with psxhip_spu_file_size.  Built from spu_bank_plan.cpp and
// this file alone, with a host compiler and the host sanitizers: every case is arithmetic, so a bank may name huge sample counts
// without anything being allocated or read.
//
//   spu_bank_plan_check <banks>
// banks: per bank a line "<has settings> <format> <alignment> <no_leading_dummy> <bank_alignment> <beam> <has entries> <n> <threshold> <m>"
//        and m lines "<pcm_offset> <samples> <frequency> <loop point> <enable_loop> <name, 32 hex digits>": the first m entries; the
//        entries behind them, up to n, repeat the last one
// out:   per bank "<rc> | <error text>", or "0 | <total> <chunked> <max_units> <total_units> <pcm_elements> <tiles>", then a line per
//        entry "e <offset> <size> <the row's eight numbers> <header, 96 hex digits> <the chain's five numbers> <unit_base>" and a
//        line per tile "t <entry> <part> <first> <count>"; then what psxhip_spu_bank_plan answers for the same bank: "p <rc> <total>"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../psxavenc_amd/csrc/spu_bank_plan.h"

// the error sink: the one symbol the plan module links against
static char g_error[512];
extern "C" void psxhip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

typedef long long ll;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    int has_settings, has_entries, n, threshold, m;
    psxhip_spu_bank_settings_t s;
    while (fscanf(in, "%d %d %d %d %d %d %d %d %d %d", &has_settings, &s.format, &s.alignment, &s.no_leading_dummy, &s.bank_alignment, &s.beam,
                  &has_entries, &n, &threshold, &m) == 10) {
        if (m < 0 || m > 65536) return 3;
        std::vector<psxhip_spu_bank_entry_t> entries;
        for (int i = 0; i < m; i++) {
            psxhip_spu_bank_entry_t e;
            ll offset, samples;
            char hex[40];
            if (fscanf(in, "%lld %lld %d %d %d %32s", &offset, &samples, &e.audio_frequency, &e.audio_loop_point, &e.enable_loop, hex) != 6) return 3;
            if (strlen(hex) != 32) return 3;
            e.pcm_offset = offset;
            e.samples = samples;
            for (int k = 0; k < 16; k++) {
                unsigned v;
                if (sscanf(hex + 2 * k, "%2x", &v) != 1) return 3;
                e.name[k] = (char)v;
            }
            entries.push_back(e);
        }
        while (m > 0 && (int)entries.size() < n) entries.push_back(entries.back());
        const psxhip_spu_bank_entry_t* ep = has_entries ? entries.data() : nullptr;
        const psxhip_spu_bank_settings_t* sp = has_settings ? &s : nullptr;
        g_error[0] = 0;
        SpuBankPlan p;
        const int rc = spu_bank_plan_build(sp, ep, n, threshold, &p);
        if (rc) {
            printf("%d | %s\n", rc, g_error);
        } else {
            printf("0 | %lld %d %d %lld %lld %zu\n", (ll)p.total, (int)p.chunked, p.max_units, (ll)p.total_units, (ll)p.pcm_elements, p.tiles.size());
            if (p.offsets.size() != (size_t)n || p.sizes.size() != (size_t)n || p.rows.size() != (size_t)n || p.chains.size() != (size_t)n ||
                p.unit_base.size() != (size_t)n)
                return 4;
            for (int i = 0; i < n; i++) {
                const psxhip_spu_bank_row_t& r = p.rows[(size_t)i];
                const psxhip_adpcm_chain_t& c = p.chains[(size_t)i];
                printf("e %lld %lld %d %d %d %d %d %d %d %d ", (ll)p.offsets[(size_t)i], (ll)p.sizes[(size_t)i], r.first_word, r.header_words, r.dummy,
                       r.data_blocks, r.trap, r.end_word, r.loop_start_block, r.loop_repeat);
                const uint8_t* h = (const uint8_t*)r.header;
                for (int k = 0; k < 48; k++) printf("%02x", h[k]);
                printf(" %lld %d %d %d %d %d\n", (ll)c.sample_offset, c.pitch, c.sample_limit, c.n_units, c.unit_stride, p.unit_base[(size_t)i]);
            }
            for (const psxhip_spu_bank_tile_t& t : p.tiles) printf("t %d %d %d %d\n", t.entry, t.part, t.first, t.count);
        }
        // the public function: the same refusals, and the layout into the caller's arrays (no more than n elements are written)
        std::vector<int64_t> offsets((size_t)(n > 0 ? n : 0)), sizes((size_t)(n > 0 ? n : 0));
        int64_t total = -1;
        const int prc = psxhip_spu_bank_plan(sp, ep, n, offsets.data(), sizes.data(), &total);
        if (prc != rc) return 5;
        if (!prc && (total != p.total || offsets != p.offsets || sizes != p.sizes)) return 5;
        if (!prc && psxhip_spu_bank_plan(sp, ep, n, nullptr, nullptr, nullptr) != 0) return 5;
        printf("p %d %lld\n", prc, (ll)total);
    }
    fclose(in);
    return 0;
}
