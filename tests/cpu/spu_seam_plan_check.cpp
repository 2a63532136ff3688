// spu_seam_plan_check.cpp -- runs a table of banks through psxavenc_amd/csrc/spu_bank_plan.cpp and prints the seam tables the plan
// derives ("psxhip SPU loop seam v1"), for tests/test_spu_seam_plan_cpu.py to compare with its restatement;
// and, beside them, what the plan derived before there were seam tables, which must not have moved.  Built from spu_bank_plan.cpp and
// this file alone, with a host compiler and the host sanitizers.
//
//   spu_seam_plan_check <banks>
// banks: the format of tests/cpu/spu_bank_plan_check.cpp
// out:   per bank "<rc> | <error text>", or "0 | <total> <total_units> <tiles> <seam_first> <seam_body>", then a line per entry
//        "e <offset> <size> <the row's eight numbers> <the chain's five numbers> <unit_base> <seam block> <the seam row's five numbers>",
//        a line per seam chain "c <the chain's five numbers> <unit_base>", a line per body chain "b <entry> <intro slot>" and a line per
//        tile "t <entry> <part> <first> <count>"
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
        g_error[0] = 0;
        SpuBankPlan p;
        const int rc = spu_bank_plan_build(has_settings ? &s : nullptr, has_entries ? entries.data() : nullptr, n, threshold, &p);
        if (rc) {
            printf("%d | %s\n", rc, g_error);
            continue;
        }
        const size_t N = (size_t)n;
        printf("0 | %lld %lld %zu %d %d\n", (ll)p.total, (ll)p.total_units, p.tiles.size(), p.seam_first, p.seam_body);
        if (p.seam_block.size() != N || p.seam_rows.size() != N || p.seam_chains.size() != (size_t)(p.seam_first + p.seam_body) ||
            p.seam_unit_base.size() != p.seam_chains.size() || p.seam_body_entry.size() != (size_t)p.seam_body ||
            p.seam_body_intro.size() != (size_t)p.seam_body)
            return 4;
        for (size_t i = 0; i < N; i++) {
            const psxhip_spu_bank_row_t& r = p.rows[i];
            const psxhip_adpcm_chain_t& c = p.chains[i];
            const psxhip_spu_seam_row_t& q = p.seam_rows[i];
            printf("e %lld %lld %d %d %d %d %d %d %d %d %lld %d %d %d %d %d %d %lld %d %d %d %d\n", (ll)p.offsets[i], (ll)p.sizes[i], r.first_word,
                   r.header_words, r.dummy, r.data_blocks, r.trap, r.end_word, r.loop_start_block, r.loop_repeat, (ll)c.sample_offset, c.pitch,
                   c.sample_limit, c.n_units, c.unit_stride, p.unit_base[i], p.seam_block[i], (ll)q.pcm_offset, q.samples, q.first_block,
                   q.data_blocks, q.seam_block);
        }
        for (size_t k = 0; k < p.seam_chains.size(); k++) {
            const psxhip_adpcm_chain_t& c = p.seam_chains[k];
            printf("c %lld %d %d %d %d %d\n", (ll)c.sample_offset, c.pitch, c.sample_limit, c.n_units, c.unit_stride, p.seam_unit_base[k]);
        }
        for (int j = 0; j < p.seam_body; j++) printf("b %d %d\n", p.seam_body_entry[(size_t)j], p.seam_body_intro[(size_t)j]);
        for (const psxhip_spu_bank_tile_t& t : p.tiles) printf("t %d %d %d %d\n", t.entry, t.part, t.first, t.count);
    }
    fclose(in);
    return 0;
}
