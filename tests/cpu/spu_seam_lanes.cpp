// tests/cpu/spu_seam_lanes.cpp -- TEST INFRASTRUCTURE: runs the text of psxavenc_amd/csrc/spu_seam_kernels.hip (and with it
// spu_seam_core.h) on the CPU under -fsanitize=address,undefined (tests/test_spu_seam_lanes_cpu.py), behind the wavefront model of
// the stand-in tests/cpu/hip_lanes.  The report's rows are built by the plan module's own text (spu_bank_plan.cpp).  A program, not a
// library.
//
//   spu_seam_lanes <in> <out> <order: 0 ascending, 1 descending, 2 shuffled> [seed]
// in:  records of 8 int32.
//      kind 0, the step sequence of one encode: {0, n_body, n_first, n_entries, passes, 0, 0, 0}; then n_body int32 each of the intro
//        slots, the entries and the bodies' units; n_first states (two int32) of the chains encoded once; then per pass k two tables
//        of n_body states: s_k as the statement has it and e_k, what the encoder makes of it.  The program arms the bodies (k = -1),
//        then plays the encoder between the step launches: a body that still has units must hold s_k in its state slot and in
//        `start` (exit 7 otherwise) and gets e_k.  Behind the last step a body that still has units must hold s_0 again (exit 8).
//      kind 1, one report launch: {1, format, alignment, no_leading_dummy, bank_alignment, n, has_pcm, pcm_elements}; n x
//        psxhip_spu_bank_entry_t; the bank's `total` bytes; pcm_elements int16 when has_pcm
// out: kind 0: n_entries int32 of outcome (-1 before the arming launch), then n_body int32: the units left in the device chain table;
//      kind 1: n x psxhip_spu_seam_t
// Every table is a heap block of its own that ends with its last element.
#define HIP_LANES_WAVES 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip_lanes/psxhip_api_standin.h"

#include "../../psxavenc_amd/csrc/spu_seam_kernels.hip"
#include "../../psxavenc_amd/csrc/spu_bank_plan.cpp"

namespace {
void* block16(size_t bytes) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 16)) exit(4);
    return p;
}
template <class T>
T* read_block(FILE* in, size_t count) {
    T* p = (T*)block16(sizeof(T) * count);
    if (count && fread(p, sizeof(T), count, in) != count) exit(4);
    return p;
}
bool same(const psxhip_adpcm_state_t& a, const psxhip_adpcm_state_t& b) { return a.prev1 == b.prev1 && a.prev2 == b.prev2; }
}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    hip_lanes::order = atoi(argv[3]);
    if (argc > 4) hip_lanes::seed = strtoull(argv[4], nullptr, 10);
    int32_t head[8];
    while (fread(head, sizeof head, 1, in) == 1) {
        if (head[0] == 0) {
            const int n_body = head[1], n_first = head[2], n_entries = head[3], passes = head[4];
            if (n_body < 1 || n_first < 0 || n_entries < 1 || passes < 1) return 3;
            const size_t B = (size_t)n_body;
            int32_t* intro = read_block<int32_t>(in, B);
            int32_t* entry = read_block<int32_t>(in, B);
            int32_t* units = read_block<int32_t>(in, B);
            psxhip_adpcm_state_t* first = read_block<psxhip_adpcm_state_t>(in, (size_t)n_first);
            auto* chains = (psxhip_adpcm_chain_t*)block16(sizeof(psxhip_adpcm_chain_t) * B);
            auto* states = (psxhip_adpcm_state_t*)block16(sizeof(psxhip_adpcm_state_t) * B);
            auto* start = (psxhip_adpcm_state_t*)block16(sizeof(psxhip_adpcm_state_t) * B);
            auto* outcome = (int32_t*)block16(sizeof(int32_t) * (size_t)n_entries);
            memset(chains, 0, sizeof(psxhip_adpcm_chain_t) * B);            // (no units: what an earlier encode may have left)
            memset(states, 0x5A, sizeof(psxhip_adpcm_state_t) * B);
            memset(start, 0x5A, sizeof(psxhip_adpcm_state_t) * B);
            for (int i = 0; i < n_entries; i++) outcome[i] = -1;
            psxhip_spu_seam_step_job_t job = {chains, states, first, start, intro, entry, units, outcome, n_body, -1, passes};
            if (psxhip_spu_seam_step_launch(&job, nullptr) != hipSuccess) return 6;
            std::vector<psxhip_adpcm_state_t> s0(states, states + B);
            for (int k = 0; k < passes; k++) {
                psxhip_adpcm_state_t* sk = read_block<psxhip_adpcm_state_t>(in, B);
                psxhip_adpcm_state_t* ek = read_block<psxhip_adpcm_state_t>(in, B);
                for (size_t j = 0; j < B; j++) {
                    if (chains[j].n_units == 0) continue;
                    if (chains[j].n_units != units[j] || !same(states[j], sk[j]) || !same(start[j], sk[j])) {
                        fprintf(stderr, "pass %d, body %zu: the state in front of the encoder is not s_k\n", k, j);
                        return 7;
                    }
                    states[j] = ek[j];
                }
                job.k = k;
                if (psxhip_spu_seam_step_launch(&job, nullptr) != hipSuccess) return 6;
                free(sk);
                free(ek);
            }
            for (size_t j = 0; j < B; j++)
                if (chains[j].n_units && !same(states[j], s0[j])) return 8;
            if (fwrite(outcome, sizeof(int32_t), (size_t)n_entries, out) != (size_t)n_entries) return 5;
            for (size_t j = 0; j < B; j++)
                if (fwrite(&chains[j].n_units, sizeof(int32_t), 1, out) != 1) return 5;
            free(intro); free(entry); free(units); free(first); free(chains); free(states); free(start); free(outcome);
        } else if (head[0] == 1) {
            const int n = head[5], has_pcm = head[6], pcm_elements = head[7];
            const psxhip_spu_bank_settings_t s = {head[1], head[2], head[3], head[4], 0};
            if (n < 1 || n > 65535 || pcm_elements < 0) return 3;
            std::vector<psxhip_spu_bank_entry_t> entries((size_t)n);
            if (fread(entries.data(), sizeof(psxhip_spu_bank_entry_t), (size_t)n, in) != (size_t)n) return 4;
            SpuBankPlan p;
            if (spu_bank_plan_build(&s, entries.data(), n, 0x7FFFFFFF, &p)) {
                fprintf(stderr, "the plan refused the bank: %s\n", psxhip_last_error());
                return 6;
            }
            auto* rows = (psxhip_spu_seam_row_t*)block16(sizeof(psxhip_spu_seam_row_t) * (size_t)n);
            memcpy(rows, p.seam_rows.data(), sizeof(psxhip_spu_seam_row_t) * (size_t)n);
            uint8_t* bank = read_block<uint8_t>(in, (size_t)p.total);
            // the PCM ends with its last sample: an int16 block is placed at the end of its 16-byte-aligned allocation
            const size_t pcm_bytes = sizeof(int16_t) * (size_t)pcm_elements, pad = (16 - pcm_bytes % 16) % 16;
            uint8_t* pcm_block = has_pcm ? (uint8_t*)block16(pcm_bytes + pad) : nullptr;
            if (has_pcm && pcm_bytes && fread(pcm_block + pad, 1, pcm_bytes, in) != pcm_bytes) return 4;
            auto* seam = (psxhip_spu_seam_t*)block16(sizeof(psxhip_spu_seam_t) * (size_t)n);
            memset(seam, 0x5A, sizeof(psxhip_spu_seam_t) * (size_t)n);
            psxhip_spu_seam_report_job_t job = {rows, n, bank, has_pcm ? (const int16_t*)(pcm_block + pad) : nullptr, seam};
            if (psxhip_spu_seam_report_launch(&job, nullptr) != hipSuccess) return 6;
            if (fwrite(seam, sizeof(psxhip_spu_seam_t), (size_t)n, out) != (size_t)n) return 5;
            free(seam); free(pcm_block); free(bank); free(rows);
        } else {
            return 3;
        }
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
