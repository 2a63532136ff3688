// tests/cpu/adpcm_beam_lanes.cpp -- TEST INFRASTRUCTURE: runs the text of psxavenc_amd/csrc/adpcm_beam_kernels.hip and of the
// encoder's host layer psxavenc_amd/csrc/psxhip_adpcm_encode.cpp (the beam entry points, the session and its verify passes) on the
// CPU under -fsanitize=address,undefined (tests/test_adpcm_beam_lanes_cpu.py), behind the wavefront model of the stand-in
// tests/cpu/hip_lanes.  A record is one call of psxhip_adpcm_beam_encode_chains_device (kind 0), of
// psxhip_adpcm_beam_encode_chains_chunked (kind 1) or a session with psxhip_adpcm_session_set_beam that is run from wrong start
// states first and from the right ones then (kind 2).  The plain encoder's kernels (adpcm_kernels.hip: inline assembly) and the
// packers are not part of this program: their launch functions are stand-ins that fail, but for the gather of the chains' final
// states, which is restated here in two lines.  A program, not a library.
//
//   adpcm_beam_lanes <in> <out> <order: 0 ascending, 1 descending, 2 shuffled> [seed]
// in:  records of 16 int32 {kind, bits, filter_count, n_chains, n_records, total_samples, beam, has_err, chunk_units, warmup_units,
//      max_passes, fill, 0, 0, 0, 0}; n_chains x psxhip_adpcm_chain_t; n_chains x int32 unit_base; n_chains x psxhip_adpcm_state_t;
//      total_samples int16
// out: the records (n_records x PSXHIP_ADPCM_RECORD_SIZE(bits) bytes that held `fill`), the states, the errors (n_records uint32 that
//      held `fill`) when has_err
// Every buffer is a heap block of its own that ends with the last element include/psxav_hip.h lets the call touch, and starts behind
// an offset that keeps only the promised alignment: samples 2 bytes, the errors 4, the records 16 (4-bit) or 4 (8-bit).
#define HIP_LANES_WAVES 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip_lanes/psxhip_api_standin.h"

#include "../../psxavenc_amd/csrc/adpcm_beam_kernels.hip"
#include "../../psxavenc_amd/csrc/adpcm_plan.cpp"
#include "../../psxavenc_amd/csrc/psxhip_adpcm_encode.cpp"

// what psxhip_adpcm_encode.cpp takes from adpcm_kernels.hip, sector_kernels.hip and the device (its plans are adpcm_plan.cpp's own text)
int psxhip_adpcm_device_cus(int) { return 4; }
extern "C" hipError_t psxhip_adpcm_chains_launch(const psxhip_adpcm_chain_job_t*, void*) { return 1; }
extern "C" hipError_t psxhip_adpcm_chunks_launch(const psxhip_adpcm_chunk_job_t*, int, void*) { return 1; }
extern "C" hipError_t psxhip_spu_pack_launch(const uint8_t*, int, uint8_t*, void*) { return 1; }
extern "C" hipError_t psxhip_xa_assemble_launch(const psxhip_xa_job_t*, int, void*) { return 1; }
extern "C" int psxhip_sector_tables(int) { return PSXHIP_EDEVICE; }
extern "C" hipError_t psxhip_adpcm_final_states_launch(const psxhip_adpcm_chain_t* chains, const int64_t* state_base, int n_chains,
                                                       const psxhip_adpcm_state_t* unit_states, psxhip_adpcm_state_t* states, void*) {
    for (int c = 0; c < n_chains; c++)
        if (chains[c].n_units > 0) states[c] = unit_states[state_base[c] + chains[c].n_units - 1];
    return hipSuccess;
}

namespace {
struct Block {
    uint8_t* all = nullptr;
    size_t offset = 0, size = 0;
    int fill = 0;
    uint8_t* make(size_t offset_, size_t size_, int fill_) {
        offset = offset_; size = size_; fill = fill_;
        all = (uint8_t*)malloc(offset + size);
        if (!all) exit(4);
        memset(all, fill, offset + size);
        return all + offset;
    }
    bool load(FILE* in) { return !size || fread(all + offset, 1, size, in) == size; }
    bool front_kept() const {
        for (size_t i = 0; i < offset; i++)
            if (all[i] != (uint8_t)fill) return false;
        return true;
    }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    hip_lanes::order = atoi(argv[3]);
    if (argc > 4) hip_lanes::seed = strtoull(argv[4], nullptr, 10);
    int32_t head[16];
    while (fread(head, sizeof head, 1, in) == 1) {
        const int kind = head[0], bits = head[1], filter_count = head[2], nc = head[3], n_records = head[4], total = head[5], beam = head[6],
                  has_err = head[7], chunk_units = head[8], warmup_units = head[9], max_passes = head[10], fill = head[11];
        if (kind < 0 || kind > 2 || nc < 0 || n_records < 0 || total < 0 || (bits != 4 && bits != 8)) return 3;
        Block chains, base, states, samples, units, err;
        auto* d_chains = (psxhip_adpcm_chain_t*)chains.make(0, (size_t)nc * sizeof(psxhip_adpcm_chain_t), fill);
        auto* d_base = (int32_t*)base.make(0, (size_t)nc * 4, fill);
        auto* d_states = (psxhip_adpcm_state_t*)states.make(0, (size_t)nc * sizeof(psxhip_adpcm_state_t), fill);
        auto* d_samples = (int16_t*)samples.make(2, (size_t)total * 2, fill);
        if (!chains.load(in) || !base.load(in) || !states.load(in) || !samples.load(in)) return 4;
        auto* d_units = units.make(bits == 4 ? 16 : 4, (size_t)n_records * (bits == 4 ? 16 : 32), fill);
        auto* d_err = has_err ? (uint32_t*)err.make(4, (size_t)n_records * 4, fill) : nullptr;
        int rc;
        if (kind == 0) {
            rc = psxhip_adpcm_beam_encode_chains_device(0, d_samples, d_chains, d_base, nc, filter_count, bits, beam, d_states, d_units, d_err, nullptr);
        } else if (kind == 1) {
            rc = psxhip_adpcm_beam_encode_chains_chunked(0, d_samples, d_chains, d_base, nc, filter_count, bits, d_states, d_units, beam, chunk_units,
                                                         warmup_units, max_passes, nullptr);
            if (rc == 0 && nc > 0) return 8;            // (at least the pass that finds nothing)
        } else {
            psxhip_adpcm_session_t* s = nullptr;
            rc = psxhip_adpcm_session_create(&s, 0, d_samples, d_chains, d_base, nullptr, nc, filter_count, bits, d_units, chunk_units, warmup_units, nullptr);
            if (rc == 0) rc = psxhip_adpcm_session_set_beam(s, beam);
            std::vector<psxhip_adpcm_state_t> wrong((size_t)nc), final_states((size_t)nc);
            for (int c = 0; c < nc; c++) {
                wrong[(size_t)c].prev1 = d_states[c].prev2 ^ 0x155;
                wrong[(size_t)c].prev2 = -d_states[c].prev1 / 2;
            }
            if (rc == 0) rc = psxhip_adpcm_session_run(s, wrong.data(), nullptr, max_passes, final_states.data(), nullptr);
            if (rc >= 0 && psxhip_adpcm_session_set_beam(s, beam) != PSXHIP_EINVAL) return 9;       // refused behind a run
            if (rc >= 0) rc = psxhip_adpcm_session_run(s, d_states, nullptr, max_passes, final_states.data(), nullptr);
            if (rc >= 0) memcpy(d_states, final_states.data(), (size_t)nc * sizeof(psxhip_adpcm_state_t));
            psxhip_adpcm_session_destroy(s);
        }
        if (rc < 0) {
            fprintf(stderr, "the call returned %d: %s\n", rc, psxhip_last_error());
            return 6;
        }
        for (const Block* k : {&units, &states, &err})
            if (k->all && k->size && fwrite(k->all + k->offset, 1, k->size, out) != k->size) return 5;
        for (Block* k : {&chains, &base, &states, &samples, &units, &err}) {
            if (k->all && !k->front_kept()) return 7;
            free(k->all);
        }
    }
    psxhip_adpcm_release_blocks();
    fclose(in);
    return fclose(out) ? 5 : 0;
}
