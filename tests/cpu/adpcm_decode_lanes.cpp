// tests/cpu/adpcm_decode_lanes.cpp -- TEST INFRASTRUCTURE: runs the text of psxavenc_amd/csrc/adpcm_decode_kernels.hip and of its
// host layer psxavenc_amd/csrc/psxhip_adpcm_decode.cpp (with its plans, adpcm_plan.cpp) on the CPU under -fsanitize=address,undefined
// (tests/test_adpcm_decode_lanes_cpu.py), behind the wavefront model of the stand-in tests/cpu/hip_lanes.  A record is one call of
// psxhip_adpcm_decode_chains_device (kind 0), psxhip_adpcm_decode_chains_chunked (kind 1: the host layer's chunk tables, workspace
// and verify passes) or psxhip_adpcm_sse_device (kind 2).  The host-buffer conveniences of that file decode through the same two
// calls behind the XA disassembler (sector_kernels.hip, an encoder-side file), which this program gives as a stand-in that fails.
// A program, not a library.
//
//   adpcm_decode_lanes <in> <out> <order: 0 ascending, 1 descending, 2 shuffled> [seed]
// in:  records of 16 int32 {kind, bits, filter_count, n_chains, n_records, total_samples, has_flags | has_unit_sse, has_tail,
//      chunk_units, warmup_units, max_passes, fill, has_chain_sums, 0, 0, 0}; n_chains x psxhip_adpcm_chain_t; n_chains x int32
//      unit_base; then kind 0 / 1: n_chains x psxhip_adpcm_state_t, n_records records; kind 2: total_samples int16 a, as many b,
//      n_chains x 28 int16 a_tail when has_tail
// out: kind 0 / 1: the samples (total_samples int16 that held `fill`), the states, the flags (n_records bytes) when has_flags, the
//      tail (n_chains x 28 int16) when has_tail, kind 1: the call's return value (int32, the verify passes); kind 2: unit_sse
//      (n_records uint64) when has_unit_sse, chain_sums (n_chains x 2 uint64) when has_chain_sums
// Every buffer is a heap block of its own that ends with the last element include/psxav_hip.h lets the call touch, and starts
// behind an offset that keeps only the promised alignment: samples 2 bytes, flags 1, tail 4, the sums 8; the records 16.
#define HIP_LANES_WAVES 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip_lanes/psxhip_api_standin.h"

#include "../../psxavenc_amd/csrc/adpcm_decode_kernels.hip"
#include "../../psxavenc_amd/csrc/adpcm_plan.cpp"
#include "../../psxavenc_amd/csrc/psxhip_adpcm_decode.cpp"

// stand-ins for the device-facing wrappers psxhip_adpcm_decode.cpp takes from the encoder side (its plans are adpcm_plan.cpp's own text)
int psxhip_adpcm_device_cus(int) { return 4; }
extern "C" int psxhip_sector_tables(int) { return PSXHIP_EDEVICE; }
extern "C" hipError_t psxhip_xa_disassemble_launch(const psxhip_xa_dis_job_t*, void*) { return hipErrorInvalidValue; }

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
        const int kind = head[0], bits = head[1], filter_count = head[2], nc = head[3], n_records = head[4], total = head[5], has_flags = head[6],
                  has_tail = head[7], chunk_units = head[8], warmup_units = head[9], max_passes = head[10], fill = head[11], has_sums = head[12];
        if (kind < 0 || kind > 2 || nc < 0 || n_records < 0 || total < 0 || (bits != 4 && bits != 8)) return 3;
        Block chains, base, states, units, samples, flags, tail, a, b, unit_sse, sums;
        auto* d_chains = (psxhip_adpcm_chain_t*)chains.make(0, (size_t)nc * sizeof(psxhip_adpcm_chain_t), fill);
        auto* d_base = (int32_t*)base.make(0, (size_t)nc * 4, fill);
        if (!chains.load(in) || !base.load(in)) return 4;
        int rc;
        std::vector<const Block*> written;
        if (kind < 2) {
            auto* d_states = (psxhip_adpcm_state_t*)states.make(0, (size_t)nc * sizeof(psxhip_adpcm_state_t), fill);
            auto* d_units = units.make(0, (size_t)n_records * (bits == 4 ? 16 : 32), fill);
            if (!states.load(in) || !units.load(in)) return 4;
            auto* d_samples = (int16_t*)samples.make(2, (size_t)total * 2, fill);
            uint8_t* d_flags = has_flags ? flags.make(1, (size_t)n_records, fill) : nullptr;
            auto* d_tail = has_tail ? (int16_t*)tail.make(4, (size_t)nc * 56, fill) : nullptr;
            rc = kind == 0 ? psxhip_adpcm_decode_chains_device(0, d_units, d_chains, d_base, nc, filter_count, bits, d_states, d_samples, d_flags, d_tail,
                                                               nullptr)
                           : psxhip_adpcm_decode_chains_chunked(0, d_units, d_chains, d_base, nc, filter_count, bits, d_states, d_samples, d_flags,
                                                                d_tail, chunk_units, warmup_units, max_passes, nullptr);
            written = {&samples, &states, &flags, &tail};
        } else {
            auto* d_a = (int16_t*)a.make(2, (size_t)total * 2, fill);
            auto* d_b = (int16_t*)b.make(2, (size_t)total * 2, fill);
            if (!a.load(in) || !b.load(in)) return 4;
            auto* d_tail = has_tail ? (int16_t*)tail.make(2, (size_t)nc * 56, fill) : nullptr;
            if (has_tail && !tail.load(in)) return 4;
            auto* d_unit = has_flags ? (uint64_t*)unit_sse.make(8, (size_t)n_records * 8, fill) : nullptr;
            auto* d_sums = has_sums ? (uint64_t*)sums.make(8, (size_t)nc * 16, fill) : nullptr;
            rc = psxhip_adpcm_sse_device(0, d_a, d_tail, d_b, d_chains, nc, d_unit, d_base, d_sums, nullptr);
            written = {&unit_sse, &sums};
        }
        if (rc < 0) {
            fprintf(stderr, "the call returned %d: %s\n", rc, psxhip_last_error());
            return 6;
        }
        for (const Block* k : written)
            if (k->all && k->size && fwrite(k->all + k->offset, 1, k->size, out) != k->size) return 5;
        if (kind == 1) {
            const int32_t passes = rc;
            if (fwrite(&passes, 4, 1, out) != 1) return 5;
        }
        for (Block* k : {&chains, &base, &states, &units, &samples, &flags, &tail, &a, &b, &unit_sse, &sums}) {
            if (k->all && !k->front_kept()) return 7;
            free(k->all);
        }
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
