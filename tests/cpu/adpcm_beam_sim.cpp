// adpcm_beam_sim.cpp -- psxavenc_amd/csrc/adpcm_beam_core.h on the CPU (built with -fsanitize=address,undefined by
// tests/test_adpcm_beam_core_cpu.py): the step, the pool's selection, the trace back and the record's words that the kernels compile,
// unit after unit along a chain.
//
// usage: adpcm_beam_sim IN OUT.  IN is a sequence of cases: int32 {bits, filter_count, beam, n_units, p1, p2} + 28 n_units int16
// samples.  OUT per case and unit: the record (16 or 32 bytes), uint32 e, int32 p1, p2 behind the unit.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../psxavenc_amd/csrc/adpcm_beam_core.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t head[6];
    while (fread(head, sizeof head, 1, in) == 1) {
        const int bits = head[0], filter_count = head[1], beam = head[2], n_units = head[3];
        if ((bits != 4 && bits != 8) || (filter_count != 4 && filter_count != 5) || beam < 1 || beam > PSXHIP_ADPCM_BEAM_MAX || n_units < 0) return 3;
        std::vector<int16_t> pcm((size_t)n_units * 28);     // (ends with the last sample: a read past it is the sanitizer's)
        if (!pcm.empty() && fread(pcm.data(), 2, pcm.size(), in) != pcm.size()) return 4;
        int p1 = head[4], p2 = head[5];
        for (int u = 0; u < n_units; u++) {
            std::vector<int> xs(28);
            for (int i = 0; i < 28; i++) xs[(size_t)i] = pcm[(size_t)u * 28 + (size_t)i];
            const BeamUnit r = beam_encode_unit(xs.data(), p1, p2, filter_count, bits == 4 ? 12 : 8, beam);
            p1 = r.p1;
            p2 = r.p2;
            const int32_t st[2] = {p1, p2};
            if (fwrite(r.rec, 1, bits == 4 ? 16 : 32, out) != (size_t)(bits == 4 ? 16 : 32) || fwrite(&r.e, 4, 1, out) != 1 || fwrite(st, 4, 2, out) != 2) return 5;
        }
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
