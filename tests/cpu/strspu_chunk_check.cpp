// strspu_chunk_check.cpp -- runs psxavenc_amd/csrc/strspu_chunk.h, the header reading the STRSPU reader's kernels compile, over a file
// of cases for tests/test_strspu_chunk_cpu.py to compare with tests/strspu_demux_ref.py.  Built with the host sanitizers.
// A case: int32 ch, id, d, loop, frequency; int64 k; the 32 header bytes.  A result: int32 audio, flags, mismatch; int64 number.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../psxavenc_amd/csrc/strspu_chunk.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<uint8_t> rec(5 * 4 + 8 + 32);
    while (fread(rec.data(), 1, rec.size(), in) == rec.size()) {
        int32_t p[5];
        int64_t k;
        uint8_t bytes[32];
        memcpy(p, rec.data(), sizeof p);
        memcpy(&k, rec.data() + 20, 8);
        memcpy(bytes, rec.data() + 28, 32);
        uint32_t h[8];
        for (int i = 0; i < 8; i++)
            h[i] = (uint32_t)bytes[4 * i] | (uint32_t)bytes[4 * i + 1] << 8 | (uint32_t)bytes[4 * i + 2] << 16 | (uint32_t)bytes[4 * i + 3] << 24;
        const StrspuChunkRules r = {p[0], (uint32_t)p[1], p[2], p[3], (uint32_t)p[4]};
        const int32_t res[3] = {strspu_is_audio(h, r) ? 1 : 0, (int32_t)strspu_chunk_flags(h), strspu_chunk_mismatch(h, k, r) ? 1 : 0};
        const int64_t number = strspu_chunk_number(h);
        fwrite(res, sizeof res, 1, out);
        fwrite(&number, sizeof number, 1, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
