// tests/cpu/disc_read_lanes.cpp -- TEST INFRASTRUCTURE: runs the text of psxavenc_amd/csrc/disc_read_kernels.hip and of its host
// layer psxavenc_amd/csrc/psxhip_disc_read.cpp on the CPU under -fsanitize=address,undefined (tests/test_disc_read_lanes_cpu.py),
// behind the wavefront model of the stand-in tests/cpu/hip_lanes.  A record is one call of psxhip_disc_read_host (mode 0: the host
// layer stages everything in one block of its own layout) or of psxhip_disc_read_device (mode 1: the program's own blocks).  A
// program, not a library.
//
//   disc_read_lanes <in> <out> <order: 0 ascending, 1 descending, 2 shuffled> [seed]
// in:  records of int32 {mode, n_sectors, n_tracks, has_table, fill}, n_tracks x int32 {sector_size, capacity, file, channel, mask,
//      value, stride}, then n_sectors x 2352 bytes
// out: per record every track's buffer, (capacity - 1) * stride + sector_size bytes that held `fill` before; the table
//      (n_sectors x 16 bytes) when has_table; the counts (n_tracks x 4); the summary (64 bytes)
// The image is a heap block of exactly n_sectors x 2352 bytes.  Every output is a block of its own that ends with the last byte
// include/psxav_hip.h lets the call touch, some bytes into its allocation -- 4 for the device call (it is promised 4-byte alignment
// and no more; 8 for the summary, which is promised 8), 1 for the host call (no alignment rule) -- and the bytes in front must keep
// `fill`.
#define HIP_LANES_WAVES 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip_lanes/psxhip_api_standin.h"

#include "../../psxavenc_amd/csrc/disc_read_kernels.hip"
#include "../../psxavenc_amd/csrc/psxhip_disc_read.cpp"

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
    int32_t head[5];
    while (fread(head, sizeof head, 1, in) == 1) {
        // a reader of its own for every record: its workspace is a block of exactly the size the host layer works out for this call
        psxhip_disc_reader_t* reader = nullptr;
        if (psxhip_disc_reader_create(&reader, 0) != PSXHIP_OK) return 6;
        const int mode = head[0], n = head[1], nt = head[2], has_table = head[3], fill = head[4];
        if (n < 0 || nt < 0 || nt > PSXHIP_DISC_MAX_SOURCES || (mode != 0 && mode != 1)) return 3;
        const size_t off = mode ? 4 : 1;
        psxhip_disc_track_t tracks[PSXHIP_DISC_MAX_SOURCES];
        std::vector<Block> blocks((size_t)nt + 3);
        memset(tracks, 0, sizeof tracks);
        for (int t = 0; t < nt; t++) {
            int32_t v[7];
            if (fread(v, sizeof v, 1, in) != 1) return 4;
            psxhip_disc_track_t& T = tracks[t];
            T.sector_size = v[0]; T.capacity = v[1]; T.file_number = v[2]; T.channel_number = v[3];
            T.submode_mask = (uint8_t)v[4]; T.submode_value = (uint8_t)v[5]; T.stride = v[6];
            if (T.capacity < 0 || T.stride < T.sector_size || T.sector_size < 2048) return 3;
            T.sectors = T.capacity ? blocks[t].make(off, (size_t)(T.capacity - 1) * (size_t)T.stride + (size_t)T.sector_size, fill) : nullptr;
        }
        uint8_t* image = (uint8_t*)malloc((size_t)n * 2352);
        if (n && (!image || fread(image, 2352, (size_t)n, in) != (size_t)n)) return 4;
        auto* table = has_table ? (psxhip_disc_read_sector_t*)blocks[nt].make(off, (size_t)n * sizeof(psxhip_disc_read_sector_t), fill) : nullptr;
        auto* counts = (int32_t*)blocks[nt + 1].make(off, (size_t)nt * 4, fill);
        auto* summary = (psxhip_disc_read_summary_t*)blocks[nt + 2].make(mode ? 8 : 1, sizeof(psxhip_disc_read_summary_t), fill);
        const int rc = mode ? psxhip_disc_read_device(reader, image, n, tracks, nt, table, nt ? counts : nullptr, summary, nullptr)
                            : psxhip_disc_read_host(reader, image, n, tracks, nt, table, nt ? counts : nullptr, summary);
        if (rc != PSXHIP_OK) {
            fprintf(stderr, "the call returned %d: %s\n", rc, psxhip_last_error());
            return 6;
        }
        for (const Block& b : blocks) {
            if (!b.all) continue;
            if (!b.front_kept()) return 7;
            if (b.size && fwrite(b.all + b.offset, 1, b.size, out) != b.size) return 5;
            free(b.all);
        }
        free(image);
        psxhip_disc_reader_destroy(reader);
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
