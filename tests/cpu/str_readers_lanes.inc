// tests/cpu/str_readers_lanes.inc -- TEST INFRASTRUCTURE: the body of tests/cpu/str_demux_lanes.cpp and
// tests/cpu/strspu_demux_lanes.cpp.  The two readers share their host file (psxavenc_amd/csrc/psxhip_str_demux.cpp), and the STRSPU
// reader runs the STR reader's kernels as its video half, so both programs hold the text of both kernel files and of the host file
// and differ in name only; a record's format says which entry point it calls: psxhip_str_demux_device (formats 6, 7, 9) or
// psxhip_strspu_demux_device (format 8).  Those are the calls that build the job and lay the workspace out.  The modules' _host
// entry points (psxhip_str_read_host, psxhip_strspu_read_host) are not called: they put these calls between the BS decoder, the XA
// disassembler (sector_kernels.hip, an encoder-side file) and the ADPCM decoder, which this program gives as stand-ins that fail.
//
//   <program> <in> <out> <order: 0 ascending, 1 descending, 2 shuffled> [seed]
// in:  records of 32 int32: the 16 words of psxhip_str_settings_t, then {n_streams, n_sectors, first_frame, max_frames, bs_stride,
//      capacity (XA sectors / audio chunks), has_table, in_pad, bs_pad, out_pad, fill, in_offset, 0...}; then n_streams x n_sectors
//      sectors
// out: per record, each from a block of its own that held `fill`: the rows ((S - 1) x bs_stream_stride + max_frames x bs_stride),
//      the sizes, the frame records, the XA sectors or unit records ((S - 1) x stride + capacity x sector size or x 126 x 16), the chunk
//      records (format 8), the table when has_table, the summaries, the audio summaries (format 8)
// Stream strides are a stream's size plus the pad.  The sectors are one heap block that ends with the last stream's last sector,
// in_offset bytes (a multiple of 4) into its allocation; every output starts 4 bytes into its allocation (the unit records: 16),
// which is the alignment include/psxav_hip.h promises and no more, and the bytes in front must keep `fill`.
#define HIP_LANES_WAVES 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip_lanes/psxhip_api_standin.h"

#include "../../psxavenc_amd/csrc/str_demux_kernels.hip"
#include "../../psxavenc_amd/csrc/strspu_demux_kernels.hip"
#include "../../psxavenc_amd/csrc/psxhip_str_demux.cpp"
#include "../../psxavenc_amd/csrc/reader_plan.cpp"
#include "../../psxavenc_amd/csrc/str_plan.cpp"

// stand-ins for what the _host entry points compose the readers with; never reached from this program
extern "C" int psxhip_mdec_decoder_create(psxhip_mdec_decoder_t**, int, int, int, int) { return PSXHIP_EDEVICE; }
extern "C" void psxhip_mdec_decoder_destroy(psxhip_mdec_decoder_t*) {}
extern "C" int psxhip_mdec_decode_frames_device(psxhip_mdec_decoder_t*, const uint8_t*, size_t, const int32_t*, int, int, int16_t*, uint8_t*, size_t,
                                                psxhip_mdec_decoded_t*, void*) { return PSXHIP_EDEVICE; }
extern "C" int psxhip_adpcm_decode_chains_chunked(int, const uint8_t*, const psxhip_adpcm_chain_t*, const int32_t*, int, int, int,
                                                  psxhip_adpcm_state_t*, int16_t*, uint8_t*, int16_t*, int, int, int, void*) { return PSXHIP_EDEVICE; }
extern "C" int psxhip_xa_disassemble_device(int, const uint8_t*, int, int, int, int, int, uint8_t*, int32_t*, void*) { return PSXHIP_EDEVICE; }

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
    int32_t head[32];
    static_assert(sizeof(psxhip_str_settings_t) == 16 * sizeof(int32_t), "the record holds the settings as 16 words");
    while (fread(head, sizeof head, 1, in) == 1) {
        // a reader of its own for every record: its workspace is a block of exactly the size the host layer works out for this call
        psxhip_str_reader_t* reader = nullptr;
        if (psxhip_str_reader_create(&reader, 0) != PSXHIP_OK) return 6;
        psxhip_str_settings_t s;
        memcpy(&s, head, sizeof s);
        const int S = head[16], n = head[17], first_frame = head[18], mf = head[19], cap = head[21], has_table = head[22], fill = head[26];
        const size_t bs_stride = (size_t)head[20], in_pad = (size_t)head[23], bs_pad = (size_t)head[24], out_pad = (size_t)head[25],
                     in_offset = (size_t)head[27];
        const bool spu = s.format == 8;
        int ssz = 2048, sub_at, hdr_at;
        if (!spu && !str_sector_geometry(s.format, &ssz, &sub_at, &hdr_at)) return 3;
        if (S < 1 || S > 16 || n < 0 || mf < 0 || cap < 0 || (in_offset & 3)) return 3;
        const size_t in_stride = (size_t)n * ssz + in_pad, bs_stream = (size_t)mf * bs_stride + bs_pad;
        const size_t out_unit = spu ? (size_t)126 * 16 : (size_t)ssz, out_stream = (size_t)cap * out_unit + out_pad;
        Block src;
        uint8_t* sectors = src.make(in_offset, (size_t)(S - 1) * in_stride + (size_t)n * ssz, fill);
        for (int i = 0; i < S; i++)
            if (n && fread(sectors + (size_t)i * in_stride, (size_t)ssz, (size_t)n, in) != (size_t)n) return 4;
        std::vector<Block> b(8);
        uint8_t* bs = mf ? b[0].make(4, (size_t)(S - 1) * bs_stream + (size_t)mf * bs_stride, fill) : nullptr;
        auto* sizes = mf ? (int32_t*)b[1].make(4, (size_t)S * mf * 4, fill) : nullptr;
        auto* info = mf ? (psxhip_str_frame_info_t*)b[2].make(4, (size_t)S * mf * sizeof(psxhip_str_frame_info_t), fill) : nullptr;
        uint8_t* audio = cap ? b[3].make(spu ? 16 : 4, (size_t)(S - 1) * out_stream + (size_t)cap * out_unit, fill) : nullptr;
        auto* cinfo = spu && cap ? (psxhip_strspu_chunk_info_t*)b[4].make(4, (size_t)S * cap * sizeof(psxhip_strspu_chunk_info_t), fill) : nullptr;
        auto* table = has_table ? (psxhip_str_sector_t*)b[5].make(4, (size_t)S * n * sizeof(psxhip_str_sector_t), fill) : nullptr;
        auto* summary = (psxhip_str_summary_t*)b[6].make(4, (size_t)S * sizeof(psxhip_str_summary_t), fill);
        auto* asum = spu ? (psxhip_strspu_audio_summary_t*)b[7].make(4, (size_t)S * sizeof(psxhip_strspu_audio_summary_t), fill) : nullptr;
        const int rc = spu ? psxhip_strspu_demux_device(reader, &s, S, n ? sectors : nullptr, in_stride, n, first_frame, mf, bs, bs_stride, bs_stream,
                                                        sizes, info, audio, cap, out_stream, cinfo, table, summary, asum, nullptr)
                           : psxhip_str_demux_device(reader, &s, S, n ? sectors : nullptr, in_stride, n, first_frame, mf, bs, bs_stride, bs_stream, sizes,
                                                     info, audio, cap, out_stream, table, summary, nullptr);
        if (rc != PSXHIP_OK) {
            fprintf(stderr, "the call returned %d: %s\n", rc, psxhip_last_error());
            return 6;
        }
        for (const Block& k : b) {
            if (!k.all) continue;
            if (!k.front_kept()) return 7;
            if (k.size && fwrite(k.all + k.offset, 1, k.size, out) != k.size) return 5;
            free(k.all);
        }
        if (!src.front_kept()) return 7;
        free(src.all);
        psxhip_str_reader_destroy(reader);
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
