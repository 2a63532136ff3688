// tests/cpu/mdec_decode_lanes.cpp -- TEST INFRASTRUCTURE: runs the text of psxavenc_amd/csrc/mdec_decode_kernels.hip and of its
// host layer psxavenc_amd/csrc/psxhip_decode.cpp on the CPU under -fsanitize=address,undefined
// (tests/test_mdec_decode_lanes_cpu.py), behind the wavefront model of the stand-in tests/cpu/hip_lanes.  A record is one call of
// psxhip_mdec_decode_frames_device (kind 0: the program's own blocks), psxhip_mdec_decode_frames_host (kind 1: the host layer's
// staging and its re-striding of rows) or psxhip_mdec_sse_device (kind 2).  The display back-end, which psxhip_decode.cpp can chain
// behind the decoder, is a stand-in that fails.  A program, not a library.
//
//   mdec_decode_lanes <in> <out> <order: 0 ascending, 1 descending, 2 shuffled> [seed]
// in:  records of 16 int32 {kind, width, height, dc_wrap, n_frames, bs_stride | frame_stride, has_sizes, uniform_size, want_levels,
//      want_frames, frame_pad, fill, 0...}; kind 0 / 1: n_frames int32 sizes when has_sizes, then n_frames rows of bs_stride bytes;
//      kind 2: n_frames frames of width x height x 3 / 2 bytes, twice
// out: kind 0 / 1: n_frames x psxhip_mdec_decoded_t, the levels when want_levels, the frames ((n_frames - 1) x frame_stride + frame
//      bytes that held `fill`) when want_frames; kind 2: n_frames x 3 uint64
// Device call: the bitstream block ends with the last byte of the LAST frame's size (a size above bs_stride counts as bs_stride) --
// single-frame records make that every frame's --, 4 bytes into its allocation; levels 2 bytes in, frames and records 4, the sums 8.
// Host call: rows of bs_stride bytes, everything 1 byte into its allocation (no alignment rule).
#define HIP_LANES_WAVES 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip_lanes/psxhip_api_standin.h"

#include "../../psxavenc_amd/csrc/mdec_decode_kernels.hip"
#include "../../psxavenc_amd/csrc/psxhip_decode.cpp"

// stand-ins for the display back-end behind psxhip_mdec_decode_display_device; never reached from this program
int psxhip_display_check(const char*, const psxhip_display_job_t*, bool) { return PSXHIP_EDEVICE; }
extern "C" hipError_t psxhip_display_launch(const psxhip_display_job_t*, void*) { return hipErrorInvalidValue; }

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
    int32_t head[16];
    while (fread(head, sizeof head, 1, in) == 1) {
        const int kind = head[0], w = head[1], h = head[2], wrap = head[3], n = head[4], has_sizes = head[6], uniform = head[7],
                  want_levels = head[8], want_frames = head[9], fill = head[11];
        const size_t stride = (size_t)head[5], fb = (size_t)w * h * 3 / 2, frame_stride = fb + (size_t)head[10];
        if (kind < 0 || kind > 2 || n < 1 || n > 4096) return 3;
        Block bs, sizes_b, decoded, levels, frames, a, b, sse;
        int rc;
        std::vector<Block*> written;
        if (kind < 2) {
            // a decoder of its own for every record: its workspace and staging blocks are exactly this call's
            psxhip_mdec_decoder_t* dec = nullptr;
            if (psxhip_mdec_decoder_create(&dec, 0, w, h, wrap) != PSXHIP_OK) return 6;
            const size_t nblk = (size_t)(w / 16) * (h / 16) * 6, off = kind ? 1 : 4;
            std::vector<int32_t> sz((size_t)n);
            if (has_sizes && fread(sz.data(), 4, (size_t)n, in) != (size_t)n) return 4;
            std::vector<uint8_t> rows((size_t)n * stride);
            if (fread(rows.data(), 1, rows.size(), in) != rows.size()) return 4;
            int64_t last = has_sizes ? sz[(size_t)n - 1] : uniform;
            last = last < 0 ? 0 : (last > (int64_t)stride ? (int64_t)stride : last);
            const size_t bs_bytes = kind ? (size_t)n * stride : (size_t)(n - 1) * stride + (size_t)last;
            uint8_t* p_bs = bs.make(off, bs_bytes, fill);
            memcpy(p_bs, rows.data(), bs_bytes);
            auto* p_dec = (psxhip_mdec_decoded_t*)decoded.make(off, (size_t)n * sizeof(psxhip_mdec_decoded_t), fill);
            auto* p_lv = want_levels ? (int16_t*)levels.make(kind ? 1 : 2, (size_t)n * nblk * 128, fill) : nullptr;
            uint8_t* p_fr = want_frames ? frames.make(off, kind ? (size_t)n * fb : (size_t)(n - 1) * frame_stride + fb, fill) : nullptr;
            if (kind == 0) {
                int32_t* p_sz = has_sizes ? (int32_t*)sizes_b.make(4, (size_t)n * 4, fill) : nullptr;
                if (p_sz) memcpy(p_sz, sz.data(), (size_t)n * 4);
                rc = psxhip_mdec_decode_frames_device(dec, p_bs, stride, p_sz, uniform, n, p_lv, p_fr, frame_stride, p_dec, nullptr);
            } else {
                int32_t* p_sz = has_sizes ? (int32_t*)sizes_b.make(1, (size_t)n * 4, fill) : nullptr;
                if (p_sz) memcpy(p_sz, sz.data(), (size_t)n * 4);
                rc = psxhip_mdec_decode_frames_host(dec, p_bs, stride, p_sz, uniform, n, p_lv, p_fr, p_dec);
            }
            psxhip_mdec_decoder_destroy(dec);
            written = {&decoded, &levels, &frames};
        } else {
            const size_t bytes = (size_t)(n - 1) * stride + fb;
            uint8_t* pa = a.make(4, bytes, fill);
            uint8_t* pb = b.make(4, bytes, fill);
            for (uint8_t* p : {pa, pb})
                for (int i = 0; i < n; i++)
                    if (fread(p + (size_t)i * stride, 1, fb, in) != fb) return 4;
            auto* p_sse = (uint64_t*)sse.make(8, (size_t)n * 24, fill);
            rc = psxhip_mdec_sse_device(0, pa, pb, stride, w, h, n, p_sse, nullptr);
            written = {&sse};
        }
        if (rc != PSXHIP_OK) {
            fprintf(stderr, "the call returned %d: %s\n", rc, psxhip_last_error());
            return 6;
        }
        for (Block* k : written)
            if (k->all && k->size && fwrite(k->all + k->offset, 1, k->size, out) != k->size) return 5;
        for (Block* k : {&bs, &sizes_b, &decoded, &levels, &frames, &a, &b, &sse}) {
            if (k->all && !k->front_kept()) return 7;
            free(k->all);
        }
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
