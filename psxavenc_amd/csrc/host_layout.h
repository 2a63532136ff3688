// host_layout.h -- the layouts the host layer derives from a format: what an XA sector holds, where an STR sector keeps its
// subheader and chunk header, which chain of a stream reads which samples and writes which unit records, and how a workspace is
// carved.  Arithmetic only (no HIP): a host compiler builds it alone.  The kernels keep their own copies of these constants.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/psxav_hip.h"

struct XaLayout {
    int channels;
    int units_per_group;        // 28-sample sound units per 128-byte sound group
    int units_per_sector;       // 18 groups
    int sector_bytes;
    int samples_per_sector;     // int16, all channels together
    int record_bytes;           // between the unit records of the ADPCM kernels
};

// format 0: 2336-byte XA sectors, 1: 2352-byte XACD sectors; bits 4 or 8
static inline XaLayout xa_layout(int format, int stereo, int bits) {
    XaLayout x;
    x.channels = stereo ? 2 : 1;
    x.units_per_group = bits == 4 ? 8 : 4;
    x.units_per_sector = 18 * x.units_per_group;
    x.sector_bytes = format == 0 ? 2336 : 2352;
    x.samples_per_sector = x.units_per_sector * 28;
    x.record_bytes = PSXHIP_ADPCM_RECORD_SIZE(bits);
    return x;
}

// sectors from one sector of an XA channel to its next at 1x speed (filefmt.c:399-403): 2 stereo, 4 mono; x 2 at 18900 Hz, x 2 at 4 bits
static inline int xa_sector_interleave(int stereo, int frequency, int bits) {
    return (stereo ? 2 : 4) * (frequency == 18900 ? 2 : 1) * (bits == 4 ? 2 : 1);
}

// format 6 (STR), 7 (STRCD), 9 (STRV): bytes per sector, where the XA subheader lies (-1: none) and the chunk header (mdec.c:822-829)
static inline bool str_sector_geometry(int format, int* sector_size, int* sub_at, int* hdr_at) {
    switch (format) {
    case 6: *sector_size = 2336; *sub_at = 0; *hdr_at = 0x08; return true;
    case 7: *sector_size = 2352; *sub_at = 0x10; *hdr_at = 0x18; return true;
    case 9: *sector_size = 2048; *sub_at = -1; *hdr_at = 0x00; return true;
    }
    return false;
}

// format 8 (STRSPU, "psxhip STRSPU v1"): 2048-byte sectors; an audio sector holds 126 SPU blocks behind a
// 32-byte chunk header, shared by the channels in lanes of L bytes.  Audio sectors are a share p / q < 1 of the stream:
// audio_frequency / (samples per channel per sector x 75 sectors a second x CD speed), reduced.
struct StrspuLayout {
    int channels;
    int blocks;                 // B: SPU blocks per channel per audio sector
    int lane_bytes;             // L = 16 B
    int samples_per_sector;     // spc = 28 B, per channel
    int64_t p, q;               // the audio share of the sectors; p >= q: the rate does not fit the CD speed
};

// channels 1 or 2, frequency > 0, cd_speed 1 or 2 (the caller's checks)
static inline StrspuLayout strspu_layout(int channels, int frequency, int cd_speed) {
    StrspuLayout x;
    x.channels = channels;
    x.blocks = 126 / channels;
    x.lane_bytes = 16 * x.blocks;
    x.samples_per_sector = 28 * x.blocks;
    int64_t a = frequency, b = (int64_t)x.samples_per_sector * 75 * cd_speed;
    x.p = a;
    x.q = b;
    while (b) { const int64_t t = a % b; a = b; b = t; }
    x.p /= a;
    x.q /= a;
    return x;
}

// a(n): audio sectors among the first n sectors -- leading audio never falls behind (ceil), trailing audio never runs ahead (floor).
// Sector n is an audio sector iff a(n + 1) > a(n).  n < 2^31 and p < q <= 2 x 28 x 126 x 75: the product stays far inside 64 bits.
static inline int64_t strspu_audio_before(const StrspuLayout& x, bool trailing, int64_t n) {
    return trailing ? n * x.p / x.q : (n * x.p + x.q - 1) / x.q;
}

// n_streams planar streams, one chain each: stream i reads from sample i * stream_stride on, its records follow stream i - 1's
static inline void fill_planar_chains(psxhip_adpcm_chain_t* chains, int32_t* unit_base, int n_streams, int64_t stream_stride, int pitch,
                                      int sample_limit, int n_units) {
    for (int i = 0; i < n_streams; i++) {
        chains[i].sample_offset = (int64_t)i * stream_stride;
        chains[i].pitch = pitch;
        chains[i].sample_limit = sample_limit;
        chains[i].n_units = n_units;
        chains[i].unit_stride = 1;
        unit_base[i] = i * n_units;
    }
}

// n_streams streams of `channels` interleaved channels, one chain per channel (chain i * channels + c): the channels' records
// interleave into encode order within the stream's units_per_stream records
static inline void fill_interleaved_chains(psxhip_adpcm_chain_t* chains, int32_t* unit_base, int n_streams, int channels, int64_t stream_stride,
                                           int sample_limit, int units_per_stream) {
    for (int i = 0; i < n_streams; i++)
        for (int c = 0; c < channels; c++) {
            psxhip_adpcm_chain_t& d = chains[(size_t)i * channels + c];
            d.sample_offset = (int64_t)i * stream_stride + c;
            d.pitch = channels;
            d.sample_limit = sample_limit;
            d.n_units = units_per_stream / channels;
            d.unit_stride = channels;
            unit_base[(size_t)i * channels + c] = i * units_per_stream + c;
        }
}

// the alignment every device pointer of the readers' entry points needs at the least: 4 bytes
static inline bool misaligned(uintptr_t p) { return (p & 3) != 0; }
static inline bool misaligned(const void* p) { return misaligned((uintptr_t)p); }

// carves one allocation into 256-byte aligned parts: take() returns the part's offset, `end` is the size so far
struct BumpOffsets {
    size_t end = 0;
    size_t take(size_t bytes) {
        const size_t at = end;
        end += (bytes + 255) & ~(size_t)255;
        return at;
    }
};
