// spu_file_layout.h -- the framing of a mono SPU / VAG file, stated once: what psxavenc's encode_file_spu (psxavenc/filefmt.c:212-293)
// and its .vag header writer (:95-162) put around the blocks of psx_audio_spu_encode.  Both callers read it from here: the one-file
// entry points (psxhip_spufile.cpp) and the sound bank's plan (spu_bank_plan.cpp).  Arithmetic only (no HIP): a host compiler
// builds it alone.
//
// A file is: a 48-byte header (VAG), a leading zero block unless no_leading_dummy, ceil(samples / 28) data blocks, a trap block
// unless enable_loop, zero padding of that body to `alignment`.  LOOP_START goes into byte 1 of the data block the loop point falls
// into, LOOP_REPEAT into byte 1 of the last data block when enable_loop is set.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/psxav_audio.h"
#include "../../include/psxav_hip.h"
#include "../../include/psxav_mdec.h"

constexpr int kSpuBlockBytes = PSX_AUDIO_SPU_BLOCK_SIZE;             // 16
constexpr int kSpuBlockSamples = PSX_AUDIO_SPU_SAMPLES_PER_BLOCK;    // 28
constexpr int kVagHeaderBytes = 0x30;                                // filefmt.c:93

static inline void put_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// write_vag_header, filefmt.c:95-162
static inline void vag_header(const psxhip_spu_file_settings_t* s, int size_per_channel, uint8_t* h) {
    memset(h, 0, kVagHeaderBytes);
    h[0] = 'V'; h[1] = 'A'; h[2] = 'G';
    h[3] = s->format == FORMAT_VAGI ? 'i' : 'p';
    put_be32(h + 0x04, 0x20);                                     // version
    if (s->format == FORMAT_VAGI) {                               // interleave, little endian
        h[0x08] = (uint8_t)s->audio_interleave;
        h[0x09] = (uint8_t)(s->audio_interleave >> 8);
        h[0x0A] = (uint8_t)(s->audio_interleave >> 16);
        h[0x0B] = (uint8_t)(s->audio_interleave >> 24);
    }
    put_be32(h + 0x0C, (uint32_t)size_per_channel);
    put_be32(h + 0x10, (uint32_t)s->audio_frequency);
    if (s->format == FORMAT_VAGI && s->audio_loop_point >= 0) {   // loop point in bytes (non-standard)
        int loop_start_block = (s->audio_loop_point * s->audio_frequency) / (kSpuBlockSamples * 1000);
        if (!s->no_leading_dummy) loop_start_block++;
        put_be32(h + 0x14, (uint32_t)(loop_start_block * kSpuBlockBytes));
    }
    h[0x1E] = (uint8_t)s->audio_channels;
    strncpy((char*)(h + 0x20), s->name, 16);
}

// spu / vag: the file's bytes for n samples; *data_blocks the encoder's blocks, *block_count the body's blocks (the header's
// size_per_channel is block_count x 16: the unpadded body)
static inline int64_t spu_layout(const psxhip_spu_file_settings_t* s, int64_t n, int64_t* data_blocks, int64_t* block_count) {
    const int64_t blocks = (n + kSpuBlockSamples - 1) / kSpuBlockSamples;
    int64_t count = (s->no_leading_dummy ? 0 : 1) + blocks + (s->enable_loop ? 0 : 1);
    *data_blocks = blocks;
    *block_count = count;
    int64_t bytes = count * kSpuBlockBytes;
    const int64_t overflow = bytes % s->alignment;
    if (overflow) bytes += s->alignment - overflow;
    // the reference seeks past the header, writes the data, then seeks back (filefmt.c:218-219,287-292)
    return (s->format == FORMAT_VAG ? kVagHeaderBytes : 0) + bytes;
}

// the data block (0 = the first behind the dummy) that takes LOOP_START, or -1: no loop point, or one behind the last data block
// (filefmt.c:234-235,251-252)
static inline int64_t spu_loop_start_data_block(const psxhip_spu_file_settings_t* s, int64_t data_blocks) {
    if (s->audio_loop_point < 0) return -1;
    const int64_t b = ((int64_t)s->audio_loop_point * s->audio_frequency) / (kSpuBlockSamples * 1000);
    return b < data_blocks ? b : -1;
}
