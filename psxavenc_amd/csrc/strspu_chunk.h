// strspu_chunk.h -- how the STRSPU reader reads the 32-byte header of an audio chunk ("psxhip STRSPU demux v1"):
// which sectors are audio, the chunk's number, and the MISMATCH rule against what section 15 requires of a header.  Plain C++ for host
// and device: the scan and finish kernels (strspu_demux_kernels.hip) and the CPU check under the host sanitizers
// (tests/cpu/strspu_chunk_check.cpp) compile this text.  A header is handed over as its eight little-endian dwords.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STRSPU_HD __host__ __device__ inline
#else
#define STRSPU_HD inline
#endif

// what the settings say of the audio chunks: ch 0 (no audio), 1 or 2; id, d, loop from strspu_options; frequency 0 = not compared
struct StrspuChunkRules {
    int32_t ch;
    uint32_t id;
    int32_t d;                  // 1: the lanes start with the dummy block
    int32_t loop;
    uint32_t frequency;
};

// an audio sector: bytes 0, 1 are 60 01 and le16(2) is the audio chunk id (never with ch == 0)
STRSPU_HD bool strspu_is_audio(const uint32_t* h, const StrspuChunkRules& r) {
    return r.ch != 0 && (h[0] & 0xFFFFu) == 0x0160u && (h[0] >> 16) == r.id;
}

// k = le32(8) - 1 in 64 bits: -1 for the number 0, 2^32 - 2 for the number 2^32 - 1
STRSPU_HD int64_t strspu_chunk_number(const uint32_t* h) { return (int64_t)h[2] - 1; }

STRSPU_HD uint32_t strspu_chunk_flags(const uint32_t* h) { return h[7] & 0xFFFFu; }

// the header of chunk k (>= 0) disagrees with what section 15 writes for these settings
STRSPU_HD bool strspu_chunk_mismatch(const uint32_t* h, int64_t k, const StrspuChunkRules& r) {
    const int64_t B = r.ch ? 126 / r.ch : 0;
    const uint32_t flags = strspu_chunk_flags(h);
    const int64_t first = k == 0 ? 0 : 28 * (k * B - r.d);
    bool bad = (h[1] & 0xFFFFu) != 0u;                          // chunk index 0
    bad = bad || (h[1] >> 16) != 1u;                            // of 1
    bad = bad || h[3] != 2016u;                                 // bytes used
    bad = bad || (int32_t)(h[4] & 0xFFFFu) != r.ch;
    bad = bad || (int64_t)(h[4] >> 16) != 16 * B;               // lane bytes L
    bad = bad || (r.frequency != 0u && h[5] != r.frequency);
    bad = bad || (int64_t)h[6] != first;                        // the chunk's first sample per channel
    bad = bad || ((flags >> 1) & 1u) != (uint32_t)(k == 0 && r.d);
    bad = bad || ((flags >> 2) & 1u) != (uint32_t)(r.loop != 0);
    bad = bad || (flags >> 3) != 0u;
    return bad;
}
