// adpcm_decode_core.h -- "psxhip ADPCM decode v1"  as plain C++ for host and device: the header byte, the code
// unpacking of both record layouts and the unit step.  The kernels (adpcm_decode_kernels.hip) compile this text; tests/cpu/
// adpcm_decode_sim.cpp runs the same text on the CPU under the host sanitizers, against tests/adpcm_decode_ref.py.
//
// Integers only; >> is arithmetic.  For a unit with header byte h and 28 codes c[i] of 4 or 8 bits:
//   R = 12 (4-bit) or 8 (8-bit); s = h & 15; f = h >> 4 (& 3 when filter_count == 4);
//   k1 = {0, 60, 115, 98, 122}[f], k2 = {0, 0, -52, -55, -60}[f]; f >= 5: k1 = k2 = 0 and flag bit 0; s > R: flag bit 1
//   t = sext16((c[i] << R) & 0xFFFF) >> s;  d = clamp(t + ((k1 p1 + k2 p2 + 32) >> 6), -32768, 32767);  p2 = p1;  p1 = d
// (the reconstruction inside the reference's encoder, libpsxav/adpcm.c:120-124, state :135-136).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PSXHIP_HD __host__ __device__ __forceinline__
#else
#define PSXHIP_HD inline
#endif

enum { PSXHIP_ADPCM_FLAG_FILTER = 1, PSXHIP_ADPCM_FLAG_SHIFT = 2 };

struct AdpcmDecHeader {
    int k1, k2, shift, flags;
};

// (the two filter tables as bytes of a constant: an indexed table would live in memory on the device)
PSXHIP_HD AdpcmDecHeader adpcm_dec_header(uint32_t h, int filter_count, int range) {
    AdpcmDecHeader r;
    r.shift = (int)(h & 15u);
    int f = (int)((h >> 4) & 15u);
    if (filter_count == 4) f &= 3;
    const bool bad = f >= 5;
    const int sh = bad ? 0 : 8 * f;
    r.k1 = bad ? 0 : (int)((0x7A62733C00ull >> sh) & 0xFFu);
    r.k2 = bad ? 0 : -(int)((0x3C37340000ull >> sh) & 0xFFu);
    r.flags = (bad ? PSXHIP_ADPCM_FLAG_FILTER : 0) | (r.shift > range ? PSXHIP_ADPCM_FLAG_SHIFT : 0);
    return r;
}

// the code of sample i as a signed number of BITS bits.  4-bit record (an SPU block): byte 0 header, byte 1 loop flags (ignored),
// byte 2 + i / 2 holds sample i in its low (i even) or high nibble.  8-bit record: byte 0 header, byte 4 + i the code.
template <int BITS>
PSXHIP_HD int adpcm_dec_code(const uint32_t* w, int i) {
    if (BITS == 4) {
        const int nib = 4 + i;
        return (int)(w[nib >> 3] << (28 - 4 * (nib & 7))) >> 28;
    }
    const int b = 4 + i;
    return (int)(w[b >> 2] << (24 - 8 * (b & 3))) >> 24;
}

// one sample.  code * 2^range is sext16((c << range) & 0xFFFF): bits + range = 16.  |k1 p1 + k2 p2| < 2^23.
PSXHIP_HD int adpcm_dec_sample(int code, int range, const AdpcmDecHeader& h, int p1, int p2) {
    const int t = (code * (1 << range)) >> h.shift;
    const int d = t + ((h.k1 * p1 + h.k2 * p2 + 32) >> 6);
    return d < -32768 ? -32768 : (d > 32767 ? 32767 : d);
}

// one unit: w = the record's dwords (4 for 4-bit codes, 8 for 8-bit), little-endian.  out[k] = sample 2k | sample 2k+1 << 16.
// Returns the unit's flags; p1 / p2 are carried.
template <int BITS>
PSXHIP_HD int adpcm_dec_unit(const uint32_t* w, int filter_count, int& p1, int& p2, uint32_t* out) {
    constexpr int kRange = BITS == 4 ? 12 : 8;
    const AdpcmDecHeader h = adpcm_dec_header(w[0] & 0xFFu, filter_count, kRange);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 14; k++) {
        const int a = adpcm_dec_sample(adpcm_dec_code<BITS>(w, 2 * k), kRange, h, p1, p2);
        const int b = adpcm_dec_sample(adpcm_dec_code<BITS>(w, 2 * k + 1), kRange, h, a, p1);
        p2 = a;
        p1 = b;
        out[k] = (uint32_t)(a & 0xFFFF) | (uint32_t)b << 16;
    }
    return h.flags;
}

// ---- cutting chains into chunks (speculate and verify along time): the arithmetic the host tables and the kernel share
// units a chunk starting at chain-local unit `first` decodes in front of itself to guess its start state
PSXHIP_HD int adpcm_dec_warm(int first, int warmup_units) { return first < warmup_units ? first : warmup_units; }
// a unit's last two samples were stored (they can be read back as its end state) when the whole unit lies below sample_limit
PSXHIP_HD bool adpcm_dec_unit_stored(int u, int sample_limit) { return (long long)u * 28 + 28 <= (long long)sample_limit; }
