// xa_edc.h -- the EDC (CRC-32, polynomial 0xD8018001) of a CD-ROM XA sector by one wavefront, and the tables it needs.  Shared by the
// sector kernels (sector_kernels.hip) and the STR reader (str_demux_kernels.hip); every translation unit that includes it owns a
// copy of the tables and uploads it with its own xa_tables().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "psxhip_internal.h"

namespace {

// EDC tables, the same for every sector: built once on the host (xa_tables()).
//   [0..255]          reflected CRC-32 table for polynomial 0xD8018001 (cdrom.c:28-41), copied into LDS by every workgroup
//   [256 + 32 j + b]  CRC state (1 << b) advanced over 40 * 2^j zero bytes, j = 0..5 (read through the scalar cache)
__constant__ uint32_t c_xa_tables[256 + 8 * 32];

constexpr int kEdcChunk = 40;                       // bytes per lane of the wavefront that computes the EDC
constexpr int kEdcSpan = 0x91C;                     // form 2: sector bytes 0x10 .. 0x92B (cdrom.c:102-110)
constexpr int kEdcSpanForm1 = 0x808;                // form 1: sector bytes 0x10 .. 0x817 (cdrom.c:92-100)

// CRC state c advanced over 40 * 2^J zero bytes: the xor of the table rows of its set bits (the CRC is linear over GF(2))
template <int J>
__device__ __forceinline__ uint32_t edc_advance(uint32_t c) {
    uint32_t r = 0;
#pragma unroll
    for (int bit = 0; bit < 32; bit++) r ^= c_xa_tables[256 + 32 * J + bit] & (uint32_t)(((int)(c << (31 - bit))) >> 31);
    return r;
}

// The EDC of SPAN bytes from sector byte 0x10 on, by ONE wavefront (all 64 lanes call; the result is lane 0's).  The CRC has zero
// init and no final xor, so it is linear over GF(2): the CRC of the span is the xor of the CRCs of its chunks, each advanced over the
// zero bytes that follow it.  Lane t runs the table CRC over chunk t of 40 bytes (64 x 40 bytes = the span behind some zero bytes of
// padding in front, which change nothing), then six rounds of a binary tree -- lane t takes its partial advanced over 40 * 2^j zero
// bytes xor the partial 2^j lanes up -- leave the span's EDC in lane 0.
template <int SPAN>
__device__ __forceinline__ uint32_t edc_wave(const uint32_t* sec32, const uint32_t* crc_tab, int lane) {
    constexpr int kPad = 64 * kEdcChunk - SPAN;
    static_assert(kPad >= 0 && kPad % 4 == 0 && kEdcChunk % 4 == 0, "the lanes' chunks are whole dwords of the sector");
    uint32_t c = 0;
    const int d0 = lane * (kEdcChunk / 4) - kPad / 4;        // first dword of the chunk, relative to sector byte 0x10
#pragma unroll
    for (int i = 0; i < kEdcChunk / 4; i++) {
        const int d = d0 + i;
        c ^= d >= 0 ? sec32[4 + d] : 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) c = (c >> 8) ^ crc_tab[c & 0xFF];
    }
    c = edc_advance<0>(c) ^ (uint32_t)__shfl_down((int)c, 1, 64);
    c = edc_advance<1>(c) ^ (uint32_t)__shfl_down((int)c, 2, 64);
    c = edc_advance<2>(c) ^ (uint32_t)__shfl_down((int)c, 4, 64);
    c = edc_advance<3>(c) ^ (uint32_t)__shfl_down((int)c, 8, 64);
    c = edc_advance<4>(c) ^ (uint32_t)__shfl_down((int)c, 16, 64);
    c = edc_advance<5>(c) ^ (uint32_t)__shfl_down((int)c, 32, 64);
    return c;
}

}  // namespace

// builds c_xa_tables on the host and uploads it, once per device
static int xa_tables(int device) {
    static bool done[64] = {false};
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (device >= 0 && device < 64 && done[device]) return PSXHIP_OK;
    uint32_t t[256 + 8 * 32];
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t v = i;
        for (int k = 0; k < 8; k++) v = (v >> 1) ^ ((v & 1u) ? 0xD8018001u : 0u);
        t[i] = v;
    }
    uint32_t* z = t + 256;
    for (int b = 0; b < 32; b++) {
        uint32_t v = 1u << b;
        for (int i = 0; i < kEdcChunk; i++) v = (v >> 8) ^ t[v & 0xFF];
        z[b] = v;
    }
    for (int k = 1; k < 8; k++)
        for (int b = 0; b < 32; b++) {
            const uint32_t v = z[32 * (k - 1) + b];
            uint32_t r = 0;
            for (int bit = 0; bit < 32; bit++)
                if ((v >> bit) & 1u) r ^= z[32 * (k - 1) + bit];
            z[32 * k + b] = r;
        }
    if (hipMemcpyToSymbol(HIP_SYMBOL(c_xa_tables), t, sizeof t) != hipSuccess) {
        psxhip_set_error("xa_assemble: table upload failed");
        return PSXHIP_EDEVICE;
    }
    if (device >= 0 && device < 64) done[device] = true;
    return PSXHIP_OK;
}
