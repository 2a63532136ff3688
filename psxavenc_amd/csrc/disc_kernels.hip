// disc_kernels.hip -- the disc finisher on the device for MI355X (gfx950), hand-written HIP: sectors as the encoders leave them ->
// interleaved raw Mode 2 sectors with sync, absolute BCD header, both subheader copies, EDC and (form 1) the P and Q Reed-Solomon
// parity of ECMA-130, and the check that is its inverse ("psxhip disc finish v1" / "psxhip disc check v1").
// One wavefront per sector, four sectors to a 256-thread workgroup, the sector in LDS as 588 dwords.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psxhip_disc_internal.h"
#include "xa_edc.h"

namespace {

constexpr int kSPG = PSXHIP_DISC_SECTORS_PER_GROUP;
constexpr int kSecWords = 2352 / 4;
constexpr int kSumWords = 88;                     // the P column sums of a sector: A[43] at 0, H[43] at 44
constexpr int kWaveWords = kSecWords + kSumWords;
constexpr int kEdc1 = 0x818 / 4, kEdc2 = 0x92C / 4, kP = 0x81C, kQ = 0x8C8;

__device__ __forceinline__ uint32_t to_bcd(int v) { return (uint32_t)(v + (v / 10) * 6); }

// header dword of the sector at `lba`: BCD minute, second, frame of lba + 150, mode 2 (cdrom.c:62-65)
__device__ __forceinline__ uint32_t header_word(int lba) {
    const int t = lba + 150;
    return to_bcd(t / 4500) | to_bcd((t / 75) % 60) << 8 | to_bcd(t % 75) << 16 | 0x02000000u;
}

// GF(2^8), polynomial 0x11D: four packed bytes times alpha, and times 3^-1 = 0xF4 = alpha^7 + alpha^6 + alpha^5 + alpha^4 + alpha^2
__device__ __forceinline__ uint32_t gf_x2(uint32_t x) { return ((x & 0x7F7F7F7Fu) << 1) ^ (((x >> 7) & 0x01010101u) * 0x1Du); }
__device__ __forceinline__ uint32_t gf_div3(uint32_t x) {
    const uint32_t x2 = gf_x2(gf_x2(x)), x4 = gf_x2(gf_x2(x2)), x5 = gf_x2(x4), x6 = gf_x2(x5), x7 = gf_x2(x6);
    return x2 ^ x4 ^ x5 ^ x6 ^ x7;
}

// P: the 86 byte-columns of d (sector byte 0xC on) are adjacent in memory, but a row of 86 bytes is no whole number of dwords; a PAIR
// of rows is (172 bytes = 43 dwords).  Lane t < 43 walks dword t of every row pair k: four columns at once, columns 0..85 of the even
// rows in bytes 0..85 of the pair and of the odd rows in bytes 86..171.  It leaves per byte position p the sums A_p = xor of x_k and
// H_p = sum (alpha^2)^(PAIRS-1-k) x_k (Horner), from which the caller combines positions m and 86 + m into a codeword's two sums.
// PAIRS = 12: the data rows (finish); 13: with the parity rows (check).  HDR0: read the header (d[0..3]) as zero.
template <int PAIRS, bool HDR0>
__device__ __forceinline__ void p_sums(const uint32_t* sec32, uint32_t* sums, int lane) {
    if (lane < 43) {
        uint32_t a = 0, h = 0;
#pragma unroll
        for (int k = 0; k < PAIRS; k++) {
            uint32_t x = sec32[3 + 43 * k + lane];
            if (HDR0 && k == 0 && lane == 0) x = 0;
            a ^= x;
            h = gf_x2(gf_x2(h)) ^ x;
        }
        sums[lane] = a;
        sums[44 + lane] = h;
    }
}

// Q: codeword m walks the diagonal d[((m >> 1) * 86 + (m & 1) + 88 i) mod 2236], i = 0..42: one lane per codeword, byte reads.  Leaves
// a = sum c_i and b = sum alpha^(42-i) c_i over the 43 data symbols.
template <bool HDR0>
__device__ __forceinline__ void q_sums(const uint8_t* sec, int m, uint32_t& a, uint32_t& b) {
    int idx = (m >> 1) * 86 + (m & 1);
    a = 0;
    b = 0;
#pragma unroll 1
    for (int i = 0; i < 43; i++) {
        uint32_t x = sec[12 + idx];
        if (HDR0 && idx < 4) x = 0;
        a ^= x;
        b = gf_x2(b) ^ x;
        idx += 88;
        if (idx >= 2236) idx -= 2236;
    }
}

// ---- finish.  Wavefront w of the workgroup builds output sector 4 g + w of the call in its own 588 dwords of LDS: source data by
// dword loads, subheader with the overrides, EDC (edc_wave), P, Q, then dword stores with the header put in on the way out -- in LDS
// the header stays zero, which is how the ECC wants it.  The barriers are workgroup-wide and outside every branch: the four sectors of
// a group may be of different forms.
__global__ __launch_bounds__(256) void disc_finish_kernel(const psxhip_disc_finish_job_t job) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kSPG * kWaveWords];
    __shared__ uint32_t crc_tab[256];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint32_t* const sec32 = lds + wave * kWaveWords;
    uint8_t* const sec = (uint8_t*)sec32;
    uint32_t* const sums = sec32 + kSecWords;

    crc_tab[tid] = c_xa_tables[tid];
    {
        const int64_t j = (int64_t)blockIdx.x * kSPG + wave, ja = job.first_out + j;
        const bool active = j < job.n_out;
        bool form1 = false;
        if (active) {
            const int q = (int)(ja % job.period);
            const int s = job.slot_source[q];
            uint32_t sub = 0x00200000u;           // the null sector: form 2, subheader 00 00 20 00
            const uint32_t* src = nullptr;        // the source sector, or none
            int lead4 = 0;
            if (s >= 0) {
                const psxhip_disc_dev_source_t& S = job.src[s];
                const int64_t idx = ja / job.period * S.count + job.slot_rank[q];
                if (idx < S.n_sectors) {
                    src = (const uint32_t*)(S.base + idx * S.stride);
                    lead4 = S.lead / 4;
                    sub = S.has_subheader ? src[4 - lead4] : S.data_subheader;
                    if (S.file >= 0) sub = (sub & 0xFFFFFF00u) | (uint32_t)S.file;
                    if (S.channel >= 0) sub = (sub & 0xFFFFE0FFu) | (uint32_t)S.channel << 8;
                }
            }
            form1 = (sub & 0x00200000u) == 0u;
            const int data_end = form1 ? kEdc1 : kEdc2;       // data dwords 6 .. data_end - 1 come from the source
            for (int i = lane; i < kSecWords; i += 64) {
                uint32_t v = 0;
                if (i >= 6 && i < data_end && src) v = src[i - lead4];
                if (i == 0) v = 0xFFFFFF00u;
                if (i == 1) v = 0xFFFFFFFFu;
                if (i == 2) v = 0x00FFFFFFu;
                if (i == 4 || i == 5) v = sub;
                sec32[i] = v;
            }
        }
        __syncthreads();
        if (active) {
            const uint32_t c = form1 ? edc_wave<kEdcSpanForm1>(sec32, crc_tab, lane) : edc_wave<kEdcSpan>(sec32, crc_tab, lane);
            if (lane == 0) sec32[form1 ? kEdc1 : kEdc2] = c;
        }
        __syncthreads();
        if (active && form1) p_sums<12, false>(sec32, sums, lane);
        __syncthreads();
        if (active && form1) {
            // codeword m: A = A_m ^ A_(86+m); the data symbol of row i weighs alpha^(25-i): alpha^3 H_m ^ alpha^2 H_(86+m)
            const uint8_t* ab = (const uint8_t*)sums;
            const uint8_t* hb = (const uint8_t*)(sums + 44);
            for (int m = lane; m < 86; m += 64) {
                const uint32_t a = (uint32_t)(ab[m] ^ ab[86 + m]);
                const uint32_t b = gf_x2(gf_x2(gf_x2(hb[m]) ^ hb[86 + m]));
                const uint32_t p0 = gf_div3(a ^ b) & 0xFFu;
                sec[kP + m] = (uint8_t)p0;
                sec[kP + 86 + m] = (uint8_t)(p0 ^ a);
            }
        }
        __syncthreads();
        if (active && form1 && lane < 52) {
            uint32_t a, b;
            q_sums<false>(sec, lane, a, b);
            const uint32_t q0 = gf_div3(a ^ gf_x2(gf_x2(b))) & 0xFFu;       // the data symbol i weighs alpha^(44-i)
            sec[kQ + lane] = (uint8_t)q0;
            sec[kQ + 52 + lane] = (uint8_t)(q0 ^ a);
        }
        __syncthreads();
        if (active) {
            const uint32_t hdr = header_word((int)(job.start_lba + ja));
            uint32_t* dst = (uint32_t*)(job.out + j * 2352);
            for (int i = lane; i < kSecWords; i += 64) dst[i] = i == 3 ? hdr : sec32[i];
        }
    }
}

// ---- check: the same sums with the parity symbols in them are the syndromes.  Bits per sector; the counts go through LDS to one
// atomic per non-zero counter and workgroup (a clean image: one, its form's).
__global__ __launch_bounds__(256) void disc_check_kernel(const psxhip_disc_check_job_t job) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kSPG * kWaveWords];
    __shared__ uint32_t crc_tab[256];
    __shared__ int tally[12];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint32_t* const sec32 = lds + wave * kWaveWords;
    const uint8_t* const sec = (const uint8_t*)sec32;
    uint32_t* const sums = sec32 + kSecWords;

    crc_tab[tid] = c_xa_tables[tid];
    if (tid < 12) tally[tid] = 0;
    {
        const int64_t j = (int64_t)blockIdx.x * kSPG + wave;
        const bool active = j < job.n_sectors;
        if (active) {
            const uint32_t* src = (const uint32_t*)(job.image + j * 2352);
            for (int i = lane; i < kSecWords; i += 64) sec32[i] = src[i];
        }
        __syncthreads();
        bool form1 = false;
        int st = 0;
        if (active) {
            const uint32_t hdr = sec32[3], sub0 = sec32[4], sub1 = sec32[5];
            form1 = (sub0 & 0x00200000u) == 0u;
            if (sec32[0] != 0xFFFFFF00u || sec32[1] != 0xFFFFFFFFu || sec32[2] != 0x00FFFFFFu) st |= PSXHIP_DISC_SYNC;
            if (job.start_lba >= 0) {
                if (hdr != header_word((int)(job.start_lba + j))) st |= PSXHIP_DISC_HEADER;
            } else {
                const uint32_t lo = hdr & 0x000F0F0Fu, hi = (hdr >> 4) & 0x000F0F0Fu;
                if ((hdr >> 24) != 2u || (((lo + 0x00060606u) | (hi + 0x00060606u)) & 0x00101010u)) st |= PSXHIP_DISC_HEADER;
            }
            if (sub0 != sub1) st |= PSXHIP_DISC_SUBHEADER;
            const uint32_t c = form1 ? edc_wave<kEdcSpanForm1>(sec32, crc_tab, lane) : edc_wave<kEdcSpan>(sec32, crc_tab, lane);
            const uint32_t edc = (uint32_t)__shfl((int)c, 0, 64), stored = sec32[form1 ? kEdc1 : kEdc2];
            if (!form1 && stored == 0u) st |= PSXHIP_DISC_EDC_ABSENT;
            else if (stored != edc) st |= PSXHIP_DISC_EDC;
            if (form1) p_sums<13, true>(sec32, sums, lane);
        }
        __syncthreads();
        if (active) {
            if (form1) {
                const uint8_t* ab = (const uint8_t*)sums;
                const uint8_t* hb = (const uint8_t*)(sums + 44);
                int bad_p = 0, bad_q = 0;
                for (int m = lane; m < 86; m += 64) {
                    // with the parity rows in, row i weighs alpha^(25-i): alpha H_m ^ H_(86+m)
                    const uint32_t s0 = (uint32_t)(ab[m] ^ ab[86 + m]), s1 = (gf_x2(hb[m]) ^ hb[86 + m]) & 0xFFu;
                    if (s0 | s1) bad_p = 1;
                }
                if (lane < 52) {
                    uint32_t a, b;
                    q_sums<true>(sec, lane, a, b);
                    const uint32_t y0 = sec[kQ + lane], y1 = sec[kQ + 52 + lane];
                    a ^= y0 ^ y1;
                    b = (gf_x2(gf_x2(b) ^ y0) ^ y1) & 0xFFu;
                    if (a | b) bad_q = 1;
                }
                if (__ballot(bad_p)) st |= PSXHIP_DISC_ECC_P;
                if (__ballot(bad_q)) st |= PSXHIP_DISC_ECC_Q;
            }
            if (lane == 0) {
                if (job.status) job.status[j] = st;
                atomicAdd(&tally[form1 ? 1 : 2], 1);
                if (st) atomicAdd(&tally[3], 1);
                if (st & PSXHIP_DISC_SYNC) atomicAdd(&tally[4], 1);
                if (st & PSXHIP_DISC_HEADER) atomicAdd(&tally[5], 1);
                if (st & PSXHIP_DISC_SUBHEADER) atomicAdd(&tally[6], 1);
                if (st & PSXHIP_DISC_EDC) atomicAdd(&tally[7], 1);
                if (st & PSXHIP_DISC_ECC_P) atomicAdd(&tally[8], 1);
                if (st & PSXHIP_DISC_ECC_Q) atomicAdd(&tally[9], 1);
                if (st & PSXHIP_DISC_EDC_ABSENT) atomicAdd(&tally[10], 1);
            }
        }
    }
    __syncthreads();
    if (tid >= 1 && tid < 11 && tally[tid]) atomicAdd(&((int*)job.summary)[tid], tally[tid]);
    if (tid == 0 && blockIdx.x == 0) job.summary->n_sectors = (int32_t)job.n_sectors;
}
}  // namespace

extern "C" int psxhip_disc_tables(int device) { return xa_tables(device); }

extern "C" hipError_t psxhip_disc_finish_launch(const psxhip_disc_finish_job_t* j, int grid, void* stream) {
    hipLaunchKernelGGL(disc_finish_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}

extern "C" hipError_t psxhip_disc_check_launch(const psxhip_disc_check_job_t* j, int grid, void* stream) {
    hipLaunchKernelGGL(disc_check_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}
