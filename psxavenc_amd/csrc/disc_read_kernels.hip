// disc_read_kernels.hip -- the disc reader on the device for MI355X (gfx950), hand-written HIP: a raw image of 2352-byte sectors ->
// damaged form-1 sectors repaired from their P and Q parity, every sector routed to a track by file, channel and submode, every
// track's sectors compacted in image order ("psxhip disc read v1").  Five kernels on one stream: classify
// (repair in LDS, verdict, routing key, one record per sector), count / prefix / place (the ordinals: per 1024-sector span and
// track a count, an exclusive scan over the spans, the rank inside the span), gather (the copy; a repaired sector is repaired again
// in LDS -- the repair is deterministic -- so no patch workspace exists).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psxhip_disc_read_internal.h"
#include "wave_ops.h"
#include "xa_edc.h"

namespace {

constexpr int kSPG = PSXHIP_DISC_READ_SECTORS_PER_GROUP;
constexpr int kSpan = PSXHIP_DISC_READ_SPAN;
constexpr int kSecWords = 2352 / 4;
constexpr int kSumWords = 88;                     // the P column sums of a sector: A[43] at 0, H[43] at 44
constexpr int kWaveWords = kSecWords + kSumWords;
constexpr int kEdc1 = 0x818 / 4, kEdc2 = 0x92C / 4, kQ = 0x8C8;
constexpr int kRounds = 4;                        // rounds that correct; one more pass of syndromes judges the fourth
constexpr int kFlags = kRounds + 1;
constexpr int64_t kGroupsPerLaunch = 1 << 23;     // 2^31 threads to a launch of classify or gather: 2^25 sectors

// log_alpha of GF(2^8), polynomial 0x11D (log 0 is never asked for)
struct GfLog {
    alignas(16) uint8_t v[256];
    constexpr GfLog() : v() {
        int x = 1;
        for (int i = 0; i < 255; i++) {
            v[x] = (uint8_t)i;
            x <<= 1;
            if (x & 0x100) x ^= 0x11D;
        }
    }
};
__constant__ const GfLog c_gf_log = GfLog();

// copies of the finisher's helpers (disc_kernels.hip is pinned to its two kernels; the EDC tables are copies the same way)
__device__ __forceinline__ uint32_t gf_x2(uint32_t x) { return ((x & 0x7F7F7F7Fu) << 1) ^ (((x >> 7) & 0x01010101u) * 0x1Du); }

// P column sums with the parity rows in and the header read as zero: lane t < 43 walks dword t of the 13 row pairs (172 bytes = 43
// dwords each) and leaves per byte position p of the pair A_p = xor x_k and H_p = sum (alpha^2)^(12-k) x_k
__device__ __forceinline__ void p_sums(const uint32_t* sec32, uint32_t* sums, int lane) {
    if (lane < 43) {
        uint32_t a = 0, h = 0;
#pragma unroll
        for (int k = 0; k < 13; k++) {
            uint32_t x = sec32[3 + 43 * k + lane];
            if (k == 0 && lane == 0) x = 0;
            a ^= x;
            h = gf_x2(gf_x2(h)) ^ x;
        }
        sums[lane] = a;
        sums[44 + lane] = h;
    }
}

// d index of symbol i < 43 of Q codeword m
__device__ __forceinline__ int q_index(int m, int i) { return ((m >> 1) * 86 + (m & 1) + 88 * i) % 2236; }

// Q syndromes of codeword m, parity symbols in, header as zero: s0 = sum c_i, s1 = sum alpha^(44-i) c_i
__device__ __forceinline__ void q_syndromes(const uint8_t* sec, int m, uint32_t& s0, uint32_t& s1) {
    int idx = (m >> 1) * 86 + (m & 1);
    uint32_t a = 0, b = 0;
#pragma unroll 1
    for (int i = 0; i < 43; i++) {
        uint32_t x = sec[12 + idx];
        if (idx < 4) x = 0;
        a ^= x;
        b = gf_x2(b) ^ x;
        idx += 88;
        if (idx >= 2236) idx -= 2236;
    }
    const uint32_t y0 = sec[kQ + m], y1 = sec[kQ + 52 + m];
    s0 = a ^ y0 ^ y1;
    s1 = (gf_x2(gf_x2(b) ^ y0) ^ y1) & 0xFFu;
}

// the symbol a codeword of n symbols with syndromes s0, s1 (both non-zero) has wrong if exactly one is, or -1
__device__ __forceinline__ int wrong_symbol(const uint8_t* log_tab, uint32_t s0, uint32_t s1, int n) {
    int e = (int)log_tab[s1] - (int)log_tab[s0];
    if (e < 0) e += 255;
    return e < n ? n - 1 - e : -1;
}

// Rules 2-4 of the repair on the sector in this wavefront's LDS, by ALL wavefronts of the workgroup: the barriers are workgroup-wide
// and outside every divergent branch, and the round loop's exit is workgroup-uniform (flags[r]: a wavefront goes on after round r).
// `want`: this wavefront's sector is to be repaired (wave-uniform).  Returns the corrections made; ecc_clean says that every P and Q
// syndrome of what is now in LDS is zero.  Every index is a function of the codeword number and a symbol number below n: nothing
// in the sector's bytes reaches an address.  Ends behind a barrier.
__device__ __forceinline__ int repair_rounds(uint32_t* sec32, uint32_t* sums, const uint8_t* log_tab, int* flags, int lane, bool want,
                                             bool& ecc_clean) {
    uint8_t* const sec = (uint8_t*)sec32;
    bool live = want;
    int total = 0;
    ecc_clean = false;
    for (int r = 0; r < kFlags; r++) {
        const bool fix = r < kRounds;
        int corr = 0, nz = 0;
        if (live) p_sums(sec32, sums, lane);
        __syncthreads();
        if (live) {
            const uint8_t* ab = (const uint8_t*)sums;
            const uint8_t* hb = (const uint8_t*)(sums + 44);
            for (int m = lane; m < 86; m += 64) {
                // row i weighs alpha^(25-i): alpha H_m ^ H_(86+m)
                const uint32_t s0 = (uint32_t)(ab[m] ^ ab[86 + m]), s1 = (gf_x2(hb[m]) ^ hb[86 + m]) & 0xFFu;
                if (s0 | s1) nz = 1;
                if (fix && s0 && s1) {
                    const int i = wrong_symbol(log_tab, s0, s1, 26);
                    const int k = m + 86 * i;
                    if (i >= 0 && k >= 4) {
                        sec[12 + k] ^= (uint8_t)s0;
                        corr++;
                    }
                }
            }
        }
        __syncthreads();
        if (live && lane < 52) {
            uint32_t s0, s1;
            q_syndromes(sec, lane, s0, s1);
            if (s0 | s1) nz = 1;
            if (fix && s0 && s1) {
                const int i = wrong_symbol(log_tab, s0, s1, 45);
                if (i >= 43) {
                    sec[kQ + 52 * (i - 43) + lane] ^= (uint8_t)s0;
                    corr++;
                } else if (i >= 0) {
                    const int k = q_index(lane, i);
                    if (k >= 4) {
                        sec[12 + k] ^= (uint8_t)s0;
                        corr++;
                    }
                }
            }
        }
        const int made = wave::reduce_add(corr);
        const bool dirty = wave::ballot(nz != 0) != 0;
        if (live) {
            total += made;
            if (made == 0) {
                live = false;
                ecc_clean = !dirty;
            }
        }
        if (live && lane == 0) flags[r] = 1;
        __syncthreads();
        if (!flags[r]) break;
    }
    return total;
}

__device__ __forceinline__ void load_sector(uint32_t* sec32, const uint32_t* src, int lane) {
    for (int i = lane; i < kSecWords; i += 64) sec32[i] = src[i];
}

// ---- classify.  Wavefront w of the workgroup takes sector 4 g + w into its own 588 dwords of LDS, repairs it there when it is a
// form-1 candidate, judges the result, and writes the record: track (the routing key of the repaired subheader against the track
// list, one lane per track, first match by ballot), status, corrections.  The counts go through LDS to one atomic per non-zero
// counter and workgroup.  A clean image leaves the round loop after one pass of syndromes, all zero: the check kernel's work.
__global__ __launch_bounds__(256) void disc_read_classify_kernel(const psxhip_disc_read_job_t job) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kSPG * kWaveWords];
    __shared__ uint32_t crc_tab[256];
    __shared__ uint32_t log_tab32[64];
    __shared__ int flags[kFlags];
    __shared__ int tally[16];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint32_t* const sec32 = lds + wave * kWaveWords;
    uint32_t* const sums = sec32 + kSecWords;

    crc_tab[tid] = c_xa_tables[tid];
    if (tid < 64) log_tab32[tid] = ((const uint32_t*)c_gf_log.v)[tid];
    if (tid < kFlags) flags[tid] = 0;
    if (tid < 16) tally[tid] = 0;
    const int64_t j = (job.first_group + blockIdx.x) * kSPG + wave;
    const bool active = j < job.n_sectors;
    const uint32_t* const src = (const uint32_t*)(job.image + j * 2352);
    if (active) load_sector(sec32, src, lane);
    __syncthreads();
    // rule 1: a form-1 candidate unless both copies of the submode say form 2
    const bool cand = active && ((sec32[4] & sec32[5]) & 0x00200000u) == 0u;
    bool ecc_clean;
    int corr = repair_rounds(sec32, sums, (const uint8_t*)log_tab32, flags, lane, cand, ecc_clean);
    bool ok = false;
    if (cand) {
        const uint32_t c = edc_wave<kEdcSpanForm1>(sec32, crc_tab, lane);
        ok = ecc_clean && (uint32_t)__shfl((int)c, 0, 64) == sec32[kEdc1];
        if (!ok) {
            if (corr > 0) load_sector(sec32, src, lane);      // a miscorrection never leaves: the input's bytes again
            corr = 0;
        }
    }
    __syncthreads();
    if (active) {
        int st = 0;
        bool form1 = ok;
        if (ok) {
            if (corr > 0) st |= PSXHIP_DISC_READ_REPAIRED;
        } else if ((sec32[4] & 0x00200000u) == 0u) {
            form1 = true;
            st |= PSXHIP_DISC_READ_UNREPAIRABLE;
        } else {
            const uint32_t c = edc_wave<kEdcSpan>(sec32, crc_tab, lane);
            const uint32_t edc = (uint32_t)__shfl((int)c, 0, 64), stored = sec32[kEdc2];
            if (stored == 0u) st |= PSXHIP_DISC_READ_EDC_ABSENT;
            else if (stored != edc) st |= PSXHIP_DISC_READ_EDC;
        }
        if (sec32[0] != 0xFFFFFF00u || sec32[1] != 0xFFFFFFFFu || sec32[2] != 0x00FFFFFFu) st |= PSXHIP_DISC_READ_SYNC;
        const uint32_t sub = sec32[4];
        if (sub != sec32[5]) st |= PSXHIP_DISC_READ_SUBHEADER;
        const uint32_t submode = (sub >> 16) & 0xFFu;
        int track = -1;
        if ((submode & 0x0Eu) == 0u) {
            st |= PSXHIP_DISC_READ_EMPTY;
        } else {
            bool hit = false;
            if (lane < job.n_tracks) {
                const uint32_t key = job.key[lane], f = key & 0x1FFu, ch = (key >> 9) & 0x3Fu;
                hit = (f == 0u || f - 1u == (sub & 0xFFu)) && (ch == 0u || ch - 1u == ((sub >> 8) & 0x1Fu)) &&
                      (submode & (key >> 16) & 0xFFu) == key >> 24;
            }
            const uint64_t hits = wave::ballot(hit);
            if (hits) track = __ffsll((unsigned long long)hits) - 1;
            else st |= PSXHIP_DISC_READ_UNCLAIMED;
        }
        if (track >= 0 && !form1 && job.track[track].lead4 == 6) st |= PSXHIP_DISC_READ_FORM;
        if (lane == 0) {
            psxhip_disc_read_sector_t rec;
            rec.track = track;
            rec.ordinal = -1;
            rec.status = st;
            rec.corrections = corr;
            job.table[j] = rec;
            atomicAdd(&tally[form1 ? 1 : 2], 1);
            if (ok) atomicAdd(&tally[corr > 0 ? 4 : 3], 1);
            if (st & PSXHIP_DISC_READ_UNREPAIRABLE) atomicAdd(&tally[5], 1);
            if (st & PSXHIP_DISC_READ_EDC) atomicAdd(&tally[6], 1);
            if (st & PSXHIP_DISC_READ_EDC_ABSENT) atomicAdd(&tally[7], 1);
            if (st & PSXHIP_DISC_READ_SYNC) atomicAdd(&tally[8], 1);
            if (st & PSXHIP_DISC_READ_SUBHEADER) atomicAdd(&tally[9], 1);
            if (st & PSXHIP_DISC_READ_EMPTY) atomicAdd(&tally[10], 1);
            if (st & PSXHIP_DISC_READ_UNCLAIMED) atomicAdd(&tally[11], 1);
            if (corr > 0) atomicAdd(&tally[13], corr);
        }
    }
    __syncthreads();
    if (tid >= 1 && tid < 12 && tally[tid]) atomicAdd(&((int*)job.summary)[tid], tally[tid]);
    if (tid == 13 && tally[13]) atomicAdd((unsigned long long*)&job.summary->n_corrections, (unsigned long long)tally[13]);
    if (tid == 0 && j == 0) job.summary->n_sectors = (int32_t)job.n_sectors;
}

// ---- count / place.  One wavefront per span of 1024 sectors, 64 records at a time; lane t holds the number for track t.  The
// records of one step are taken key by key: the first lane's key, a ballot of the lanes that have it, until none is left -- as many
// rounds as the step has different tracks.
__global__ __launch_bounds__(64) void disc_read_count_kernel(const psxhip_disc_read_job_t job) {
    const int lane = (int)threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kSpan;
    int cnt = 0;
    for (int it = 0; it < kSpan / 64; it++) {
        const int64_t i = base + it * 64 + lane;
        const int key = i < job.n_sectors ? job.table[i].track : -1;
        uint64_t todo = wave::ballot(key >= 0);
        while (todo) {
            const int k = __shfl(key, __ffsll((unsigned long long)todo) - 1, 64);
            const uint64_t same = wave::ballot(key == k);
            if (lane == k) cnt += __popcll(same);
            todo &= ~same;
        }
    }
    job.span_counts[(int64_t)blockIdx.x * 64 + lane] = cnt;
}

// ---- prefix: one wavefront per track turns its column of span counts into the sectors before each span, 64 spans at a time, and
// leaves the track's count and its dropped sectors
__global__ __launch_bounds__(64) void disc_read_prefix_kernel(const psxhip_disc_read_job_t job) {
    const int lane = (int)threadIdx.x, t = (int)blockIdx.x;
    int carry = 0;
    for (int b0 = 0; b0 < job.n_spans; b0 += 64) {
        const int b = b0 + lane;
        const int v = b < job.n_spans ? job.span_counts[(int64_t)b * 64 + t] : 0;
        const int incl = wave::inclusive_scan_add(v);
        if (b < job.n_spans) job.span_counts[(int64_t)b * 64 + t] = carry + incl - v;
        carry += __builtin_amdgcn_readlane(incl, 63);
    }
    if (lane == 0) {
        job.track_counts[t] = carry;
        const int dropped = carry - job.track[t].capacity;
        if (dropped > 0) atomicAdd(&job.summary->n_dropped, dropped);
    }
}

__global__ __launch_bounds__(64) void disc_read_place_kernel(const psxhip_disc_read_job_t job) {
    const int lane = (int)threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kSpan;
    int run = job.span_counts[(int64_t)blockIdx.x * 64 + lane];
    const int cap = lane < job.n_tracks ? job.track[lane].capacity : 0;
    for (int it = 0; it < kSpan / 64; it++) {
        const int64_t i = base + it * 64 + lane;
        const int key = i < job.n_sectors ? job.table[i].track : -1;
        int ordinal = -1, room = 0;
        uint64_t todo = wave::ballot(key >= 0);
        while (todo) {
            const int k = __shfl(key, __ffsll((unsigned long long)todo) - 1, 64);
            const uint64_t same = wave::ballot(key == k);
            const int before = __shfl(run, k, 64), cap_k = __shfl(cap, k, 64);
            if (key == k) {
                ordinal = before + wave::popc_below(same);
                room = cap_k;
            }
            if (lane == k) run += __popcll(same);
            todo &= ~same;
        }
        if (key >= 0) {
            job.table[i].ordinal = ordinal;
            if (ordinal >= room) job.table[i].status |= PSXHIP_DISC_READ_DROPPED;
        }
    }
}

// ---- gather.  One wavefront per sector: its record says where it goes.  A sector the classify kernel repaired goes through LDS
// and the same rounds again; every other one is a straight copy, coalesced dwords both ways, in the track's sector size.
__global__ __launch_bounds__(256) void disc_read_gather_kernel(const psxhip_disc_read_job_t job) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kSPG * kWaveWords];
    __shared__ uint32_t log_tab32[64];
    __shared__ int flags[kFlags];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint32_t* const sec32 = lds + wave * kWaveWords;
    uint32_t* const sums = sec32 + kSecWords;

    if (tid < 64) log_tab32[tid] = ((const uint32_t*)c_gf_log.v)[tid];
    if (tid < kFlags) flags[tid] = 0;
    const int64_t j = (job.first_group + blockIdx.x) * kSPG + wave;
    int track = -1, ordinal = -1, status = 0;
    if (j < job.n_sectors) {
        const psxhip_disc_read_sector_t rec = job.table[j];
        track = __builtin_amdgcn_readfirstlane(rec.track);
        ordinal = __builtin_amdgcn_readfirstlane(rec.ordinal);
        status = __builtin_amdgcn_readfirstlane(rec.status);
    }
    // the record is this call's own; its numbers are bounded all the same before they reach an address
    const bool write = track >= 0 && track < job.n_tracks && ordinal >= 0 && ordinal < job.track[track < 0 ? 0 : track & 63].capacity;
    const bool fix = write && (status & PSXHIP_DISC_READ_REPAIRED);
    const uint32_t* const src = (const uint32_t*)(job.image + j * 2352);
    if (fix) load_sector(sec32, src, lane);
    __syncthreads();
    bool ecc_clean;
    repair_rounds(sec32, sums, (const uint8_t*)log_tab32, flags, lane, fix, ecc_clean);
    if (write) {
        const psxhip_disc_read_dev_track_t& T = job.track[track];
        uint32_t* const dst = (uint32_t*)(T.base + (int64_t)ordinal * T.stride);
        const int lead4 = T.lead4, size4 = T.size4;
        if (fix) {
            for (int i = lane; i < size4; i += 64) dst[i] = sec32[lead4 + i];
        } else {
            for (int i = lane; i < size4; i += 64) dst[i] = src[lead4 + i];
        }
    }
}
}  // namespace

extern "C" int psxhip_disc_read_tables(int device) { return xa_tables(device); }

extern "C" hipError_t psxhip_disc_read_launch(const psxhip_disc_read_job_t* j, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int64_t groups = (j->n_sectors + kSPG - 1) / kSPG;
    psxhip_disc_read_job_t part = *j;
    for (part.first_group = 0; part.first_group < groups; part.first_group += kGroupsPerLaunch) {
        const int64_t left = groups - part.first_group;
        hipLaunchKernelGGL(disc_read_classify_kernel, dim3((unsigned)(left < kGroupsPerLaunch ? left : kGroupsPerLaunch)), dim3(256), 0, st, part);
    }
    if (j->n_tracks > 0) {
        hipLaunchKernelGGL(disc_read_count_kernel, dim3((unsigned)j->n_spans), dim3(64), 0, st, *j);
        hipLaunchKernelGGL(disc_read_prefix_kernel, dim3((unsigned)j->n_tracks), dim3(64), 0, st, *j);
        hipLaunchKernelGGL(disc_read_place_kernel, dim3((unsigned)j->n_spans), dim3(64), 0, st, *j);
        for (part.first_group = 0; part.first_group < groups; part.first_group += kGroupsPerLaunch) {
            const int64_t left = groups - part.first_group;
            hipLaunchKernelGGL(disc_read_gather_kernel, dim3((unsigned)(left < kGroupsPerLaunch ? left : kGroupsPerLaunch)), dim3(256), 0, st, part);
        }
    }
    return hipGetLastError();
}
