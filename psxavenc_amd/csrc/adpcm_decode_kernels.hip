// adpcm_decode_kernels.hip -- the ADPCM way back for MI355X (gfx950), hand-written HIP: unit records -> int16 PCM
// (adpcm_decode_kernel), the sums of squared errors of two sample sets per unit and per chain (adpcm_sse_kernel), XA sectors -> unit
// records (xa_disassemble_kernel), and the device-level entry points of include/psxav_hip.h that launch them.  The arithmetic is
// "psxhip ADPCM decode v1" (adpcm_decode_core.h): the reconstruction inside the reference's encoder
// (libpsxav/adpcm.c:120-124,135-136).
//
// A chain is serial in time -- the last two decoded samples feed the next one -- and a decode step is a handful of dependent integer
// instructions with nothing to search, so ONE LANE is one work item: a whole chain, or one chunk of a chain (speculate and verify
// along time, like adpcm_chunks_kernel on the encode side).  A unit moves 16 (32) bytes in and 56 out against ~250 instructions of
// arithmetic: the kernel is bound by how it touches memory, so it never lets a lane touch global memory for its own unit.  Work goes
// in ROUNDS of kRound units per lane:
//   1. the wavefront fetches every lane's run of records as 16-byte pieces, PP lanes per work item, into LDS -- the NEXT round's
//      pieces are fetched into registers before this round is decoded, and staged after it;
//   2. each lane reads its records from its LDS row (ds_read_b128), decodes, and writes 14 dwords per unit into its output row;
//   3. the wavefront writes each work item's contiguous output (kRound x 56 bytes) with one 256-byte-wide store instruction.
// Rows are padded (input + 16 bytes, output + 8 bytes) so that the per-lane 128-bit reads and 64-bit writes of 64 lanes spread
// over all banks instead of landing on a few.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "adpcm_decode_core.h"
#include "device_buffer.h"
#include "host_layout.h"
#include "psxhip_internal.h"
#include "xa_edc.h"

#define PSXHIP_ADPCM_DECODE_KERNEL_REV "adpcm-dec-k1.0"

namespace {

// Units per lane and round.  LDS per wavefront: 64 x (kRound x 16 + 16) bytes of records (4-bit; 64 x (kRound x 32 + 16) for 8-bit)
// + 64 x (kRound x 56 + 8) bytes of samples = 19.5 KiB (23.5 KiB) at kRound 4: eight (six) wavefronts per CU, two per SIMD, each with
// its next round's records in flight while it decodes.  kRound 8 would make a work item's run of 4-bit records a whole 128-byte line,
// but costs 37 KiB per wavefront -- one wavefront per SIMD, nothing to overlap its write-out with; kRound 2 (10.7 KiB, four per SIMD)
// leaves 32-byte runs and half-empty store instructions and measured slower on config 5: 4.5 ms against 3.9.
// kRound x 14 output dwords per work item must fit one store instruction of the wavefront.
constexpr int kRound = 4;
static_assert(kRound * 14 <= 64, "a work item's round is written by one store instruction of the wavefront");

__device__ __forceinline__ unsigned long long pack_state(int p1, int p2) {
    return (unsigned long long)(uint32_t)p1 | (unsigned long long)(uint32_t)p2 << 32;
}

struct DecodeJob {
    const uint8_t* units;
    const psxhip_adpcm_chain_t* chains;
    const int32_t* unit_base;
    int n_items;                         // work items: chains, or chunks when chunk_chain is given
    int filter_count;
    psxhip_adpcm_state_t* states;        // [n_chains] serial: read and updated; chunked: the start state of every chain's first chunk
    int16_t* samples;
    uint8_t* unit_flags;                 // optional: one byte per record index
    int16_t* tail;                       // optional: 28 samples per chain, the unit sample_limit cuts
    const int32_t* chunk_chain;          // [n_items] chain of each chunk; NULL: one work item per chain
    const int32_t* chunk_first;          // [n_items] first unit (chain-local) of each chunk
    const int32_t* chunk_pred;           // [n_items] the chunk in front of it in its chain (-1: the chain's first).  The two chains of an
                                         //           interleaved stereo pair alternate chunk by chunk, so that L and R of the same stretch of
                                         //           time are neighbouring lanes (see the write-out)
    int chunk_units, warmup_units;
    unsigned long long* start_used;      // [n_items] state each chunk was last decoded from (pack_state)
    unsigned long long* chunk_end;       // [n_items] state behind each chunk's last unit -- kept here, not read back from PCM that
                                         //           sample_limit may have kept from being stored
    int* changed;                        // verify: set to 1 when any chunk was decoded again
    const int* changed_before;           // verify: the previous pass's word (NULL: first pass of a batch); 0 there = nothing to do
};

template <int BITS>
struct Geo {
    static constexpr int kRecBytes = BITS == 4 ? 16 : 32;
    static constexpr int kRecWords = kRecBytes / 4;
    static constexpr int kPieces = kRound * kRecBytes / 16;       // 16-byte pieces per work item and round = lanes that fetch one item
    static constexpr int kInRow = kRound * kRecWords + 4;         // dwords per LDS input row (16 bytes of padding)
    static constexpr int kOutRow = kRound * 14 + 2;               // dwords per LDS output row (8 bytes of padding)
    static_assert(64 % kPieces == 0, "whole work items per fetch instruction");
};

// what a lane knows about its work item's current round
struct Round {
    long long rec;        // record index of the round's unit 0
    int stride;           // record stride
    int n;                // units of the round this lane wants (0 .. kRound)
};

template <int BITS>
__device__ __forceinline__ void fetch_round(const uint8_t* units, const Round& r, int lane, uint4 (&buf)[Geo<BITS>::kPieces]) {
    using G = Geo<BITS>;
    const int q = lane % G::kPieces, j = q / (G::kRecBytes / 16), part = q % (G::kRecBytes / 16);
#pragma unroll
    for (int i = 0; i < G::kPieces; i++) {
        const int sl = lane / G::kPieces + (64 / G::kPieces) * i;
        const int n = __shfl(r.n, sl, 64), stride = __shfl(r.stride, sl, 64);
        const long long rec = (long long)(((unsigned long long)(uint32_t)__shfl((int)(r.rec >> 32), sl, 64) << 32) |
                                          (uint32_t)__shfl((int)r.rec, sl, 64));
        buf[i] = make_uint4(0u, 0u, 0u, 0u);
        if (j < n) buf[i] = *(const uint4*)(units + (rec + (long long)j * stride) * G::kRecBytes + part * 16);
    }
}

template <int BITS>
__device__ __forceinline__ void stage_round(uint32_t* in_lds, int lane, const uint4 (&buf)[Geo<BITS>::kPieces]) {
    using G = Geo<BITS>;
#pragma unroll
    for (int i = 0; i < G::kPieces; i++) {
        const int sl = lane / G::kPieces + (64 / G::kPieces) * i;
        *(uint4*)&in_lds[sl * G::kInRow + (lane % G::kPieces) * 4] = buf[i];
    }
}

template <bool VERIFY, int BITS>
__global__ __launch_bounds__(64) void adpcm_decode_kernel(const DecodeJob job) {
    using G = Geo<BITS>;
    __shared__ __attribute__((aligned(16))) uint32_t in_lds[64 * G::kInRow];
    __shared__ __attribute__((aligned(16))) uint32_t out_lds[64 * G::kOutRow];
    // verify passes are launched in batches, back to back: the passes behind the one that changed nothing fall through here
    if (VERIFY && job.changed_before && *job.changed_before == 0) return;
    const int lane = (int)(threadIdx.x & 63);
    const int item = (int)blockIdx.x * 64 + lane;
    const bool live = item < job.n_items;
    const bool chunked = job.chunk_chain != nullptr;

    psxhip_adpcm_chain_t ch;
    ch.sample_offset = 0; ch.pitch = 1; ch.sample_limit = 0; ch.n_units = 0; ch.unit_stride = 1;
    int c = 0, first = 0, count = 0, warm = 0, p1 = 0, p2 = 0;
    long long rec0 = 0;
    bool active = false;
    if (live) {
        c = chunked ? job.chunk_chain[item] : item;
        ch = job.chains[c];
        rec0 = job.unit_base[c];
        first = chunked ? job.chunk_first[item] : 0;
        count = chunked ? min(job.chunk_units, ch.n_units - first) : ch.n_units;
        count = max(count, 0);
        if (!VERIFY) {
            active = count > 0;
            if (first == 0) {
                p1 = job.states[c].prev1;
                p2 = job.states[c].prev2;
            } else {
                warm = adpcm_dec_warm(first, job.warmup_units);       // decoded from silence, output discarded
            }
        } else if (first > 0) {                                       // (a chain's first chunk started from the truth)
            const unsigned long long used = job.start_used[item], truth = job.chunk_end[job.chunk_pred[item]];
            if (used != truth) {
                active = true;
                p1 = (int)(uint32_t)truth;
                p2 = (int)(uint32_t)(truth >> 32);
                job.start_used[item] = truth;
                *job.changed = 1;
            }
        }
    }
    if (VERIFY && !__any(active)) return;

    const int limit = max(ch.sample_limit, 0);
    const int cut_unit = limit % 28 ? limit / 28 : -1;            // the unit sample_limit cuts, if any
    const int u_begin = first - warm;
    const int total = active ? warm + count : 0;
    int t_max = total;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t_max = max(t_max, __shfl_xor(t_max, off, 64));

    bool running = active;
    uint4 buf[G::kPieces];
    Round rd;
    rd.stride = ch.unit_stride;
    rd.rec = rec0 + (long long)u_begin * ch.unit_stride;
    rd.n = min(total, kRound);
    fetch_round<BITS>(job.units, rd, lane, buf);
    stage_round<BITS>(in_lds, lane, buf);
    __syncthreads();

    for (int base = 0; base < t_max; base += kRound) {
        const bool more = base + kRound < t_max;
        if (more) {                                                // the next round's records travel while this one is decoded
            rd.rec = rec0 + (long long)(u_begin + base + kRound) * ch.unit_stride;
            rd.n = running ? min(max(total - base - kRound, 0), kRound) : 0;
            fetch_round<BITS>(job.units, rd, lane, buf);
        }
        const int n = running ? min(max(total - base, 0), kRound) : 0;
        const int u0 = u_begin + base;
        // (verify) the end states this chunk stored for the round's units the last time: two samples each, where they were stored
        uint32_t old_end[kRound];
        if (VERIFY) {
#pragma unroll
            for (int j = 0; j < kRound; j++) {
                old_end[j] = 0;
                if (j < n && adpcm_dec_unit_stored(u0 + j, limit)) {
                    const int16_t* s = job.samples + ch.sample_offset + ((long long)(u0 + j) * 28 + 26) * ch.pitch;
                    old_end[j] = (uint32_t)(uint16_t)s[0] | (uint32_t)(uint16_t)s[ch.pitch] << 16;
                }
            }
        }
        int done = 0;
#pragma unroll
        for (int j = 0; j < kRound; j++) {
            if (j < n && running) {
                const int u = u0 + j;
                if (!VERIFY && chunked && first > 0 && u == first) job.start_used[item] = pack_state(p1, p2);     // the guess
                uint32_t w[G::kRecWords], out[14];
#pragma unroll
                for (int k = 0; k < G::kRecWords / 4; k++) {
                    const uint4 v = *(const uint4*)&in_lds[lane * G::kInRow + j * G::kRecWords + 4 * k];
                    w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
                }
                const int flags = adpcm_dec_unit<BITS>(w, job.filter_count, p1, p2, out);
#pragma unroll
                for (int k = 0; k < 7; k++) *(uint2*)&out_lds[lane * G::kOutRow + j * 14 + 2 * k] = make_uint2(out[2 * k], out[2 * k + 1]);
                if (u >= first) {
                    if (job.unit_flags) job.unit_flags[rec0 + (long long)u * ch.unit_stride] = (uint8_t)flags;
                    if (job.tail && u == cut_unit) {
#pragma unroll
                        for (int k = 0; k < 14; k++) ((uint32_t*)job.tail)[(size_t)c * 14 + k] = out[k];
                    }
                    // (verify) the same end state as the last time: everything behind this unit is consistent already
                    if (VERIFY && adpcm_dec_unit_stored(u, limit) && old_end[j] == ((uint32_t)(p2 & 0xFFFF) | (uint32_t)p1 << 16))
                        running = false;
                }
                done = j + 1;
            }
        }
        __syncthreads();

        // ---- write-out: work item by work item, the whole wavefront on one item's contiguous samples
        const int skip = min(max(first - u0, 0), kRound);           // warm-up units of the round: decoded, not stored
        const long long e_lo = (long long)(u0 + skip) * 28;
        long long e_hi = (long long)(u0 + done) * 28;
        e_hi = e_hi < limit ? e_hi : limit;
        const int cnt = done > skip && e_hi > e_lo ? (int)(e_hi - e_lo) : 0;
        const long long elem = ch.sample_offset + e_lo * ch.pitch;
        unsigned long long todo = __ballot(cnt > 0);
        while (todo) {
            const int m = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int cnt_m = __builtin_amdgcn_readlane(cnt, m), pitch_m = __builtin_amdgcn_readlane(ch.pitch, m);
            const int skip_m = __builtin_amdgcn_readlane(skip, m);
            const long long elem_m = (long long)(((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(elem >> 32), m) << 32) |
                                                 (uint32_t)__builtin_amdgcn_readlane((int)elem, m));
            const uint32_t* row = out_lds + m * G::kOutRow + skip_m * 14;
            int16_t* dst = job.samples + elem_m;
            if (pitch_m == 2 && m < 63 && ((todo >> (m + 1)) & 1ull) && !((uintptr_t)dst & 3)) {
                // the next lane holds the other channel of an interleaved pair over the same stretch of time: L | R << 16 are whole
                // dwords, contiguous -- 256 bytes per store instruction instead of 64 two-byte stores four bytes apart, twice
                const int n1 = m + 1;
                const long long elem_n = (long long)(((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(elem >> 32), n1) << 32) |
                                                     (uint32_t)__builtin_amdgcn_readlane((int)elem, n1));
                if (__builtin_amdgcn_readlane(ch.pitch, n1) == 2 && elem_n == elem_m + 1 && __builtin_amdgcn_readlane(cnt, n1) == cnt_m) {
                    todo &= todo - 1;                                     // bit m + 1: the lowest one left
                    const uint32_t* row2 = out_lds + n1 * G::kOutRow + __builtin_amdgcn_readlane(skip, n1) * 14;
                    for (int k = lane; k < cnt_m; k += 64) {
                        const int sh = 16 * (k & 1);
                        ((uint32_t*)dst)[k] = ((row[k >> 1] >> sh) & 0xFFFFu) | ((row2[k >> 1] >> sh) << 16);
                    }
                    continue;
                }
            }
            if (pitch_m == 1 && !((uintptr_t)dst & 3)) {
                const int nd = cnt_m >> 1;
                if (lane < nd) ((uint32_t*)dst)[lane] = row[lane];
                if ((cnt_m & 1) && lane == nd) dst[cnt_m - 1] = (int16_t)(row[nd] & 0xFFFFu);
            } else {
                for (int k = lane; k < cnt_m; k += 64) dst[(long long)k * pitch_m] = (int16_t)((row[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
            }
        }
        if (more) stage_round<BITS>(in_lds, lane, buf);
        __syncthreads();
    }

    // a verify pass that met its old end state on the way leaves the chunk's end as it is
    if (active && running) {
        if (chunked) {
            job.chunk_end[item] = pack_state(p1, p2);
        } else {
            job.states[c].prev1 = p1;
            job.states[c].prev2 = p2;
        }
    }
}

__global__ void adpcm_decode_final_kernel(const int32_t* last_chunk, const unsigned long long* chunk_end, int n_chains,
                                          psxhip_adpcm_state_t* states) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= n_chains || last_chunk[c] < 0) return;
    const unsigned long long e = chunk_end[last_chunk[c]];
    states[c].prev1 = (int)(uint32_t)e;
    states[c].prev2 = (int)(uint32_t)(e >> 32);
}

// ---- sums of squared errors: one lane per unit, one chain per blockIdx.x, blockIdx.y strides over the chain's units
struct SseJob {
    const int16_t* a;
    const int16_t* b;
    const int16_t* a_tail;               // optional: 28 samples per chain, what the decoder computed for the unit sample_limit cuts
    const psxhip_adpcm_chain_t* chains;
    const int32_t* unit_base;            // needed with unit_sse only
    unsigned long long* unit_sse;        // optional: one sum per record index
    unsigned long long* chain_sums;      // optional: [n_chains][2] = sum (a - b)^2, sum b^2 (zero before the launch)
};

__device__ __forceinline__ void sse_add(int av, int bv, unsigned long long& e, unsigned long long& bb) {
    const int d = av - bv;
    const uint32_t ad = (uint32_t)(d < 0 ? -d : d);           // <= 65535: the square fits 32 bits
    e += ad * ad;
    bb += (uint32_t)(bv * bv);
}

// 64 units of a chain, one per lane.  With pitch 1 or 2 the wavefront first copies the stretch of memory those units span into LDS
// with coalesced dword loads (a lane reading "its" unit straight from memory touches 64 different lines per load, and with a few
// wavefronts per CU the lines leave the vector cache before their next sample is asked for: 63 ms for config 5 where the staged kernel
// takes 16), then every lane reads its samples there.  The stretch starts at the dword that holds the first sample; samples of
// the stretch outside the chain's own extent (in front of an odd start, behind sample_limit) are not touched.
constexpr int kSseStageSamples = 64 * 28 * 2 + 2;

__device__ __forceinline__ void sse_stage(const int16_t* chain0, long long first, long long extent, int span, uint32_t* lds, int lane,
                                          int& delta) {
    // chain0: the chain's sample 0; [first, first + span) memory samples of this block, of which those below `extent` are the chain's
    const int16_t* p = chain0 + first;
    delta = (int)(((uintptr_t)p >> 1) & 1);
    const uint32_t* p32 = (const uint32_t*)(p - delta);
    for (int d = lane; 2 * d < span + delta; d += 64) {
        const long long j0 = first + 2 * d - delta, j1 = j0 + 1;           // chain-local memory samples of the dword's halves
        const bool ok0 = 2 * d >= delta && j0 < extent, ok1 = j1 < extent;      // (the half in front of an odd start is not the block's)
        uint32_t v = 0;
        if (ok0 && ok1) v = p32[d];
        else if (ok0) v = (uint16_t)chain0[j0];
        else if (ok1) v = (uint32_t)(uint16_t)chain0[j1] << 16;
        lds[d] = v;
    }
}

__global__ __launch_bounds__(64) void adpcm_sse_kernel(const SseJob job) {
    __shared__ uint32_t lds_a[kSseStageSamples / 2 + 1], lds_b[kSseStageSamples / 2 + 1];
    const int c = (int)blockIdx.x, lane = (int)(threadIdx.x & 63);
    const psxhip_adpcm_chain_t ch = job.chains[c];
    const int limit = max(ch.sample_limit, 0);
    const int cut_unit = limit % 28 ? limit / 28 : -1;
    const int16_t* a = job.a + ch.sample_offset;
    const int16_t* b = job.b + ch.sample_offset;
    const bool staged = ch.pitch == 1 || ch.pitch == 2;
    const long long extent = limit ? (long long)(limit - 1) * ch.pitch + 1 : 0;      // memory samples from the chain's first to its last
    unsigned long long se = 0, sb = 0;
    for (long long u0 = (long long)blockIdx.y * 64; u0 < ch.n_units; u0 += (long long)gridDim.y * 64) {
        const long long u = u0 + lane;
        int da = 0, db = 0;
        if (staged) {
            __syncthreads();
            sse_stage(a, u0 * 28 * ch.pitch, extent, 64 * 28 * ch.pitch, lds_a, lane, da);
            sse_stage(b, u0 * 28 * ch.pitch, extent, 64 * 28 * ch.pitch, lds_b, lane, db);
            __syncthreads();
        }
        if (u < ch.n_units) {
        unsigned long long e = 0, bb = 0;
        const long long s0 = u * 28;
        const int16_t* la = (const int16_t*)lds_a + da + lane * 28 * ch.pitch;
        const int16_t* lb = (const int16_t*)lds_b + db + lane * 28 * ch.pitch;
#pragma unroll 4
        for (int k = 0; k < 28; k++) {
            int av = 0, bv = 0;
            if (s0 + k < limit) {
                av = staged ? la[k * ch.pitch] : a[(s0 + k) * ch.pitch];
                bv = staged ? lb[k * ch.pitch] : b[(s0 + k) * ch.pitch];
            } else if (job.a_tail && u == cut_unit) {
                av = job.a_tail[(size_t)c * 28 + k];
            }
            sse_add(av, bv, e, bb);
        }
        if (job.unit_sse) job.unit_sse[(long long)job.unit_base[c] + u * ch.unit_stride] = e;
        se += e;
        sb += bb;
        }
    }
    if (!job.chain_sums) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        se += __shfl_xor(se, off, 64);
        sb += __shfl_xor(sb, off, 64);
    }
    if (lane == 0) {
        if (se) atomicAdd(&job.chain_sums[2 * (size_t)c], se);
        if (sb) atomicAdd(&job.chain_sums[2 * (size_t)c + 1], sb);
    }
}

// ---- XA sectors -> unit records in encode order: the inverse of xa_assemble_kernel (adpcm_kernels.hip), one workgroup per sector
struct XaDisJob {
    const uint8_t* sectors;
    int n_sectors, format, stereo, frequency, bits;
    uint8_t* units;
    int32_t* status;        // optional
    uint32_t eof_edc_delta; // EDC of an all-zero span with 0x80 at sector bytes 18 and 22
};

__global__ __launch_bounds__(256) void xa_disassemble_kernel(const XaDisJob job) {
    __shared__ __attribute__((aligned(16))) uint8_t sec[2352];
    __shared__ uint32_t crc_tab[256];
    __shared__ int status;
    const int tid = (int)threadIdx.x;
    const int s = (int)blockIdx.x;
    const bool four = job.bits == 4;
    const int sector_size = job.format == 0 ? 2336 : 2352;
    const int lead = 2352 - sector_size;
    uint32_t* const sec32 = (uint32_t*)sec;

    crc_tab[tid] = c_xa_tables[tid];
    if (tid == 0) status = 0;
    if (tid < lead / 4) sec32[tid] = 0u;
    const uint32_t* src = (const uint32_t*)(job.sectors + (size_t)s * sector_size);
    for (int i = tid; i < sector_size / 4; i += 256) sec32[lead / 4 + i] = src[i];
    __syncthreads();

    int bad = 0;
    if (tid < 18) {
        // a sound group's header copies: bytes 4..7 against 0..3, 12..15 against 8..11 (adpcm.c:212-219)
        const uint32_t* grp = sec32 + (0x18 + tid * 128) / 4;
        if (grp[0] != grp[1] || grp[2] != grp[3]) bad |= 1;
    }
    if (tid >= 64 && tid < 128) {
        // one wavefront: subheaders, coding byte, the form-2 EDC over sector bytes 0x10 .. 0x92B (cdrom.c:102-110)
        const int l = tid - 64;
        const uint32_t sub0 = sec32[4], sub1 = sec32[5], stored = sec32[0x92C / 4];
        if (l == 0) {
            if (sub0 != sub1) bad |= 2;
            const uint32_t coding = (uint32_t)((job.stereo ? 0x01 : 0) | (job.frequency == 37800 ? 0 : 0x04) | (four ? 0 : 0x10));
            if ((sub0 >> 24) != coding) bad |= 4;
        }
        // psx_audio_xa_encode_finalize sets EOF in both subheaders behind the EDC and leaves the EDC as it was (adpcm.c:334-340):
        // such a sector carries the EDC of the sector without the bits.  The CRC is linear over GF(2): that is this sector's EDC xor
        // the EDC of a span that holds the two bits alone -- a constant (eof_edc_delta, from the host)
        const uint32_t edc = (uint32_t)__shfl((int)edc_wave<kEdcSpan>(sec32, crc_tab, l), 0, 64);
        const bool eof = (sub0 & sub1 & 0x00800000u) != 0u;
        const bool ok = stored == 0u || stored == edc || (eof && stored == (edc ^ job.eof_edc_delta));
        if (l == 0 && !ok) bad |= 8;
    }
    if (bad) atomicOr(&status, bad);

    // 18 sound groups of 128 bytes at sector byte 0x18; 576 record dwords per sector either way
    uint32_t* dst = (uint32_t*)job.units + (size_t)s * 576;
    for (int i = tid; i < 576; i += 256) {
        uint32_t v = 0;
        if (four) {
            // unit n of group g: header at group byte n (n < 4) or n + 4; sample w is nibble n & 1 of group byte 16 + 4 w + n / 2.  The
            // record is an SPU block: [header][0][14 code bytes: sample 2 k low, 2 k + 1 high]
            const int ui = i >> 2, q = i & 3, g = ui >> 3, n = ui & 7;
            const uint8_t* grp = sec + 0x18 + g * 128;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int rb = 4 * q + k;
                uint32_t byte = 0;
                if (rb == 0) byte = grp[n + (n >= 4 ? 4 : 0)];
                else if (rb >= 2) {
                    const int w = 2 * (rb - 2), sh = 4 * (n & 1);
                    byte = ((grp[16 + 4 * w + (n >> 1)] >> sh) & 15u) | (((grp[16 + 4 * (w + 1) + (n >> 1)] >> sh) & 15u) << 4);
                }
                v |= byte << (8 * k);
            }
        } else {
            // unit n of group g: header at group byte n; sample w at group byte 16 + 4 w + n.  Record: [header][0][0][0][28 codes]
            const int ui = i >> 3, q = i & 7, g = ui >> 2, n = ui & 3;
            const uint8_t* grp = sec + 0x18 + g * 128;
            if (q == 0) v = grp[n];
            else {
#pragma unroll
                for (int k = 0; k < 4; k++) v |= (uint32_t)grp[16 + 4 * (4 * (q - 1) + k) + n] << (8 * k);
            }
        }
        dst[i] = v;
    }
    __syncthreads();
    if (tid == 0 && job.status) job.status[s] = status;
}

bool bad_coding(int filter_count, int bits) {
    return (filter_count != 4 && filter_count != 5) || (bits != 4 && bits != 8) || (bits == 8 && filter_count == 5);
}

template <bool VERIFY>
void launch_decode(const DecodeJob& job, int bits, hipStream_t st) {
    const dim3 grid((unsigned)((job.n_items + 63) / 64)), block(64);
    if (bits == 4) hipLaunchKernelGGL((adpcm_decode_kernel<VERIFY, 4>), grid, block, 0, st, job);
    else hipLaunchKernelGGL((adpcm_decode_kernel<VERIFY, 8>), grid, block, 0, st, job);
}

}  // namespace

// measurement (psxhip_adpcm_decode_set_timing): the calling thread's switch and its last chunked call's two durations
static thread_local bool g_timing = false;
static thread_local float g_spec_ms = 0.f, g_verify_ms = 0.f;

extern "C" int psxhip_adpcm_decode_set_timing(int on) {
    g_timing = on != 0;
    return PSXHIP_OK;
}

extern "C" int psxhip_adpcm_decode_last_timing(float* speculate_ms, float* verify_ms) {
    if (speculate_ms) *speculate_ms = g_spec_ms;
    if (verify_ms) *verify_ms = g_verify_ms;
    return PSXHIP_OK;
}

extern "C" const char* psxhip_adpcm_decode_kernel_rev(void) { return PSXHIP_ADPCM_DECODE_KERNEL_REV; }

extern "C" int psxhip_adpcm_decode_chains_device(int device, const uint8_t* d_units, const psxhip_adpcm_chain_t* d_chains,
                                                 const int32_t* d_unit_base, int n_chains, int filter_count, int bits,
                                                 psxhip_adpcm_state_t* d_states, int16_t* d_samples, uint8_t* d_unit_flags, int16_t* d_tail,
                                                 void* stream) {
    if (n_chains < 0 || bad_coding(filter_count, bits) || (n_chains > 0 && (!d_units || !d_chains || !d_unit_base || !d_states || !d_samples)) ||
        ((uintptr_t)d_units & 15) || ((uintptr_t)d_samples & 1) || ((uintptr_t)d_tail & 3)) {
        psxhip_set_error("adpcm_decode_chains: bad argument (bits 4 or 8, filter_count 4 or 5 and 4 with 8 bits, d_units 16-byte aligned, d_tail 4-byte)");
        return PSXHIP_EINVAL;
    }
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_chains == 0) return PSXHIP_OK;
    DecodeJob job;
    memset(&job, 0, sizeof job);
    job.units = d_units; job.chains = d_chains; job.unit_base = d_unit_base; job.n_items = n_chains; job.filter_count = filter_count;
    job.states = d_states; job.samples = d_samples; job.unit_flags = d_unit_flags; job.tail = d_tail;
    launch_decode<false>(job, bits, (hipStream_t)stream);
    HIP_TRY(hipGetLastError(), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_adpcm_decode_chains_chunked(int device, const uint8_t* d_units, const psxhip_adpcm_chain_t* chains,
                                                  const int32_t* unit_base, int n_chains, int filter_count, int bits,
                                                  psxhip_adpcm_state_t* d_states, int16_t* d_samples, uint8_t* d_unit_flags, int16_t* d_tail,
                                                  int chunk_units, int warmup_units, int max_passes, void* stream) {
    if (n_chains < 0 || bad_coding(filter_count, bits) || (n_chains > 0 && (!d_units || !chains || !unit_base || !d_states || !d_samples)) ||
        ((uintptr_t)d_units & 15) || ((uintptr_t)d_samples & 1) || ((uintptr_t)d_tail & 3)) {
        psxhip_set_error("adpcm_decode_chains_chunked: bad argument (bits 4 or 8, filter_count 4 or 5 and 4 with 8 bits, d_units 16-byte aligned, d_tail 4-byte)");
        return PSXHIP_EINVAL;
    }
    long long total_units = 0;
    for (int c = 0; c < n_chains; c++) {
        if (chains[c].pitch < 1 || chains[c].n_units < 0) {
            psxhip_set_error("adpcm_decode_chains_chunked: chain %d has pitch %d, n_units %d", c, chains[c].pitch, chains[c].n_units);
            return PSXHIP_EINVAL;
        }
        total_units += chains[c].n_units;
    }
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (total_units == 0) return 0;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    if (chunk_units <= 0) {
        // the encoder's rule (pick_chunking) for wavefronts of 64 chunks: long chunks so that verify needs few passes, enough of them to
        // fill the device.  A decode wavefront holds 64 chunks and a CU eight such wavefronts: at least four rounds of them
        int w = 0, n_cu = 0;
        psxhip_adpcm_pick_chunking(total_units, 64, device, &chunk_units, &w);
        if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cu < 1) n_cu = 256;
        const long long fill = total_units / (4ll * 8 * 64 * n_cu);
        const long long want = fill < 256 ? 256 : fill;
        if (want < chunk_units) chunk_units = (int)want;
    }
    if (warmup_units < 0) warmup_units = 64;       // decoding is cheap: a long warm-up, not the encoder's

    // the chunk table: chain by chain, the two chains of an interleaved stereo pair chunk by chunk in turns
    std::vector<int32_t> chunk_chain, chunk_first, chunk_pred, last_chunk((size_t)n_chains, -1);
    for (int c = 0; c < n_chains;) {
        const bool pair = c + 1 < n_chains && chains[c].pitch == 2 && chains[c + 1].pitch == 2 && chains[c].n_units > 0 &&
                          chains[c + 1].sample_offset == chains[c].sample_offset + 1 && chains[c + 1].n_units == chains[c].n_units;
        const int span = pair ? 2 : 1;
        for (int f = 0; f < chains[c].n_units; f += chunk_units)
            for (int k = 0; k < span; k++) {
                const int32_t idx = (int32_t)chunk_chain.size();
                last_chunk[c + k] = idx;
                chunk_chain.push_back(c + k);
                chunk_first.push_back(f);
                chunk_pred.push_back(f ? idx - span : -1);
            }
        c += span;
    }
    const size_t n_chunks = chunk_chain.size();
    if (n_chunks > 0x7FFFFFFFu) {
        psxhip_set_error("adpcm_decode_chains_chunked: %zu chunks", n_chunks);
        return PSXHIP_EINVAL;
    }
    constexpr int kBatchMax = 16;
    BumpOffsets o;
    const size_t o_chains = o.take(sizeof(psxhip_adpcm_chain_t) * n_chains), o_base = o.take(4 * (size_t)n_chains), o_cc = o.take(4 * n_chunks);
    const size_t o_cf = o.take(4 * n_chunks), o_cp = o.take(4 * n_chunks), o_last = o.take(4 * (size_t)n_chains);
    const size_t o_used = o.take(8 * n_chunks), o_end = o.take(8 * n_chunks), o_flags = o.take(sizeof(int) * kBatchMax);
    DeviceBuffer ws;
    const int rc_ws = ws.reserve(o.end);
    if (rc_ws) return rc_ws;
    uint8_t* const d = ws.as<uint8_t>();
    hipStream_t st = (hipStream_t)stream;
    // declared after the workspace: on every way out the stream has come to rest before the workspace goes, and the timing events go too
    struct AtExit {
        hipStream_t st;
        bool at_rest;
        hipEvent_t ev[3];
        ~AtExit() {
            if (!at_rest) (void)hipStreamSynchronize(st);
            for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        }
    } at_exit{st, false, {nullptr, nullptr, nullptr}};
    hipEvent_t* const ev = at_exit.ev;
    int passes = 0, result = PSXHIP_OK;
    int h_flags[kBatchMax];
    HIP_TRY(hipMemcpyAsync(d + o_chains, chains, sizeof(psxhip_adpcm_chain_t) * n_chains, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + o_base, unit_base, 4 * (size_t)n_chains, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + o_cc, chunk_chain.data(), 4 * n_chunks, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + o_cf, chunk_first.data(), 4 * n_chunks, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + o_cp, chunk_pred.data(), 4 * n_chunks, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + o_last, last_chunk.data(), 4 * (size_t)n_chains, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    DecodeJob job;
    memset(&job, 0, sizeof job);
    job.units = d_units; job.chains = (const psxhip_adpcm_chain_t*)(d + o_chains); job.unit_base = (const int32_t*)(d + o_base);
    job.n_items = (int)n_chunks; job.filter_count = filter_count; job.states = d_states; job.samples = d_samples;
    job.unit_flags = d_unit_flags; job.tail = d_tail;
    job.chunk_chain = (const int32_t*)(d + o_cc); job.chunk_first = (const int32_t*)(d + o_cf);
    job.chunk_pred = (const int32_t*)(d + o_cp);
    job.chunk_units = chunk_units; job.warmup_units = warmup_units;
    job.start_used = (unsigned long long*)(d + o_used); job.chunk_end = (unsigned long long*)(d + o_end);
    int* d_flags = (int*)(d + o_flags);
    const bool timed = g_timing;
    if (timed)
        for (int i = 0; i < 3; i++) HIP_TRY(hipEventCreate(&ev[i]), PSXHIP_EDEVICE);
    if (timed) HIP_TRY(hipEventRecord(ev[0], st), PSXHIP_EDEVICE);
    launch_decode<false>(job, bits, st);
    HIP_TRY(hipGetLastError(), PSXHIP_EDEVICE);
    if (timed) HIP_TRY(hipEventRecord(ev[1], st), PSXHIP_EDEVICE);
    // verify passes in batches, back to back; a pass looks at its predecessor's word and returns at once when that changed nothing
    // (the encoder's scheme, psxhip_adpcm_session_run)
    int batch = 3;
    for (bool done = false; !done;) {
        if (max_passes > 0 && passes + batch > max_passes) batch = max_passes - passes;
        if (batch < 1) {
            psxhip_set_error("adpcm_decode_chains_chunked: not converged after %d verify passes", passes);
            result = PSXHIP_EINVAL;
            break;
        }
        HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(int) * kBatchMax, st), PSXHIP_EDEVICE);
        for (int i = 0; i < batch; i++) {
            job.changed = d_flags + i;
            job.changed_before = i ? d_flags + i - 1 : nullptr;
            launch_decode<true>(job, bits, st);
        }
        HIP_TRY(hipGetLastError(), PSXHIP_EDEVICE);
        HIP_TRY(hipMemcpyAsync(h_flags, d_flags, sizeof(int) * (size_t)batch, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
        HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
        for (int i = 0; i < batch && !done; i++) {
            passes++;
            if (!h_flags[i]) done = true;
        }
        batch = batch * 2 < kBatchMax ? batch * 2 : kBatchMax;
    }
    if (result == PSXHIP_OK) {
        hipLaunchKernelGGL(adpcm_decode_final_kernel, dim3((unsigned)((n_chains + 255) / 256)), dim3(256), 0, st,
                           (const int32_t*)(d + o_last), (const unsigned long long*)(d + o_end), n_chains, d_states);
        HIP_TRY(hipGetLastError(), PSXHIP_EDEVICE);
    }
    if (timed) {
        HIP_TRY(hipEventRecord(ev[2], st), PSXHIP_EDEVICE);
        HIP_TRY(hipEventSynchronize(ev[2]), PSXHIP_EDEVICE);
        HIP_TRY(hipEventElapsedTime(&g_spec_ms, ev[0], ev[1]), PSXHIP_EDEVICE);
        HIP_TRY(hipEventElapsedTime(&g_verify_ms, ev[1], ev[2]), PSXHIP_EDEVICE);
    }
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    at_exit.at_rest = true;
    return result == PSXHIP_OK ? passes : result;
}

extern "C" int psxhip_adpcm_sse_device(int device, const int16_t* d_a, const int16_t* d_a_tail, const int16_t* d_b,
                                       const psxhip_adpcm_chain_t* d_chains, int n_chains, uint64_t* d_unit_sse, const int32_t* d_unit_base,
                                       uint64_t* d_chain_sums, void* stream) {
    if (n_chains < 0 || (n_chains > 0 && (!d_a || !d_b || !d_chains || (d_unit_sse && !d_unit_base))) || ((uintptr_t)d_a & 1) ||
        ((uintptr_t)d_b & 1) || ((uintptr_t)d_a_tail & 1) || ((uintptr_t)d_unit_sse & 7) || ((uintptr_t)d_chain_sums & 7)) {
        psxhip_set_error("adpcm_sse: NULL or misaligned argument, negative chain count, or d_unit_sse without d_unit_base");
        return PSXHIP_EINVAL;
    }
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_chains == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    if (d_chain_sums) HIP_TRY(hipMemsetAsync(d_chain_sums, 0, (size_t)n_chains * 2 * sizeof(uint64_t), (hipStream_t)stream), PSXHIP_EDEVICE);
    SseJob job;
    job.a = d_a; job.b = d_b; job.a_tail = d_a_tail; job.chains = d_chains; job.unit_base = d_unit_base;
    job.unit_sse = (unsigned long long*)d_unit_sse; job.chain_sums = (unsigned long long*)d_chain_sums;
    // the host does not know the chains' lengths: enough slices that a few long chains fill the device, few enough that many short
    // chains do not launch mostly idle wavefronts
    int slices = 16384 / n_chains;
    slices = slices < 1 ? 1 : (slices > 1024 ? 1024 : slices);
    hipLaunchKernelGGL(adpcm_sse_kernel, dim3((unsigned)n_chains, (unsigned)slices), dim3(64), 0, (hipStream_t)stream, job);
    HIP_TRY(hipGetLastError(), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_xa_disassemble_device(int device, const uint8_t* d_sectors, int n_sectors, int format, int stereo, int frequency,
                                            int bits, uint8_t* d_units, int32_t* d_sector_status, void* stream) {
    if (n_sectors < 0 || (format != 0 && format != 1) || (bits != 4 && bits != 8) || (n_sectors > 0 && (!d_sectors || !d_units)) ||
        ((uintptr_t)d_sectors & 3) || ((uintptr_t)d_units & 3) || ((uintptr_t)d_sector_status & 3)) {
        psxhip_set_error("xa_disassemble: bad argument (format 0 or 1, bits 4 or 8, pointers 4-byte aligned)");
        return PSXHIP_EINVAL;
    }
    int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_sectors == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    if ((rc = xa_tables(device))) return rc;
    XaDisJob job;
    job.sectors = d_sectors; job.n_sectors = n_sectors; job.format = format; job.stereo = stereo; job.frequency = frequency; job.bits = bits;
    job.units = d_units; job.status = d_sector_status;
    static const uint32_t delta = [] {
        uint32_t t[256], c = 0;
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t v = i;
            for (int k = 0; k < 8; k++) v = (v >> 1) ^ ((v & 1u) ? 0xD8018001u : 0u);
            t[i] = v;
        }
        for (int i = 0; i < kEdcSpan; i++) c = (c >> 8) ^ t[(c ^ ((i == 2 || i == 6) ? 0x80u : 0u)) & 0xFF];
        return c;
    }();
    job.eof_edc_delta = delta;
    hipLaunchKernelGGL(xa_disassemble_kernel, dim3((unsigned)n_sectors), dim3(256), 0, (hipStream_t)stream, job);
    HIP_TRY(hipGetLastError(), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}
