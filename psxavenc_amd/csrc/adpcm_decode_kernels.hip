// adpcm_decode_kernels.hip -- the ADPCM way back for MI355X (gfx950), hand-written HIP: unit records -> int16 PCM
// (adpcm_decode_kernel) and the sums of squared errors of two sample sets per unit and per chain (adpcm_sse_kernel); the entry points
// of include/psxav_hip.h that launch them are psxhip_adpcm_decode.cpp, XA sectors -> unit records sector_kernels.hip.  The arithmetic is
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

#include "adpcm_decode_core.h"
#include "psxhip_adpcm_internal.h"

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
__global__ __launch_bounds__(64) void adpcm_decode_kernel(const psxhip_adpcm_decode_job_t job) {
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

__global__ __launch_bounds__(64) void adpcm_sse_kernel(const psxhip_adpcm_sse_job_t job) {
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

}  // namespace

extern "C" hipError_t psxhip_adpcm_decode_launch(const psxhip_adpcm_decode_job_t* j, int verify, int bits, void* stream) {
    const dim3 grid((unsigned)((j->n_items + 63) / 64));
    hipStream_t st = (hipStream_t)stream;
    if (verify) {
        if (bits == 4) hipLaunchKernelGGL((adpcm_decode_kernel<true, 4>), grid, dim3(64), 0, st, *j);
        else hipLaunchKernelGGL((adpcm_decode_kernel<true, 8>), grid, dim3(64), 0, st, *j);
    } else {
        if (bits == 4) hipLaunchKernelGGL((adpcm_decode_kernel<false, 4>), grid, dim3(64), 0, st, *j);
        else hipLaunchKernelGGL((adpcm_decode_kernel<false, 8>), grid, dim3(64), 0, st, *j);
    }
    return hipGetLastError();
}

extern "C" hipError_t psxhip_adpcm_decode_final_launch(const int32_t* last_chunk, const unsigned long long* chunk_end, int n_chains,
                                                       psxhip_adpcm_state_t* states, void* stream) {
    hipLaunchKernelGGL(adpcm_decode_final_kernel, dim3((unsigned)((n_chains + 255) / 256)), dim3(256), 0, (hipStream_t)stream, last_chunk,
                       chunk_end, n_chains, states);
    return hipGetLastError();
}

extern "C" hipError_t psxhip_adpcm_sse_launch(const psxhip_adpcm_sse_job_t* j, int n_chains, int slices, void* stream) {
    hipLaunchKernelGGL(adpcm_sse_kernel, dim3((unsigned)n_chains, (unsigned)slices), dim3(64), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}
