// adpcm_beam_kernels.hip -- "psxhip ADPCM beam v1"  for MI355X (gfx950): the SPU / XA ADPCM search with a
// delayed decision inside the sound unit.  The arithmetic is adpcm_beam_core.h; the C ABI over these kernels is
// psxhip_adpcm_encode.cpp.
//
// Mapping.  As in adpcm_kernels.hip a chain owns a row of 16 lanes and lane c of the row owns candidate (filter c / 3, shift
// m - 1 + c % 3): four chains per wavefront, one wavefront per workgroup.  A lane keeps ALL of its candidate's slots -- up to four
// (e, p1, p2) -- in registers, so the 28 steps need no word from another lane: it makes its slots' <= 11 pool children, keeps the
// three smallest in a sorted list by insertion (strict <: the pool's order breaks ties) and writes one word of codes and one byte
// of parent slots per step to LDS words of its own.  The row agrees on the winner with a 16-lane minimum and a ballot, exactly as
// the plain encoder does; the winning lane alone walks its 28 kept decisions back, packs the record and stores it.
// The unit's 28 samples are staged in LDS (one broadcast read per step); __syncthreads orders the staging: a workgroup is one
// wavefront, so it is a wavefront-level ordering point and costs no barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adpcm_beam_core.h"
#include "psxhip_adpcm_internal.h"

namespace {

constexpr int kXsStride = 33;            // a row's staged samples: 28 + padding, rows in different LDS banks (see adpcm_kernels.hip)

struct BeamFetch {
    int a, b;
};

// lane c of a row fetches samples c and c + 16 of chain-local unit u.  Samples at chain index >= sample_limit read as zero without
// touching memory (adpcm.c:65,110).
__device__ __forceinline__ BeamFetch beam_fetch(const int16_t* src, const psxhip_adpcm_chain_t& ch, int u, bool live, int lane) {
    const int c = lane & 15;
    const long long limit = (long long)ch.sample_limit - (long long)u * 28;
    BeamFetch f;
    f.a = (live && c < limit) ? (int)src[((long long)u * 28 + c) * ch.pitch] : 0;
    f.b = (live && c + 16 < 28 && c + 16 < limit) ? (int)src[((long long)u * 28 + c + 16) * ch.pitch] : 0;
    return f;
}

// (every lane of the workgroup comes here: the callers' loops run to wavefront-wide bounds)
__device__ __forceinline__ void beam_stage(int* xs, const BeamFetch& f, int lane) {
    const int c = lane & 15;
    __syncthreads();            // the previous unit's readers are done
    xs[c] = f.a;
    xs[c + 16] = f.b;           // slots 28 .. 31 are padding
    __syncthreads();
}

__device__ __forceinline__ int beam_wave_max(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return __builtin_amdgcn_readfirstlane(v);       // a scalar: the loops it bounds branch without a saved exec mask
}

// One sound unit for the row this lane belongs to.  Returns true on the winning lane, which has stored the unit's record (and its
// error when unit_err is given); (prev1, prev2) advance to the winner's state when `unit_live`.
__device__ __forceinline__ bool beam_encode_unit_row(int filter_count, int range, int beam, const int* xs, bool unit_live, int lane, int& prev1,
                                                     int& prev2, uint32_t* codes_hist, uint8_t* parents_hist, uint8_t* units,
                                                     uint32_t* unit_err, long long index, bool store) {
    const int cand = lane & 15;
    const int filter = cand / 3, which = cand - filter * 3;
    const bool cand_live = filter < filter_count;
    const int f = cand_live ? filter : 0;
    const int m = beam_min_shift(xs, 1, prev1, prev2, f, range);
    const int shift = m - 1 + which;
    const bool valid = unit_live && cand_live && shift >= 0 && shift <= range;
    const int sh = valid ? shift : 0;

    int slot, np1, np2;
    const uint32_t e = beam_candidate(beam_cand(f, sh, range), beam, xs, 1, prev1, prev2, codes_hist + lane, parents_hist + lane, 64, slot, np1, np2);

    // the first strict minimum in (filter, shift) loop order (adpcm.c:158-183): a row's lanes are in that order.  Lanes without a
    // candidate carry 2^32 - 1; the candidate (filter 0, shift m) of a live unit never saturates, and a beam's result is at most
    // its anchor's
    const uint32_t mine = valid ? e : 0xFFFFFFFFu;
    uint32_t best = mine;
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)best, off, 16);
        best = o < best ? o : best;
    }
    const unsigned long long wmask = __ballot(valid && mine == best);
    const int wlane = (int)__builtin_ctzll(((wmask >> (lane & 48)) & 0xFFFFull) | 0x10000ull) + (lane & 48);
    const bool winner = valid && lane == wlane;
    const int w1 = __shfl(np1, wlane & 63, 64);
    const int w2 = __shfl(np2, wlane & 63, 64);
    if (unit_live) {
        prev1 = w1;
        prev2 = w2;
    }
    if (winner && store) {
        uint32_t pk[7];
        beam_trace_back(codes_hist + lane, parents_hist + lane, 64, slot, pk);
        const uint32_t header = (uint32_t)((sh & 0x0F) | (f << 4));
        if (range == 12) {          // (wave-uniform)
            uint32_t rec[4];
            beam_record4(header, pk, rec);
            uint4 v;
            v.x = rec[0]; v.y = rec[1]; v.z = rec[2]; v.w = rec[3];
            *(uint4*)(units + index * 16) = v;
        } else {
            uint32_t rec[8];
            beam_record8(header, pk, rec);
            uint32_t* out = (uint32_t*)(units + index * 32);
#pragma unroll
            for (int w = 0; w < 8; w++) out[w] = rec[w];
        }
        if (unit_err) unit_err[index] = e;
    }
    return winner;
}

// every chain serially, four chains per wavefront (the analogue of adpcm_chains_kernel)
__global__ __launch_bounds__(64) void adpcm_beam_chains_kernel(const psxhip_adpcm_beam_chain_job_t bj) {
    const psxhip_adpcm_chain_job_t& job = bj.job;
    const int lane = (int)(threadIdx.x & 63);
    const int chain = (int)blockIdx.x * 4 + (lane >> 4);
    const bool chain_live = chain < job.n_chains;

    psxhip_adpcm_chain_t ch;
    ch.sample_offset = 0; ch.pitch = 1; ch.sample_limit = 0; ch.n_units = 0; ch.unit_stride = 1;
    int prev1 = 0, prev2 = 0;
    long long rec0 = 0;
    // (the lane's own address, in vector registers from here to the last store: as a scalar base kept across the loop it was spilled)
    psxhip_adpcm_state_t* const my_state = job.states + (chain_live ? chain : 0);
    if (chain_live) {
        ch = job.chains[chain];
        prev1 = my_state->prev1;
        prev2 = my_state->prev2;
        rec0 = job.unit_base[chain];
    }
    // the four chains of a wavefront may have different lengths: iterate to the longest, mask the rest
    const int n_max = beam_wave_max(ch.n_units);

    const int16_t* src = job.samples + ch.sample_offset;
    __shared__ int xs_all[4][kXsStride];
    __shared__ uint32_t codes_hist[28 * 64];
    __shared__ uint8_t parents_hist[28 * 64];
    int* xs = xs_all[lane >> 4];

    // (no prefetch of the next unit's samples: a unit is some thousands of instructions, the load's latency one part in a hundred of it)
    for (int u = 0; u < n_max; u++) {
        const bool unit_live = u < ch.n_units;          // (a row without a chain has no units)
        beam_stage(xs, beam_fetch(src, ch, u, unit_live, lane), lane);
        (void)beam_encode_unit_row(job.filter_count, job.range, bj.beam, xs, unit_live, lane, prev1, prev2, codes_hist, parents_hist, job.units,
                                   bj.unit_err, rec0 + (long long)u * ch.unit_stride, true);
    }
    if (chain < job.n_chains && (lane & 15) == 0) {
        my_state->prev1 = prev1;
        my_state->prev2 = prev2;
    }
}

// Speculate-and-verify along time: the schedule of adpcm_chunks_kernel (adpcm_kernels.hip) with this file's unit
// encoder.  The scheme is right for any unit encoder that is a function of (prev1, prev2, 28 samples): at the fixpoint every chunk
// was encoded from its predecessor's final state.  Four chunks per wavefront.
template <bool VERIFY>
__global__ __launch_bounds__(64) void adpcm_beam_chunks_kernel(const psxhip_adpcm_beam_chunk_job_t bj) {
    const psxhip_adpcm_chunk_job_t& job = bj.job;
    // the passes behind the one that changed nothing fall through (the whole workgroup: no lane meets a barrier)
    if (VERIFY && job.changed_before && *job.changed_before == 0) return;
    const int lane = (int)(threadIdx.x & 63);
    const int row = lane >> 4, col = lane & 15;
    const int chunk = (int)blockIdx.x * 4 + row;
    const bool chunk_live = chunk < job.n_chunks;

    psxhip_adpcm_chain_t ch;
    ch.sample_offset = 0; ch.pitch = 1; ch.sample_limit = 0; ch.n_units = 0; ch.unit_stride = 1;
    int first = 0, count = 0, prev1 = 0, prev2 = 0, warm = 0;
    long long rec0 = 0, st0 = 0;
    bool active = false;
    if (chunk_live) {
        const int c = job.chunk_chain[chunk];
        ch = job.chains[c];
        first = job.chunk_first[chunk];
        count = min(job.chunk_units, ch.n_units - first);
        rec0 = job.unit_base[c];
        st0 = job.state_base[c];
        const int lead = job.lead_units[c];
        if (!VERIFY) {
            active = true;
            if (first == 0 && lead == 0) {
                prev1 = job.chain_states[c].prev1;
                prev2 = job.chain_states[c].prev2;
            } else {
                warm = min(job.warmup_units, first + lead);   // may reach back before the chain (negative unit index)
            }
        } else {
            const int used1 = job.start_used[chunk].prev1, used2 = job.start_used[chunk].prev2;
            int truth1 = used1, truth2 = used2;
            if (first > 0) {
                truth1 = job.unit_states[st0 + first - 1].prev1;
                truth2 = job.unit_states[st0 + first - 1].prev2;
            } else if (job.start_known[c]) {
                truth1 = job.chain_states[c].prev1;
                truth2 = job.chain_states[c].prev2;
            }
            if (truth1 != used1 || truth2 != used2) {
                active = true;
                prev1 = truth1;
                prev2 = truth2;
            }
        }
    }
    const int16_t* src = job.samples + ch.sample_offset;
    __shared__ int xs_all[4][kXsStride];
    __shared__ uint32_t codes_hist[28 * 64];
    __shared__ uint8_t parents_hist[28 * 64];
    int* xs = xs_all[row];

    // ---- warm-up (speculate only): advance the state from silence, keep nothing
    const int n_warm = active ? warm : 0;
    const int w_max = beam_wave_max(n_warm);
    for (int t = 0; t < w_max; t++) {
        const bool live = t < n_warm;
        beam_stage(xs, beam_fetch(src, ch, first - n_warm + t, live, lane), lane);
        (void)beam_encode_unit_row(job.filter_count, job.range, bj.beam, xs, live, lane, prev1, prev2, codes_hist, parents_hist, job.units, nullptr, 0, false);
    }
    // (the truth was read above by every lane of the row; it is replaced only behind the row's last read of it)
    if (chunk_live && col == 0 && (!VERIFY || active)) {
        psxhip_adpcm_state_t s0;
        s0.prev1 = prev1;
        s0.prev2 = prev2;
        job.start_used[chunk] = s0;
        if (VERIFY) *job.changed = 1;
    }

    // ---- the chunk itself
    const int n_run = active ? count : 0;
    const int n_max = beam_wave_max(n_run);
    bool running = active;
    for (int t = 0; t < n_max; t++) {
        const bool live = running && t < n_run;
        if (!__any(live)) break;
        const int u = first + t;
        psxhip_adpcm_state_t old;
        old.prev1 = 0;
        old.prev2 = 0;
        if (VERIFY && live) old = job.unit_states[st0 + u];
        beam_stage(xs, beam_fetch(src, ch, u, live, lane), lane);
        (void)beam_encode_unit_row(job.filter_count, job.range, bj.beam, xs, live, lane, prev1, prev2, codes_hist, parents_hist, job.units, bj.unit_err,
                                   rec0 + (long long)u * ch.unit_stride, true);
        // (verify) coincided with the state stored for this unit: everything after it is already consistent.  The record of THIS
        // unit may still differ (different start, same end), so it was written; the chunk stops here.  Every lane of the row has
        // read `old` before lane 0 replaces it below: the encode's shuffles lie in between.
        if (VERIFY && live && old.prev1 == prev1 && old.prev2 == prev2) running = false;
        if (live && col == 0) {
            psxhip_adpcm_state_t s1;
            s1.prev1 = prev1;
            s1.prev2 = prev2;
            job.unit_states[st0 + u] = s1;
        }
    }
}

}  // namespace

extern "C" hipError_t psxhip_adpcm_beam_chains_launch(const psxhip_adpcm_beam_chain_job_t* j, void* stream) {
    hipLaunchKernelGGL(adpcm_beam_chains_kernel, dim3((unsigned)((j->job.n_chains + 3) / 4)), dim3(64), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}

extern "C" hipError_t psxhip_adpcm_beam_chunks_launch(const psxhip_adpcm_beam_chunk_job_t* j, int verify, void* stream) {
    const dim3 grid((unsigned)((j->job.n_chunks + 3) / 4));
    if (verify) hipLaunchKernelGGL(adpcm_beam_chunks_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, *j);
    else hipLaunchKernelGGL(adpcm_beam_chunks_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}
