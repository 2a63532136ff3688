// adpcm_kernels.hip -- SPU / XA ADPCM filter x shift search for MI355X (gfx950), hand-written HIP.
//
// Replaces libpsxav/adpcm.c:39-191 (find_min_shift, attempt_to_encode, encode) for batches of
// independent encoder chains, plus the SPU block packing (adpcm.c:367-372).  (The XA sound-group / sector assembly that reads
// the unit records is sector_kernels.hip; the C ABI over these kernels is psxhip_adpcm_encode.cpp.)
//
// A chain (one SPU stream, or one XA channel side) is serial in time: the two last DECODED samples
// feed the next sound unit (adpcm.c:135-136).  Inside one unit the reference tries, for each of the
// 4 (XA) or 5 (SPU) filters, the <=3 shifts around that filter's minimum shift and keeps the first
// strict minimum of the squared error in (filter, shift) loop order (adpcm.c:158-183).  Mapping:
//   * 16 lanes per chain = one DPP row; lane c of the row owns candidate (filter c/3, shift m-1+c%3);
//     4 chains per wavefront;
//   * every lane runs the 28-step predictor recursion for its own candidate in registers;
//   * the winner is a 16-lane DPP min-reduce on the packed key (sse << 8 | filter << 4 | shift),
//     which orders candidates exactly like the reference's loop + strict '<';
//   * the winning lane stores the unit's record and its decoded state is broadcast to the row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psxhip_adpcm_internal.h"

namespace {

// A sound unit's record.  8-bit codes (XA): 32 bytes -- [0] header, [4..31] the 28 codes.  4-bit codes (SPU, XA): 16 bytes IN THE
// LAYOUT OF AN SPU BLOCK (adpcm.c:367-372) -- [0] header, [1] 0, [2..15] the codes two to a byte (even sample low) -- half the bytes the
// encoders write and the sector assembly reads back (round 6; the records of a 4-bit job were 2.5 GB of config 5's 3.7 GB of writes).
constexpr int kRecordBytes = 32;
constexpr int kRecordBytes4 = 16;
__device__ __forceinline__ int record_bytes(int range) { return range == 12 ? kRecordBytes4 : kRecordBytes; }

// (k1 p1 + k2 p2 + 32) >> 6  (adpcm.c:63,106).  Taps and history fit 24 bits (|k| <= 122, history is int16): full-rate
// 24-bit multiply-adds, and the p2 product is off the recursion's critical path.
__device__ __forceinline__ int predict(int k1, int k2, int p1, int p2) {
    int t, r;
    asm("v_mad_i32_i24 %0, %1, %2, 32" : "=v"(t) : "v"(k2), "v"(p2));
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(k1), "v"(p1), "v"(t));
    return r >> 6;
}

// maximum over the wavefront (a few times per kernel: loop bounds of rows with different lengths)
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// A wavefront's 64 lanes are cut into ROWS of candidates, one chain per row.  SPU has 5 filters x 3 shifts = 15 candidates:
// 16-lane rows (= DPP rows), 4 chains per wavefront.  XA has 4 filters = 12 candidates: the time-parallel kernel packs
// 12-lane rows, 5 chains per wavefront (lanes 60..63 idle), a quarter more chains per instruction issued.
template <int ROW> __device__ __forceinline__ int row_of(int lane) { return ROW == 16 ? lane >> 4 : lane / 12; }
template <int ROW> __device__ __forceinline__ int col_of(int lane) { return ROW == 16 ? lane & 15 : lane - (lane / 12) * 12; }

// Per-lane constants of the candidate this lane owns inside its row.
struct Candidate {
    int f, which, k1, k2;
    int peer_a, peer_b;      // byte addresses (lane * 4) of the two other lanes that try this lane's filter
    int peer_f[3];           // 12-lane rows: the lanes with this lane's shift choice in the three other filters
    int row_base;            // first lane of this lane's row
    bool live;
    int range, qmin, qmax, qmask, half;
};

template <int ROW>
__device__ __forceinline__ Candidate make_candidate(int lane, int filter_count, int range) {
    Candidate c;
    const int cand = col_of<ROW>(lane);
    const int filter = cand / 3;
    c.which = cand - filter * 3;
    c.row_base = lane - cand;
    {
        const int group = lane - c.which;          // cand 15 (no filter) pairs with lanes past its row: it is never valid
        c.peer_a = ((group + (c.which + 1) % 3) & 63) * 4;
        c.peer_b = ((group + (c.which + 2) % 3) & 63) * 4;
        for (int k = 0; k < 3; k++) c.peer_f[k] = ((c.row_base + (cand + 3 * (k + 1)) % 12) & 63) * 4;
    }
    c.live = filter < filter_count;
    c.f = c.live ? filter : 0;
    // taps in 1/64 units (adpcm.c:36-37)
    c.k1 = c.f == 0 ? 0 : c.f == 1 ? 60 : c.f == 2 ? 115 : c.f == 3 ? 98 : 122;
    c.k2 = c.f == 0 ? 0 : c.f == 1 ? 0 : c.f == 2 ? -52 : c.f == 3 ? -55 : -60;
    c.range = range;
    c.qmin = -0x8000 >> range;
    c.qmax = 0x7FFF >> range;
    c.qmask = 0xFFFF >> range;
    c.half = 1 << (range - 1);
    return c;
}

// One sound unit for the 16-lane row this lane belongs to (adpcm.c:142-191 encode()): every lane tries its
// own (filter, shift) candidate on the row's 28 samples xs[] (staged in LDS: one broadcast read per step, so
// the recursion needs a handful of registers and 8 wavefronts fit a SIMD), the row agrees on the winner, and
// (prev1, prev2) advance to the winner's decoded state when `unit_live`.  Returns true on the winning lane,
// whose `header` and pk_lds[w * 64 + lane] (w = 0..6: four codes per word) then hold the unit's record.  The trial
// loop is kept rolled (codes parked in LDS) so that the whole encoder needs few registers.
// A row's staged samples: 28 + padding to 32 ints, rows 33 ints apart -- every lane of a row reads the same sample (a broadcast),
// the rows read different addresses, and at a stride of 32 ints rows 0, 2, 4 met in one LDS bank (PMC: five conflict cycles per LDS
// instruction of the speculating kernel); 33 puts the wavefront's rows into different banks for every sample index.
constexpr int kXsStride = 33;
template <int ROW, bool FLAT = false>
__device__ __forceinline__ bool encode_unit(const Candidate& cd, const int* xs, bool unit_live, int lane, int& prev1,
                                            int& prev2, uint32_t& header, uint32_t* pk_lds /* [7][64] per wavefront */) {
    // ---- find_min_shift for this lane's filter (adpcm.c:39-79): history continues with RAW samples, so only the first two
    //      residuals depend on the decoded state and the 28 samples can be split: the three lanes of a filter (one per
    //      candidate shift) take samples 0..9, 10..18 and 19..27 and share their extremes afterwards.
    int lo = 0, hi = 0;
    {
        const int i0 = cd.which == 0 ? 0 : (cd.which == 1 ? 10 : 19);
        int p1 = i0 ? xs[i0 - 1] : prev1, p2 = i0 ? xs[i0 - 2] : prev2;
#pragma unroll
        for (int t = 0; t < 10; t++) {
            const int xi = xs[i0 + t];             // (which == 2, t == 9 reads padding slot 28; that residual is not used)
            const int r = xi - predict(cd.k1, cd.k2, p1, p2);
            if (t < 9) {
                lo = r < lo ? r : lo;
                hi = r > hi ? r : hi;
            } else {
                lo = (cd.which == 0 && r < lo) ? r : lo;
                hi = (cd.which == 0 && r > hi) ? r : hi;
            }
            p2 = p1;
            p1 = xi;
        }
    }
    // the two while loops of adpcm.c:72-73 in closed form: hi >> rs <= qmax = 2^(15 - range) - 1 and lo >> rs >= qmin =
    // -2^(15 - range) both say "bit length of max(hi, ~lo) minus rs is at most 15 - range" (hi >= 0 >= lo), so
    // rs = clamp(bit_length(max(hi, ~lo)) - (15 - range), 0, range); tests/test_adpcm_oracle.py checks it against the loops.
    // (As loops they compiled to ~200 instructions of lane-divergent control flow per unit.)
    int widest = hi > ~lo ? hi : ~lo;
    {
        // ... of all three lanes of the filter
        const int a = __builtin_amdgcn_ds_bpermute(cd.peer_a, widest), b = __builtin_amdgcn_ds_bpermute(cd.peer_b, widest);
        widest = widest > a ? widest : a;
        widest = widest > b ? widest : b;
    }
    int rs = (widest > 0 ? 32 - __clz(widest) : 0) - (15 - cd.range);
    rs = rs < 0 ? 0 : (rs > cd.range ? cd.range : rs);
    const int m = cd.range - rs;
    const int shift = m - 1 + cd.which;
    const bool valid = unit_live && cd.live && shift >= 0 && shift <= cd.range;
    const int sh = valid ? shift : 0;

    // ---- attempt_to_encode for (filter, shift) (adpcm.c:81-140)
    // The squared error is summed in 32 bits with saturation: the candidate (filter 0, shift m) never clips -- its error is
    // at most one quantiser step, 2^12, per sample, 28 * 2^24 < 2^29 in total -- so the minimum is always below 2^32 and a
    // candidate that saturates cannot be it.  (A 64-bit multiply-add per sample costs four issue slots.)
    uint32_t sse = 0;
    int p1 = prev1, p2 = prev2;
    const int qmin_v = cd.qmin;
    const uint32_t up = (uint32_t)(cd.range - sh);
    const uint32_t mask4 = (uint32_t)cd.qmask * 0x01010101u;
    // (FLAT: the verify passes' instantiation -- a handful of wavefronts on an empty GPU, each the serial chase of a wrong start state:
    //  the trial loop unrolled, its 28 broadcast reads and stores off the recursion's chain; the speculating kernel keeps it rolled: there
    //  eight wavefronts share a SIMD and 64 registers each is what lets them)
    auto trial_word = [&](int w) {
        int qs[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int xi = xs[w * 4 + j];
            const int pred = predict(cd.k1, cd.k2, p1, p2);
            int q = (int)((uint32_t)(xi - pred) << sh);
            q = (q + cd.half) >> cd.range;
            asm("v_med3_i32 %0, %1, %2, %3" : "=v"(q) : "v"(q), "v"(qmin_v), "s"(cd.qmax));      // clamp to [qmin, qmax]
            // adpcm.c:118-123 masks the code to (16 - range) bits, shifts it to the top of an int16, sign-extends and shifts
            // right by `shift`.  For a clamped code that is q << range, exactly representable, and shift <= range: the decoded
            // step is q << (range - shift) -- one shift-add on the recursion's critical path instead of five operations.
            int dec;
            asm("v_lshl_add_u32 %0, %1, %2, %3" : "=v"(dec) : "v"(q), "v"(up), "v"(pred));
            dec = dec > 0x7FFF ? 0x7FFF : dec;
            dec = dec < -0x8000 ? -0x8000 : dec;
            const int err = dec - xi;                              // |err| <= 65535: the low 32 bits of the 24-bit product are its square
            sse = __builtin_elementwise_add_sat(sse, (uint32_t)__mul24(err, err));
            qs[j] = q;
            p2 = p1;
            p1 = dec;
        }
        // the codes are the low (16 - range) <= 8 bits of the clamped values: gather the four low bytes, mask once
        const uint32_t lo = __builtin_amdgcn_perm((uint32_t)qs[1], (uint32_t)qs[0], 0x0C0C0400u);
        const uint32_t hi = __builtin_amdgcn_perm((uint32_t)qs[3], (uint32_t)qs[2], 0x04000C0Cu);
        pk_lds[w * 64 + lane] = (lo | hi) & mask4;
    };
    if (FLAT) {
#pragma unroll
        for (int w = 0; w < 7; w++) trial_word(w);
    } else {
#pragma unroll 1
        for (int w = 0; w < 7; w++) trial_word(w);
    }

    // ---- first strict minimum in (filter, shift) loop order (adpcm.c:158-183).  A row's lanes ARE in that order (lane c owns filter
    //      c / 3, shift m - 1 + c % 3), so the winner is the row's first lane whose error equals the row's minimum: a 32-bit minimum
    //      and a ballot, where a 64-bit key (sse << 8 | filter << 4 | shift) took five 64-bit compare-and-select steps.  Lanes
    //      without a candidate carry 2^32 - 1; a live unit always has a candidate that does not saturate (above).
    const uint32_t mine = valid ? sse : 0xFFFFFFFFu;
    uint32_t best = mine;
    if (ROW == 16) {
        uint32_t o;
        o = (uint32_t)__builtin_amdgcn_update_dpp((int)best, (int)best, 0x128, 0xF, 0xF, false); best = o < best ? o : best;      // row_ror:8
        o = (uint32_t)__builtin_amdgcn_update_dpp((int)best, (int)best, 0x124, 0xF, 0xF, false); best = o < best ? o : best;      // row_ror:4
        o = (uint32_t)__builtin_amdgcn_update_dpp((int)best, (int)best, 0x122, 0xF, 0xF, false); best = o < best ? o : best;      // row_ror:2
        o = (uint32_t)__builtin_amdgcn_update_dpp((int)best, (int)best, 0x121, 0xF, 0xF, false); best = o < best ? o : best;      // row_ror:1
    } else {
        // 12-lane rows do not coincide with DPP rows: first the three lanes of a filter, then the four filters
        uint32_t o;
        o = (uint32_t)__builtin_amdgcn_ds_bpermute(cd.peer_a, (int)mine); best = o < best ? o : best;
        o = (uint32_t)__builtin_amdgcn_ds_bpermute(cd.peer_b, (int)mine); best = o < best ? o : best;
        const uint32_t filt = best;
#pragma unroll
        for (int k = 0; k < 3; k++) { o = (uint32_t)__builtin_amdgcn_ds_bpermute(cd.peer_f[k], (int)filt); best = o < best ? o : best; }
    }
    const uint64_t wmask = __ballot(valid && mine == best);
    const int wlane = ROW == 16 ? (int)__builtin_ctzll(((wmask >> (lane & 48)) & 0xFFFFull) | 0x10000ull) + (lane & 48)
                                : (int)__builtin_ctzll(((wmask >> cd.row_base) & 0xFFFull) | 0x1000ull) + cd.row_base;
    const bool winner = valid && lane == wlane;
    header = (uint32_t)((sh & 0x0F) | (cd.f << 4));
    const int np1 = __shfl(p1, wlane & 63, 64);
    const int np2 = __shfl(p2, wlane & 63, 64);
    if (unit_live) {
        prev1 = np1;
        prev2 = np2;
    }
    return winner;
}

// wave-level ordering point for LDS traffic between lanes of the same wavefront
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Stage the 28 samples of chain-local unit u of each of the wavefront's four rows into LDS (xs = this row's
// 32-int buffer): lane c of the row fetches samples c and c + 16.  Samples at chain index >= sample_limit read
// as zero without touching memory (adpcm.c:65,110).
struct UnitFetch {
    int a, b, c;
};
template <int ROW>
__device__ __forceinline__ UnitFetch fetch_unit(const int16_t* src, const psxhip_adpcm_chain_t& ch, int u, bool live, int lane) {
    const int c = col_of<ROW>(lane);
    const int limit = ch.sample_limit - u * 28;
    UnitFetch f;
    f.a = (live && c < limit) ? (int)src[(long long)(u * 28 + c) * ch.pitch] : 0;
    f.b = (live && c + ROW < 28 && c + ROW < limit) ? (int)src[(long long)(u * 28 + c + ROW) * ch.pitch] : 0;
    f.c = 0;
    if (ROW == 12) f.c = (live && c + 24 < 28 && c + 24 < limit) ? (int)src[(long long)(u * 28 + c + 24) * ch.pitch] : 0;
    return f;
}
template <int ROW>
__device__ __forceinline__ void stage_unit(int* xs, const UnitFetch& f, int lane) {
    const int c = col_of<ROW>(lane);
    wave_sync();            // the previous unit's readers are done
    xs[c] = f.a;
    if (ROW == 16) {
        xs[c + 16] = f.b;   // slots 28..31 are padding
    } else {
        xs[c + 12] = f.b;
        if (c < 8) xs[c + 24] = f.c;       // samples 24..27, padding 28..31
    }
    wave_sync();
}

// [header][flags = 0][14 x (even | odd << 4)]  (adpcm.c:367-372).  A word of pk_lds holds four codes, one per byte, each below 16:
// c | c >> 4 pairs them up in bytes 0 and 2, one byte permute takes those of two words.
__device__ __forceinline__ void store_spu_block(uint8_t* out, long long index, uint32_t header, const uint32_t* pk_lds, int lane) {
    uint32_t t[7];
#pragma unroll
    for (int w = 0; w < 7; w++) {
        const uint32_t c = pk_lds[w * 64 + lane];
        t[w] = c | (c >> 4);
    }
    uint4 v;
    v.x = __builtin_amdgcn_perm(t[0], header & 0xFFu, 0x06040C00u);      // header, 0, codes 0..3
    v.y = __builtin_amdgcn_perm(t[2], t[1], 0x06040200u);
    v.z = __builtin_amdgcn_perm(t[4], t[3], 0x06040200u);
    v.w = __builtin_amdgcn_perm(t[6], t[5], 0x06040200u);
    *(uint4*)(out + index * 16) = v;
}
__device__ __forceinline__ void store_record(uint8_t* units, long long index, uint32_t header, const uint32_t* pk_lds, int lane, int range) {
    if (range == 12) {          // (wave-uniform)
        store_spu_block(units, index, header, pk_lds, lane);
        return;
    }
    uint32_t* rec = (uint32_t*)(units + index * kRecordBytes);
    rec[0] = header;
#pragma unroll
    for (int w = 0; w < 7; w++) rec[1 + w] = pk_lds[w * 64 + lane];
}

__global__ __launch_bounds__(64, 8) void adpcm_chains_kernel(const psxhip_adpcm_chain_job_t job) {
    const int lane = (int)(threadIdx.x & 63);
    const int chain = (int)blockIdx.x * 4 + (lane >> 4);
    const bool chain_live = chain < job.n_chains;
    const Candidate cd = make_candidate<16>(lane, job.filter_count, job.range);

    psxhip_adpcm_chain_t ch;
    ch.sample_offset = 0; ch.pitch = 1; ch.sample_limit = 0; ch.n_units = 0; ch.unit_stride = 1;
    int prev1 = 0, prev2 = 0;
    long long rec0 = 0;
    if (chain_live) {
        ch = job.chains[chain];
        prev1 = job.states[chain].prev1;
        prev2 = job.states[chain].prev2;
        rec0 = job.unit_base[chain];
    }
    // the four chains of a wavefront may have different lengths: iterate to the longest, mask the rest
    int n_max = ch.n_units;
    n_max = max(n_max, __shfl_xor(n_max, 16, 64));
    n_max = max(n_max, __shfl_xor(n_max, 32, 64));

    const int16_t* src = job.samples + ch.sample_offset;
    __shared__ int xs_all[4][kXsStride];
    __shared__ uint32_t pk_lds[7 * 64];
    int* xs = xs_all[lane >> 4];

    UnitFetch nxt = fetch_unit<16>(src, ch, 0, chain_live && 0 < ch.n_units, lane);
    for (int u = 0; u < n_max; u++) {
        const bool unit_live = chain_live && u < ch.n_units;
        stage_unit<16>(xs, nxt, lane);
        if (u + 1 < n_max) nxt = fetch_unit<16>(src, ch, u + 1, chain_live && u + 1 < ch.n_units, lane);   // prefetch
        uint32_t header;
        if (encode_unit<16>(cd, xs, unit_live, lane, prev1, prev2, header, pk_lds))
            store_record(job.units, rec0 + (long long)u * ch.unit_stride, header, pk_lds, lane, job.range);
    }
    if (chain_live && (lane & 15) == 0) {
        job.states[chain].prev1 = prev1;
        job.states[chain].prev2 = prev2;
    }
}

// ---------------------------------------------------------------------------------------------
// The reference's own call pattern -- psx_audio_spu_encode once per 28 samples (filefmt.c:243), psx_audio_xa_encode once per
// sector (filefmt.c:184) -- as ONE launch with nothing to copy around it: chain descriptors and start states ride in the
// kernel arguments, the samples are read from page-locked host memory the device can see (staged into LDS first: one PCIe
// round trip, then the serial chain runs out of LDS), SPU blocks leave packed (adpcm.c:367-372) straight into page-locked host
// memory, final states likewise.  One wavefront, up to four chains.  (The batched path's four H2D copies, two kernels, two D2H
// copies and a synchronise cost 94 us per 28-sample call against ~3 us for the reference's own loop.)
// ---------------------------------------------------------------------------------------------
constexpr int kCallStageMax = PSXHIP_ADPCM_CALL_STAGE_MAX;
constexpr int kCallWarm = 8;             // units a speculating row runs from a zero state before its segment
constexpr int kCallSpecMin = 24;         // chains shorter than this are encoded serially (nothing to win)
constexpr int kCallHist = 96;            // longest speculated segment

__global__ __launch_bounds__(64) void adpcm_call_kernel(const psxhip_adpcm_call_job_t job) {
    const int lane = (int)(threadIdx.x & 63);
    const Candidate cd = make_candidate<16>(lane, job.filter_count, job.range);
    __shared__ __attribute__((aligned(16))) int16_t stage[kCallStageMax];
    __shared__ int xs_all[4][kXsStride];
    __shared__ uint32_t pk_lds[7 * 64];

    const int16_t* base = job.samples;
    if (job.stage_elems > 0) {
        // all loads of a round in flight before the first is waited for (the source is on the far side of the PCIe link)
        const uint4* src16 = (const uint4*)job.samples;
        uint4* dst16 = (uint4*)stage;
        const int n16 = job.stage_elems >> 3;
        for (int i0 = 0; i0 < n16; i0 += 64 * 8) {
            uint4 v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = i0 + k * 64 + lane;
                v[k] = i < n16 ? src16[i] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = i0 + k * 64 + lane;
                if (i < n16) dst16[i] = v[k];
            }
        }
        __syncthreads();
        base = stage;
    }
    // ---- rows.  A wavefront has four rows; a call has 1-4 chains.  With one or two chains of some length the spare rows
    //      SPECULATE (the scheme of adpcm_chunks_kernel inside one wavefront): a chain is cut into 4 / n_chains segments; segment 0
    //      starts from the chain's true state, every other segment from a state guessed by running kCallWarm units before it
    //      from zero, and keeps the state after each of its units.  Then the row that holds the truth (the "runner": segment 0's)
    //      walks the boundaries: a segment whose guess was the truth stands; otherwise the runner re-encodes it from the truth
    //      until its state coincides with the kept one -- from there on the segment stands as well (the unit encoder is a
    //      function of state and samples).  Worst case (states never coincide: pure tones) the runner re-encodes everything, i.e.
    //      the serial schedule; typical material falls in within a few units, and a sector's 72 units per channel take 40 + a
    //      few dependent unit encodes instead of 72.  The result is the serial encode's, bit for bit, whatever the guesses.
    const int nc = job.n_chains;
    const int nu = job.chains[0].n_units;
    int nseg = nc == 1 ? 4 : (nc == 2 ? 2 : 1);
    for (int c = 1; c < nc; c++)
        if (job.chains[c].n_units != nu) nseg = 1;
    if (nu < kCallSpecMin) nseg = 1;
    int L0 = nu, Lr = 0;
    if (nseg > 1) {
        L0 = (nu + (nseg - 1) * kCallWarm + nseg - 1) / nseg;
        Lr = (nu - L0 + nseg - 2) / (nseg - 1);
        if (Lr > kCallHist || Lr < 1) { nseg = 1; L0 = nu; Lr = 0; }
    }
    const int row = lane >> 4, col = lane & 15;
    const int seg = row / nc, c_of_row = row - seg * nc;           // (nc >= 1)
    const bool row_live = row < nseg * nc;
    const int seg_s = seg == 0 ? 0 : min(nu, L0 + (seg - 1) * Lr);
    int seg_e = seg == 0 ? L0 : min(nu, seg_s + Lr);
    __shared__ int2 hist[4][kCallHist];       // state after each unit of a speculated segment
    __shared__ int2 guess[4];                 // state a speculated segment started from

    psxhip_adpcm_chain_t ch;
    ch.sample_offset = 0; ch.pitch = 1; ch.sample_limit = 0; ch.n_units = 0; ch.unit_stride = 1;
    int prev1 = 0, prev2 = 0;
    long long rec0 = 0;
#pragma unroll
    for (int c = 0; c < 4; c++)
        if (c_of_row == c && row_live) {
            ch = job.chains[c];
            rec0 = job.unit_base[c];
            if (seg == 0) {
                prev1 = job.states_in[c].prev1;
                prev2 = job.states_in[c].prev2;
            }
        }
    const int16_t* src = base + ch.sample_offset;
    if (nseg == 1 && row_live) seg_e = ch.n_units;       // no speculation: every row is a whole chain, of its OWN length (chains of one call may differ)
    int* xs = xs_all[row];
    auto put = [&](int u, uint32_t header) {
        if (job.spu_out) store_spu_block(job.spu_out, rec0 + (long long)u * ch.unit_stride, header, pk_lds, lane);
        else store_record(job.units, rec0 + (long long)u * ch.unit_stride, header, pk_lds, lane, job.range);
    };
    // ---- phase 1: every row its segment (the speculating rows start kCallWarm units early, from a zero state)
    const int u0 = seg == 0 ? 0 : seg_s - kCallWarm;               // (L0 >= kCallWarm: never negative)
    int t_max = row_live ? seg_e - u0 : 0;
    t_max = max(t_max, __shfl_xor(t_max, 16, 64));
    t_max = max(t_max, __shfl_xor(t_max, 32, 64));
    UnitFetch nxt = fetch_unit<16>(src, ch, u0, row_live && u0 < seg_e, lane);
    for (int t = 0; t < t_max; t++) {
        const int u = u0 + t;
        const bool unit_live = row_live && u < seg_e;
        stage_unit<16>(xs, nxt, lane);
        if (t + 1 < t_max) nxt = fetch_unit<16>(src, ch, u + 1, row_live && u + 1 < seg_e, lane);
        if (unit_live && col == 0 && seg > 0 && u == seg_s) guess[row] = make_int2(prev1, prev2);
        uint32_t header;
        const bool won = encode_unit<16>(cd, xs, unit_live, lane, prev1, prev2, header, pk_lds);
        if (won && unit_live && u >= seg_s) put(u, header);
        if (unit_live && col == 0 && seg > 0 && u >= seg_s) hist[row][u - seg_s] = make_int2(prev1, prev2);
    }
    wave_sync();
    // ---- phase 2: the runners (segment 0's rows) walk their chains' boundaries
    if (nseg > 1) {
        const bool runner = row < nc;
        int b = 1, u = 0;
        bool reenc = false;
        for (;;) {
            if (runner) {
                while (!reenc && b < nseg) {
                    const int rb = b * nc + row;
                    const int sb = min(nu, L0 + (b - 1) * Lr), eb = min(nu, sb + Lr);
                    if (sb >= eb) { b = nseg; break; }
                    const int2 g = guess[rb];
                    if (g.x == prev1 && g.y == prev2) {            // the guess was the truth: the segment stands
                        const int2 h = hist[rb][eb - sb - 1];
                        prev1 = h.x; prev2 = h.y;
                        b++;
                    } else {
                        reenc = true;
                        u = sb;
                    }
                }
            }
            const bool work = runner && reenc;
            if (__ballot(work) == 0) break;
            const UnitFetch f = fetch_unit<16>(src, ch, u, work, lane);
            stage_unit<16>(xs, f, lane);
            uint32_t header;
            const bool won = encode_unit<16>(cd, xs, work, lane, prev1, prev2, header, pk_lds);
            if (won && work) put(u, header);
            if (work) {
                const int rb = b * nc + row;
                const int sb = min(nu, L0 + (b - 1) * Lr), eb = min(nu, sb + Lr);
                const int2 h = hist[rb][u - sb];
                u++;
                if (h.x == prev1 && h.y == prev2) {                // fell into the speculated trajectory: the rest of the segment stands
                    const int2 hl = hist[rb][eb - sb - 1];
                    prev1 = hl.x; prev2 = hl.y;
                    reenc = false;
                    b++;
                } else if (u == eb) {                              // re-encoded to its end: this IS the truth at the next boundary
                    reenc = false;
                    b++;
                }
            }
        }
    }
    if (row < nc && col == 0) {
        job.states_out[row].prev1 = prev1;
        job.states_out[row].prev2 = prev2;
    }
}

// ---------------------------------------------------------------------------------------------
// Speculate-and-verify along time.  A chain is serial, but its whole carried state is the
// pair (prev1, prev2), and encoders started from different states on the same samples usually fall into
// the same state within a few units.  So a long chain is cut into chunks of `chunk_units`:
//   speculate: every chunk is encoded in parallel, its start state guessed by running `warmup_units`
//              units before the chunk from a zero state (chunk 0 starts from the chain's true state);
//              the state after every unit is kept;
//   verify:    every chunk compares the state it started from with the state its predecessor actually
//              ended in; on a mismatch it re-encodes forward from the true state until its new state
//              coincides with the stored one (from there on the stored records are already right).
// verify is repeated until a pass changes nothing.  At that fixpoint every chunk was encoded from its
// predecessor's final state by the deterministic unit encoder, i.e. the result equals the serial encode,
// bit for bit, whatever the guesses were.  Worst case (states never coincide, e.g. pure tones) verify
// advances one chunk per pass, which is the serial schedule.
// ---------------------------------------------------------------------------------------------

template <bool VERIFY, int ROW>
__global__ __launch_bounds__(64, VERIFY ? 4 : 8) void adpcm_chunks_kernel(const psxhip_adpcm_chunk_job_t job) {
    constexpr int kRows = 64 / ROW;            // chains per wavefront: 4 or 5
    // Verify passes are launched several at a time, back to back, without a host round trip in between (a synchronise + launch
    // per pass was 40-50 us, as much as re-encoding 40 sound units); the passes after the one that changed nothing fall through here
    if (VERIFY && job.changed_before && *job.changed_before == 0) return;
    const int lane = (int)(threadIdx.x & 63);
    const int row = row_of<ROW>(lane), col = col_of<ROW>(lane);
    const int chunk = (int)blockIdx.x * kRows + row;
    const bool chunk_live = row < kRows && chunk < job.n_chunks;
    const Candidate cd = make_candidate<ROW>(lane, job.filter_count, job.range);

    psxhip_adpcm_chain_t ch;
    ch.sample_offset = 0; ch.pitch = 1; ch.sample_limit = 0; ch.n_units = 0; ch.unit_stride = 1;
    int first = 0, count = 0, prev1 = 0, prev2 = 0, warm = 0;
    bool active = false;
    if (chunk_live) {
        const int c = job.chunk_chain[chunk];
        ch = job.chains[c];
        first = job.chunk_first[chunk];
        count = min(job.chunk_units, ch.n_units - first);
        const long long st0 = job.state_base[c];          // (the chunk loop's copy is fetched behind the warm-up: see there)
        const int lead = job.lead_units[c];
        if (!VERIFY) {
            active = true;
            if (first == 0 && lead == 0) {
                prev1 = job.chain_states[c].prev1;
                prev2 = job.chain_states[c].prev2;
            } else {
                warm = min(job.warmup_units, first + lead);   // may reach back before the chain (negative unit index)
                // The warm-up starts from silence.  Starting from the two raw samples in front of it is a kept negative: it does not
                // converge sooner (oracle/cpu_bench converge, profiles/r05_adpcm_convergence.txt).
            }
        } else {
            // (scalars, not structs: a conditional between two loaded structs went through a stack slot -- 12 bytes of scratch per
            //  lane that nothing ever read back)
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
                if (col == 0) {
                    job.start_used[chunk].prev1 = truth1;
                    job.start_used[chunk].prev2 = truth2;
                    *job.changed = 1;
                }
            }
        }
    }
    const int16_t* src = job.samples + ch.sample_offset;

    // ---- warm-up (speculate only): advance the state, keep nothing
    int n_warm = active ? warm : 0;
    int w_max = n_warm;
    w_max = wave_max(w_max);
    __shared__ int xs_all[64 / ROW + 1][kXsStride];
    __shared__ uint32_t pk_lds[7 * 64];
    int* xs = xs_all[row];
    for (int t = 0; t < w_max; t++) {
        const bool live = t < n_warm;
        stage_unit<ROW>(xs, fetch_unit<ROW>(src, ch, first - n_warm + t, live, lane), lane);
        uint32_t header;
        (void)encode_unit<ROW>(cd, xs, live, lane, prev1, prev2, header, pk_lds);
    }
    if (!VERIFY && chunk_live && col == 0) {
        psxhip_adpcm_state_t s0;
        s0.prev1 = prev1;
        s0.prev2 = prev2;
        job.start_used[chunk] = s0;
    }

    // ---- the chunk itself
    // (where its records and states go is fetched here, not in front of the warm-up: two 64-bit values a lane would carry through
    //  the warm-up loop for nothing -- at 8 wavefronts per SIMD, 64 registers, they were its scratch spill)
    long long rec0 = 0, st0 = 0;
    if (chunk_live) {
        const int c = job.chunk_chain[chunk];
        rec0 = job.unit_base[c];
        st0 = job.state_base[c];
    }
    int n_run = active ? count : 0;
    int n_max = n_run;
    n_max = wave_max(n_max);
    // Software pipeline: while unit t is encoded, the samples of unit t + 1 and (verify) the state stored for it are on
    // their way; they are staged into the other LDS buffer right after the encode -- by then they have arrived and nothing
    // younger is in flight -- and only then this unit's record and state are stored.  The loop never waits for a store.
    // (Loading the stored state where it is compared cost two exposed global round trips per unit: 2.3 us instead of 1.)
    bool running = active;
    __shared__ int xs_alt[64 / ROW + 1][kXsStride];
    int* xs_a = xs;
    int* xs_b = xs_alt[row];
    UnitFetch nxt = fetch_unit<ROW>(src, ch, first, running && 0 < n_run, lane);
    psxhip_adpcm_state_t old_nxt;
    old_nxt.prev1 = 0;
    old_nxt.prev2 = 0;
    if (VERIFY && running && 0 < n_run) old_nxt = job.unit_states[st0 + first];
    stage_unit<ROW>(xs_a, nxt, lane);
    for (int t = 0; t < n_max; t++) {
        const bool live = running && t < n_run;
        if (!__any(live)) break;
        const int u = first + t;
        const psxhip_adpcm_state_t old = old_nxt;
        const bool more = t + 1 < n_max;
        if (more) {
            const bool nlive = running && t + 1 < n_run;
            nxt = fetch_unit<ROW>(src, ch, u + 1, nlive, lane);
            if (VERIFY && nlive) old_nxt = job.unit_states[st0 + u + 1];
        }
        uint32_t header;
        const bool winner = encode_unit<ROW, VERIFY>(cd, xs_a, live, lane, prev1, prev2, header, pk_lds);
        // (verify) coincided with the state stored for this unit: everything after it is already consistent.  The record of
        // THIS unit may still differ (different start, same end), so it is written, then the chunk stops.
        if (VERIFY && live && old.prev1 == prev1 && old.prev2 == prev2) running = false;
        if (more) stage_unit<ROW>(xs_b, nxt, lane);
        if (winner) store_record(job.units, rec0 + (long long)u * ch.unit_stride, header, pk_lds, lane, job.range);
        if (live && col == 0) {
            psxhip_adpcm_state_t s1;
            s1.prev1 = prev1;
            s1.prev2 = prev2;
            job.unit_states[st0 + u] = s1;
        }
        int* const swap = xs_a;
        xs_a = xs_b;
        xs_b = swap;
    }
}

// ---- SPU block packing (adpcm.c:367-372): [header][flags = 0][14 x (even | odd << 4)]
__global__ void spu_pack_kernel(const uint8_t* units, int n_blocks, uint8_t* out) {
    // (a 4-bit record IS the block: a copy, kept as the place where the two layouts would part again)
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= n_blocks) return;
    *(uint4*)(out + (size_t)b * 16) = *(const uint4*)(units + (size_t)b * kRecordBytes4);
}

}  // namespace

// final state of every chain = state after its last unit
__global__ void adpcm_gather_final_states_kernel(const psxhip_adpcm_chain_t* chains, const int64_t* state_base, int n_chains,
                                                 const psxhip_adpcm_state_t* unit_states, psxhip_adpcm_state_t* states) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= n_chains) return;
    const int n = chains[c].n_units;
    if (n > 0) states[c] = unit_states[state_base[c] + n - 1];
}

extern "C" hipError_t psxhip_adpcm_chains_launch(const psxhip_adpcm_chain_job_t* j, void* stream) {
    hipLaunchKernelGGL(adpcm_chains_kernel, dim3((unsigned)((j->n_chains + 3) / 4)), dim3(64), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}

extern "C" hipError_t psxhip_adpcm_call_launch(const psxhip_adpcm_call_job_t* j, void* stream) {
    hipLaunchKernelGGL(adpcm_call_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}

extern "C" hipError_t psxhip_adpcm_chunks_launch(const psxhip_adpcm_chunk_job_t* j, int verify, void* stream) {
    // XA's 4 filters fill 12 of a row's lanes: 12-lane rows, five chunks per wavefront; SPU's 5 filters need 16-lane rows
    const bool narrow = j->filter_count == 4;
    const int per = narrow ? 5 : 4;
    const auto kernel = verify ? (narrow ? adpcm_chunks_kernel<true, 12> : adpcm_chunks_kernel<true, 16>)
                               : (narrow ? adpcm_chunks_kernel<false, 12> : adpcm_chunks_kernel<false, 16>);
    void* args[] = {(void*)j};
    return hipLaunchKernel((const void*)kernel, dim3((unsigned)((j->n_chunks + per - 1) / per)), dim3(64), args, 0, (hipStream_t)stream);
}

extern "C" hipError_t psxhip_adpcm_final_states_launch(const psxhip_adpcm_chain_t* chains, const int64_t* state_base, int n_chains,
                                                       const psxhip_adpcm_state_t* unit_states, psxhip_adpcm_state_t* states, void* stream) {
    hipLaunchKernelGGL(adpcm_gather_final_states_kernel, dim3((unsigned)((n_chains + 255) / 256)), dim3(256), 0, (hipStream_t)stream, chains,
                       state_base, n_chains, unit_states, states);
    return hipGetLastError();
}

extern "C" hipError_t psxhip_spu_pack_launch(const uint8_t* units, int n_blocks, uint8_t* out, void* stream) {
    hipLaunchKernelGGL(spu_pack_kernel, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, units, n_blocks, out);
    return hipGetLastError();
}
