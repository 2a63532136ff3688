// adpcm_kernels.hip -- SPU / XA ADPCM filter x shift search for MI355X (gfx950), hand-written HIP.
//
// Replaces libpsxav/adpcm.c:39-191 (find_min_shift, attempt_to_encode, encode) for batches of
// independent encoder chains, plus the SPU block packing (adpcm.c:367-372) and the XA sound-group /
// sector assembly with its EDC (adpcm.c:193-233,266-332; cdrom.c:28-41,55-74,102-110).
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
#include <string.h>

#include <mutex>
#include <vector>

#include "psxhip_internal.h"
#include "xa_edc.h"

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

struct ChainJob {
    const int16_t* samples;
    const psxhip_adpcm_chain_t* chains;
    const int32_t* unit_base;
    int n_chains;
    int filter_count;   // 5 SPU, 4 XA
    int range;          // 12 (4-bit) or 8 (8-bit)
    psxhip_adpcm_state_t* states;
    uint8_t* units;
};

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

__global__ __launch_bounds__(64, 8) void adpcm_chains_kernel(const ChainJob job) {
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
constexpr int kCallStageMax = 8192;      // int16 elements staged in LDS (an XA sector is 4032)
constexpr int kCallWarm = 8;             // units a speculating row runs from a zero state before its segment
constexpr int kCallSpecMin = 24;         // chains shorter than this are encoded serially (nothing to win)
constexpr int kCallHist = 96;            // longest speculated segment
struct CallJob {
    const int16_t* samples;                 // device-visible; chains' sample_offset counts from here
    psxhip_adpcm_chain_t chains[4];
    psxhip_adpcm_state_t states_in[4];
    int32_t unit_base[4];
    int n_chains, filter_count, range;
    int stage_elems;                        // > 0: copy this many elements into LDS first (multiple of 8, <= kCallStageMax)
    psxhip_adpcm_state_t* states_out;
    uint8_t* units;                         // 32-byte records (XA), or NULL
    uint8_t* spu_out;                       // packed 16-byte SPU blocks, or NULL
};

__global__ __launch_bounds__(64) void adpcm_call_kernel(const CallJob job) {
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
struct ChunkJob {
    const int16_t* samples;
    const psxhip_adpcm_chain_t* chains;
    const int32_t* unit_base;        // record index of each chain's unit 0
    const int64_t* state_base;       // index into unit_states of each chain's unit 0
    const int32_t* chunk_chain;      // [n_chunks] chain of each chunk
    const int32_t* chunk_first;      // [n_chunks] first unit (chain-local) of each chunk
    int n_chunks, chunk_units, warmup_units;
    int filter_count, range;
    const psxhip_adpcm_state_t* chain_states;   // start state of every chain (the truth as far as it is known)
    const int32_t* lead_units;                  // [n_chains] units available BEFORE the chain's first unit for guessing
                                                //            its start state (0: start from chain_states as given)
    const uint8_t* start_known;                 // [n_chains] 0: chain_states[c] is not known yet, keep the guess
    psxhip_adpcm_state_t* unit_states;          // state after every unit
    psxhip_adpcm_state_t* start_used;           // [n_chunks] state each chunk was last encoded from
    uint8_t* units;
    int* changed;                    // verify: set to 1 when any chunk had to be re-encoded (device memory, one word per pass)
    const int* changed_before;       // verify: the previous pass's word, NULL for the first pass of a batch -- a pass whose
                                     // predecessor changed nothing has nothing to do (the fixpoint was reached) and returns at once
};

template <bool VERIFY, int ROW>
__global__ __launch_bounds__(64, VERIFY ? 4 : 8) void adpcm_chunks_kernel(const ChunkJob job) {
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

// ---- XA sector assembly.  One 256-thread workgroup per sector; the sector is built in LDS as a full
// 2352-byte raw sector (the .xa form simply skips the first 16 bytes on write-out, adpcm.c:303-311).
struct XaJob {
    const uint8_t* units;
    int n_sectors, format, stereo, frequency, bits, file_number, channel_number, first_lba;
    const uint8_t* eof_flags;   // optional: eof_flags[s] != 0 sets the EOF submode bit (adpcm.c:334-340)
    uint32_t eof_bits;          // ... or, without eof_flags, bit s for the first 32 sectors (the per-sector call: nothing to upload)
    uint8_t* out;
    // muxed streams (psxhip_str_encode_device): sector s goes to slot dst_sector[s] of the output -- its address (the header's time
    // code, cdrom.c:61-65) is first_lba + that slot, like encode_file_str's sector counter (filefmt.c:450-503) -- and blockIdx.y
    // walks independent streams with the same layout
    const int32_t* dst_sector;  // optional [n_sectors]
    size_t units_stream_stride; // bytes between the streams' unit records
    size_t out_stream_stride;   // bytes between the streams' outputs
};

__device__ __forceinline__ uint8_t to_bcd(int v) { return (uint8_t)(v + (v / 10) * 6); }

__global__ __launch_bounds__(256) void xa_assemble_kernel(const XaJob job) {
    __shared__ __attribute__((aligned(16))) uint8_t sec[2352];
    __shared__ uint32_t crc_tab[256];
    const int tid = (int)threadIdx.x;
    const int s = (int)blockIdx.x;
    const bool four = job.bits == 4;
    const int upg = four ? 8 : 4;                 // sound units per group
    const int sector_size = job.format == 0 ? 2336 : 2352;
    uint32_t* const sec32 = (uint32_t*)sec;

    crc_tab[tid] = c_xa_tables[tid];
    for (int i = tid; i < 2352 / 4; i += 256) sec32[i] = 0u;
    __syncthreads();

    if (tid == 255) {
        if (job.format == 1) {       // psx_cdrom_init_sector, mode 2 (cdrom.c:55-74)
            for (int i = 1; i <= 10; i++) sec[i] = 0xFF;
            const int lba = job.first_lba + (job.dst_sector ? job.dst_sector[s] : s) + 150;
            sec[12] = to_bcd(lba / 4500);
            sec[13] = to_bcd((lba / 75) % 60);
            sec[14] = to_bcd(lba % 75);
            sec[15] = 0x02;
        }
        sec[16] = (uint8_t)job.file_number;
        sec[17] = (uint8_t)(job.channel_number & 0x1F);
        sec[18] = (uint8_t)(0x04 | 0x20 | 0x40);   // AUDIO | FORM2 | RT
        sec[19] = (uint8_t)((job.stereo ? 0x01 : 0) | (job.frequency == 37800 ? 0 : 0x04) | (four ? 0 : 0x10));
        sec[20] = sec[16]; sec[21] = sec[17]; sec[22] = sec[18]; sec[23] = sec[19];
    }

    // sound groups: 18 x 128 bytes at sector offset 0x18 (adpcm.c:193-233,311-322)
    const uint8_t* rec0 = job.units + (size_t)blockIdx.y * job.units_stream_stride + (size_t)s * 18 * upg * (four ? kRecordBytes4 : kRecordBytes);
    if (four) {
        // 4-bit: sample w of the group's 8 units is the 4 bytes (u0 | u1 << 4, u2 | u3 << 4, u4 | u5 << 4, u6 | u7 << 4) at group
        // byte 16 + 4 w.  A record is an SPU block: [header][0][14 code bytes, two samples each].  Thread (group, q) reads dword q
        // of the 8 records -- code bytes 4 q - 2 .. 4 q + 1, i.e. samples 8 q - 4 .. 8 q + 3 (q = 0: its upper half only) -- pairs
        // the low nibbles (even samples) and the high nibbles (odd samples) of unit pairs for four code bytes at once, and
        // transposes 4 x 4 bytes twice: 32 contiguous sector bytes from 8 dword loads.
        if (tid < 18 * 4) {
            const int g = tid >> 2, q = tid & 3;
            const uint32_t* gr = (const uint32_t*)(rec0 + (size_t)g * 8 * kRecordBytes4) + q;
            uint32_t pe[4], po[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint32_t lo = gr[(2 * c) * (kRecordBytes4 / 4)], hi = gr[(2 * c + 1) * (kRecordBytes4 / 4)];
                pe[c] = (lo & 0x0F0F0F0Fu) | ((hi << 4) & 0xF0F0F0F0u);          // byte j: column c of the EVEN sample of code byte j
                po[c] = ((lo >> 4) & 0x0F0F0F0Fu) | (hi & 0xF0F0F0F0u);          // ... of the ODD sample
            }
            // transpose: e[j] = (pe0.j, pe1.j, pe2.j, pe3.j) = the four bytes of sample 2 * (code byte j), o[j] likewise of the sample after it
            uint32_t e[4], o[4];
            {
                const uint32_t a0 = __builtin_amdgcn_perm(pe[1], pe[0], 0x05010400u), a1 = __builtin_amdgcn_perm(pe[1], pe[0], 0x07030602u);
                const uint32_t b0 = __builtin_amdgcn_perm(pe[3], pe[2], 0x05010400u), b1 = __builtin_amdgcn_perm(pe[3], pe[2], 0x07030602u);
                e[0] = __builtin_amdgcn_perm(b0, a0, 0x05040100u); e[1] = __builtin_amdgcn_perm(b0, a0, 0x07060302u);
                e[2] = __builtin_amdgcn_perm(b1, a1, 0x05040100u); e[3] = __builtin_amdgcn_perm(b1, a1, 0x07060302u);
            }
            {
                const uint32_t a0 = __builtin_amdgcn_perm(po[1], po[0], 0x05010400u), a1 = __builtin_amdgcn_perm(po[1], po[0], 0x07030602u);
                const uint32_t b0 = __builtin_amdgcn_perm(po[3], po[2], 0x05010400u), b1 = __builtin_amdgcn_perm(po[3], po[2], 0x07030602u);
                o[0] = __builtin_amdgcn_perm(b0, a0, 0x05040100u); o[1] = __builtin_amdgcn_perm(b0, a0, 0x07060302u);
                o[2] = __builtin_amdgcn_perm(b1, a1, 0x05040100u); o[3] = __builtin_amdgcn_perm(b1, a1, 0x07060302u);
            }
            // dword q holds record bytes 4 q .. 4 q + 3 = code bytes 4 q - 2 + j: samples 2 (4 q - 2 + j) and the one after
            uint32_t* grp = sec32 + (0x18 + g * 128 + 16) / 4;        // the group's 28 sample dwords
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int cb = 4 * q - 2 + j;                         // code byte (q = 0: j = 0, 1 are header and flags)
                if (cb >= 0) { grp[2 * cb] = e[j]; grp[2 * cb + 1] = o[j]; }
            }
        } else if (tid >= 128 && tid < 128 + 18 * 2) {
            // header bytes: units {0,1,2,3} at 0..3 and 4..7, units {4..7} at 8..11 and 12..15
            const int g = (tid - 128) >> 1, half = (tid - 128) & 1;
            const uint8_t* gr = rec0 + (size_t)g * 8 * kRecordBytes4 + (size_t)half * 4 * kRecordBytes4;
            const uint32_t h = (uint32_t)gr[0] | (uint32_t)gr[kRecordBytes4] << 8 | (uint32_t)gr[2 * kRecordBytes4] << 16 | (uint32_t)gr[3 * kRecordBytes4] << 24;
            uint32_t* dst = sec32 + (0x18 + g * 128 + 8 * half) / 4;
            dst[0] = h; dst[1] = h;
        }
    } else {
        for (int i = tid; i < 18 * 128; i += 256) {
            const int g = i >> 7, b = i & 127;
            const uint8_t* gr = rec0 + (size_t)g * upg * kRecordBytes;
            uint8_t v;
            if (b < 16) {
                // 8-bit: units 0..3 at 0..3 and 4..7, bytes 8..15 are never written by the reference (stay 0)
                v = b < 8 ? gr[(b & 3) * kRecordBytes] : 0;
            } else {
                const int w = (b - 16) >> 2, col = (b - 16) & 3;          // sample index, byte column
                v = gr[col * kRecordBytes + 4 + w];
            }
            sec[0x18 + i] = v;
        }
    }
    __syncthreads();

    // form-2 EDC over sector bytes 0x10 .. 0x92B (2332 bytes) -> 0x92C (cdrom.c:102-110): one wavefront (edc_wave).
    // (Before round 4: 256 chunks of 10 bytes, every thread advancing its partial to the END of the span through up to eight
    // bit-matrix products out of LDS -- four wavefronts x 8 products of 32 conditional xors where one wavefront x 6 does.)
    if (tid < 64) {
        const uint32_t c = edc_wave<kEdcSpan>(sec32, crc_tab, tid);
        if (tid == 0) sec32[0x92C / 4] = c;
        // psx_audio_xa_encode_finalize (adpcm.c:334-340) ORs EOF into both subheader copies AFTER the EDC was
        // computed and does not refresh it; kept that way for byte parity.  (Same wavefront, behind its reads of the span.)
        if (tid == 1 && (job.eof_flags ? job.eof_flags[s] != 0 : (s < 32 && ((job.eof_bits >> s) & 1u)))) {
            sec[18] |= 0x80;
            sec[22] = sec[18];
        }
    }
    __syncthreads();

    const int lead = 2352 - sector_size;
    uint8_t* dst = job.out + (size_t)blockIdx.y * job.out_stream_stride + (size_t)(job.dst_sector ? job.dst_sector[s] : s) * sector_size;
    for (int i = tid; i < sector_size / 4; i += 256) ((uint32_t*)dst)[i] = *(const uint32_t*)&sec[lead + 4 * i];
}

// ---- STR video sectors (psxhip_str_encode_device): what encode_file_str does around encode_sector_str for every video slot of the
// stream (filefmt.c:462-475 with :73-91, mdec.c:782-832, cdrom.c:92-100) -- sector header and subheaders, the 32-byte chunk header,
// 2016 bytes of the frame's bitstream, the form-1 EDC -- one workgroup per sector, the frames' bitstreams and results read where the
// frame kernel left them in HBM.  tab[i] = {slot n in the stream, frame (-2: an audio slot with no samples left: a zero sector),
// byte offset into the frame's bitstream, the frame's budget}.
struct StrVideoJob {
    const uint8_t* bs;                      // the frames' bitstreams, bs_stride apart, the streams' bs_stream_stride apart
    size_t bs_stride, bs_stream_stride;
    const psxhip_mdec_result_t* res;        // [streams][frames_per_stream]
    int frames_per_stream;
    const int4* tab;
    int n_entries;
    int format;                             // 6 STR, 7 STRCD, 9 STRV (format_t, args.h:45-58)
    int sector_size;
    int xa_file, xa_channel, video_id, width, height;
    uint8_t* out;
    size_t out_stream_stride;
};

__global__ __launch_bounds__(256) void str_video_sector_kernel(const StrVideoJob job) {
    __shared__ __attribute__((aligned(16))) uint8_t sec[2352];
    __shared__ uint32_t crc_tab[256];
    const int tid = (int)threadIdx.x;
    uint32_t* const sec32 = (uint32_t*)sec;
    const int4 e = job.tab[blockIdx.x];
    const int n = e.x, frame = e.y, offset = e.z, budget = e.w;
    uint8_t* dst = job.out + (size_t)blockIdx.y * job.out_stream_stride + (size_t)n * (size_t)job.sector_size;
    if (frame < 0) {        // an audio slot with no samples left: psx_audio_xa_encode writes nothing (adpcm.c:310); zero here
        for (int i = tid; i < job.sector_size / 4; i += 256) ((uint32_t*)dst)[i] = 0u;
        return;
    }
    crc_tab[tid] = c_xa_tables[tid];
    for (int i = tid; i < 2352 / 4; i += 256) sec32[i] = 0u;
    __syncthreads();
    const int at = job.format == 6 ? 0x08 : (job.format == 7 ? 0x18 : 0x00);          // mdec.c:822-829
    const uint8_t* fo = job.bs + (size_t)blockIdx.y * job.bs_stream_stride + (size_t)frame * job.bs_stride;
    // the 2016 payload bytes: 504 dwords (the frame's bitstream and its slices are dword-aligned, and so is at + 0x20)
    for (int i = tid; i < 2016 / 4; i += 256) sec32[(at + 0x20) / 4 + i] = ((const uint32_t*)(fo + offset))[i];
    if (tid == 255) {
        uint8_t* sub = nullptr;
        if (job.format == 7) {               // psx_cdrom_init_sector(.., MODE2_FORM1), cdrom.c:55-74
            for (int i = 1; i <= 10; i++) sec[i] = 0xFF;
            const int lba = n + 150;
            sec[12] = to_bcd(lba / 4500);
            sec[13] = to_bcd((lba / 75) % 60);
            sec[14] = to_bcd(lba % 75);
            sec[15] = 0x02;
            sub = sec + 16;
        } else if (job.format == 6) {
            sub = sec;
        }
        if (sub) {                           // init_sector_buffer_video, filefmt.c:73-91
            sub[0] = (uint8_t)job.xa_file;
            sub[1] = (uint8_t)(job.xa_channel & 0x1F);
            sub[2] = (uint8_t)(0x08 | 0x40);     // DATA | RT
            sub[3] = 0;
            sub[4] = sub[0]; sub[5] = sub[1]; sub[6] = sub[2]; sub[7] = sub[3];
        }
        // the chunk header of encode_sector_str, mdec.c:782-820
        uint8_t* hd = sec + at;
        const unsigned bytes_used = (unsigned)job.res[(size_t)blockIdx.y * job.frames_per_stream + frame].bytes_used;
        const unsigned fi = (unsigned)(frame + 1);          // frame_index counts from 1
        hd[0x00] = 0x60; hd[0x01] = 0x01;
        hd[0x02] = (uint8_t)job.video_id; hd[0x03] = (uint8_t)(job.video_id >> 8);
        hd[0x04] = (uint8_t)(offset / 2016); hd[0x05] = (uint8_t)((offset / 2016) >> 8);
        hd[0x06] = (uint8_t)(budget / 2016); hd[0x07] = (uint8_t)((budget / 2016) >> 8);
        hd[0x08] = (uint8_t)fi; hd[0x09] = (uint8_t)(fi >> 8); hd[0x0A] = (uint8_t)(fi >> 16); hd[0x0B] = (uint8_t)(fi >> 24);
        hd[0x0C] = (uint8_t)bytes_used; hd[0x0D] = (uint8_t)(bytes_used >> 8); hd[0x0E] = (uint8_t)(bytes_used >> 16); hd[0x0F] = (uint8_t)(bytes_used >> 24);
        hd[0x10] = (uint8_t)job.width; hd[0x11] = (uint8_t)(job.width >> 8);
        hd[0x12] = (uint8_t)job.height; hd[0x13] = (uint8_t)(job.height >> 8);
        for (int i = 0; i < 8; i++) hd[0x14 + i] = fo[i];       // the BS header of the frame
        hd[0x1C] = 0; hd[0x1D] = 0; hd[0x1E] = 0; hd[0x1F] = 0;
    }
    __syncthreads();
    // psx_cdrom_calculate_checksums(.., MODE2_FORM1) as the reference's muxer calls it for every flavour (filefmt.c:474): the EDC of
    // buffer bytes 0x10 .. 0x817 at 0x818 (the ECC behind it is not computed, cdrom.c:99)
    if (tid < 64) {
        const uint32_t c = edc_wave<kEdcSpanForm1>(sec32, crc_tab, tid);
        if (tid == 0) sec32[0x818 / 4] = c;
    }
    __syncthreads();
    for (int i = tid; i < job.sector_size / 4; i += 256) ((uint32_t*)dst)[i] = sec32[i];
}

}  // namespace

extern "C" int psxhip_adpcm_encode_chains_device(int device, const int16_t* d_samples, const psxhip_adpcm_chain_t* d_chains,
                                                 const int32_t* d_unit_base, int n_chains, int filter_count, int bits,
                                                 psxhip_adpcm_state_t* d_states, uint8_t* d_units, void* stream) {
    if (!d_samples || !d_chains || !d_unit_base || !d_states || !d_units || n_chains < 0 ||
        (filter_count != 4 && filter_count != 5) || (bits != 4 && bits != 8) || ((uintptr_t)d_units & 3)) {
        psxhip_set_error("adpcm_encode_chains: bad argument");
        return PSXHIP_EINVAL;
    }
    int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_chains == 0) return PSXHIP_OK;
    ChainJob job;
    job.samples = d_samples;
    job.chains = d_chains;
    job.unit_base = d_unit_base;
    job.n_chains = n_chains;
    job.filter_count = filter_count;
    job.range = bits == 4 ? 12 : 8;
    job.states = d_states;
    job.units = d_units;
    hipLaunchKernelGGL(adpcm_chains_kernel, dim3((unsigned)((n_chains + 3) / 4)), dim3(64), 0, (hipStream_t)stream, job);
    if (hipGetLastError() != hipSuccess) {
        psxhip_set_error("adpcm_encode_chains: launch failed");
        return PSXHIP_EDEVICE;
    }
    return PSXHIP_OK;
}

extern "C" hipError_t psxhip_adpcm_call_launch(const psxhip_adpcm_call_t* a, void* stream) {
    CallJob job;
    memset(&job, 0, sizeof job);
    job.samples = a->samples;
    for (int c = 0; c < 4; c++) {
        job.chains[c] = a->chains[c];
        job.states_in[c] = a->states_in[c];
        job.unit_base[c] = a->unit_base[c];
    }
    job.n_chains = a->n_chains;
    job.filter_count = a->filter_count;
    job.range = a->bits == 4 ? 12 : 8;
    job.stage_elems = a->stage_elems;
    job.states_out = a->states_out;
    job.units = a->units;
    job.spu_out = a->spu_out;
    hipLaunchKernelGGL(adpcm_call_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, job);
    return hipGetLastError();
}
extern "C" int psxhip_adpcm_call_stage_max(void) { return kCallStageMax; }

// final state of every chain = state after its last unit
__global__ void adpcm_gather_final_states_kernel(const psxhip_adpcm_chain_t* chains, const int64_t* state_base, int n_chains,
                                                 const psxhip_adpcm_state_t* unit_states, psxhip_adpcm_state_t* states) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= n_chains) return;
    const int n = chains[c].n_units;
    if (n > 0) states[c] = unit_states[state_base[c] + n - 1];
}

namespace {
// A session owns a dozen device buffers.  The one-call entry points (psxhip_adpcm_encode_chains_chunked and the *_host
// wrappers above it) build and drop a session per call, and a dozen hipMalloc / hipFree pairs cost more than encoding a
// minute of audio: freed blocks are parked per host thread and handed out again (smallest block that fits and is not more
// than four times too large).  psxhip_release_scratch() empties the cache.  A session synchronises its stream before it
// lets go of its buffers, so a parked block has no work in flight.
struct BlockCache {
    static constexpr int kMax = 32;
    struct Entry { void* p; size_t cap; int device; };
    Entry e[kMax];
    int n = 0;
    void* take(size_t need, int device, size_t* cap) {
        int best = -1;
        for (int i = 0; i < n; i++)
            if (e[i].device == device && e[i].cap >= need && e[i].cap <= 4 * need + 4096 && (best < 0 || e[i].cap < e[best].cap)) best = i;
        if (best < 0) return nullptr;
        void* p = e[best].p;
        *cap = e[best].cap;
        e[best] = e[--n];
        return p;
    }
    bool park(void* p, size_t cap, int device) {
        if (n == kMax) return false;
        e[n++] = Entry{p, cap, device};
        return true;
    }
    void release() {
        for (int i = 0; i < n; i++) (void)hipFree(e[i].p);
        n = 0;
    }
    ~BlockCache() { release(); }
};
thread_local BlockCache g_blocks;

struct DevMem {
    void* p = nullptr;
    size_t cap = 0;
    int device = 0;
    ~DevMem() {
        if (p && !g_blocks.park(p, cap, device)) (void)hipFree(p);
    }
    hipError_t alloc(size_t n) {
        if (!n) n = 4;
        (void)hipGetDevice(&device);
        p = g_blocks.take(n, device, &cap);
        if (p) return hipSuccess;
        cap = (n + 255) & ~(size_t)255;
        return hipMalloc(&p, cap);
    }
    template <typename T> T* as() { return (T*)p; }
};
}  // namespace

extern "C" void psxhip_adpcm_release_blocks(void) { g_blocks.release(); }

struct psxhip_adpcm_session {
    int device, n_chains, n_chunks;
    bool speculated;
    hipStream_t stream;
    ChunkJob job;
    DevMem d_chains, d_base, d_sbase, d_cchain, d_cfirst, d_ustates, d_used, d_cstates, d_lead, d_final, d_known, d_flags;
    int* h_flags = nullptr;     // page-locked: the verify passes' "changed" words travel back through it (a session's runs are serialised)
    // optional (psxhip_adpcm_session_set_timing): HIP events around the speculate launch and the verify passes of a run
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool timing = false;
    float spec_ms = 0.0f, verify_ms = 0.0f;
    ~psxhip_adpcm_session() {
        if (h_flags) (void)hipHostFree(h_flags);
        for (int i = 0; i < 3; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
};

#define TRY(expr)                                                                                   \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess) {                                                                    \
            psxhip_set_error("%s failed: %s", #expr, hipGetErrorString(e__));                       \
            return PSXHIP_EDEVICE;                                                                  \
        }                                                                                           \
    } while (0)

extern "C" int psxhip_adpcm_session_create(psxhip_adpcm_session_t** out, int device, const int16_t* d_samples,
                                           const psxhip_adpcm_chain_t* chains, const int32_t* unit_base,
                                           const int32_t* lead_units, int n_chains, int filter_count, int bits,
                                           uint8_t* d_units, int chunk_units, int warmup_units, void* stream) {
    if (!out) return PSXHIP_EINVAL;
    *out = nullptr;
    if (!d_samples || !chains || !unit_base || !d_units || n_chains < 0 || (filter_count != 4 && filter_count != 5) ||
        (bits != 4 && bits != 8) || chunk_units < 1 || warmup_units < 0 || ((uintptr_t)d_units & 3)) {
        psxhip_set_error("adpcm_session_create: bad argument");
        return PSXHIP_EINVAL;
    }
    int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    struct Guard {                       // frees the half-built session on every early return
        psxhip_adpcm_session* p;
        ~Guard() { delete p; }
    } guard{new psxhip_adpcm_session()};
    psxhip_adpcm_session* s = guard.p;
    s->device = device;
    s->n_chains = n_chains;
    s->speculated = false;
    s->stream = (hipStream_t)stream;

    std::vector<int64_t> state_base((size_t)n_chains);
    std::vector<int32_t> chunk_chain, chunk_first, lead((size_t)n_chains, 0);
    int64_t total_units = 0;
    for (int c = 0; c < n_chains; c++) {
        state_base[(size_t)c] = total_units;
        for (int f = 0; f < chains[c].n_units; f += chunk_units) {
            chunk_chain.push_back(c);
            chunk_first.push_back(f);
        }
        total_units += chains[c].n_units;
        if (lead_units) lead[(size_t)c] = lead_units[c] < 0 ? 0 : lead_units[c];
    }
    s->n_chunks = (int)chunk_chain.size();
    const int nc = n_chains ? n_chains : 1, nk = s->n_chunks ? s->n_chunks : 1;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = s->d_chains.alloc(sizeof(psxhip_adpcm_chain_t) * nc);
    if (e == hipSuccess) e = s->d_base.alloc(sizeof(int32_t) * nc);
    if (e == hipSuccess) e = s->d_sbase.alloc(sizeof(int64_t) * nc);
    if (e == hipSuccess) e = s->d_lead.alloc(sizeof(int32_t) * nc);
    if (e == hipSuccess) e = s->d_cstates.alloc(sizeof(psxhip_adpcm_state_t) * nc);
    if (e == hipSuccess) e = s->d_final.alloc(sizeof(psxhip_adpcm_state_t) * nc);
    if (e == hipSuccess) e = s->d_known.alloc(nc);
    if (e == hipSuccess) e = s->d_flags.alloc(64 * sizeof(int));
    if (e == hipSuccess) e = s->d_cchain.alloc(sizeof(int32_t) * nk);
    if (e == hipSuccess) e = s->d_cfirst.alloc(sizeof(int32_t) * nk);
    if (e == hipSuccess) e = s->d_used.alloc(sizeof(psxhip_adpcm_state_t) * nk);
    if (e == hipSuccess) e = s->d_ustates.alloc(sizeof(psxhip_adpcm_state_t) * (size_t)(total_units ? total_units : 1));
    if (e != hipSuccess) {
        psxhip_set_error("adpcm_session_create: hipMalloc failed: %s", hipGetErrorString(e));
        return PSXHIP_ENOMEM;
    }
    hipStream_t st = s->stream;
    if (n_chains) {
        TRY(hipMemcpyAsync(s->d_chains.p, chains, sizeof(psxhip_adpcm_chain_t) * n_chains, hipMemcpyHostToDevice, st));
        TRY(hipMemcpyAsync(s->d_base.p, unit_base, sizeof(int32_t) * n_chains, hipMemcpyHostToDevice, st));
        TRY(hipMemcpyAsync(s->d_sbase.p, state_base.data(), sizeof(int64_t) * n_chains, hipMemcpyHostToDevice, st));
        TRY(hipMemcpyAsync(s->d_lead.p, lead.data(), sizeof(int32_t) * n_chains, hipMemcpyHostToDevice, st));
    }
    if (s->n_chunks) {
        TRY(hipMemcpyAsync(s->d_cchain.p, chunk_chain.data(), sizeof(int32_t) * s->n_chunks, hipMemcpyHostToDevice, st));
        TRY(hipMemcpyAsync(s->d_cfirst.p, chunk_first.data(), sizeof(int32_t) * s->n_chunks, hipMemcpyHostToDevice, st));
    }
    TRY(hipStreamSynchronize(st));    // the host vectors go out of scope

    ChunkJob& job = s->job;
    job.samples = d_samples;
    job.chains = s->d_chains.as<psxhip_adpcm_chain_t>();
    job.unit_base = s->d_base.as<int32_t>();
    job.state_base = s->d_sbase.as<int64_t>();
    job.chunk_chain = s->d_cchain.as<int32_t>();
    job.chunk_first = s->d_cfirst.as<int32_t>();
    job.n_chunks = s->n_chunks;
    job.chunk_units = chunk_units;
    job.warmup_units = warmup_units;
    job.filter_count = filter_count;
    job.range = bits == 4 ? 12 : 8;
    job.chain_states = s->d_cstates.as<psxhip_adpcm_state_t>();
    job.lead_units = s->d_lead.as<int32_t>();
    job.start_known = s->d_known.as<uint8_t>();
    job.unit_states = s->d_ustates.as<psxhip_adpcm_state_t>();
    job.start_used = s->d_used.as<psxhip_adpcm_state_t>();
    job.units = d_units;
    job.changed = nullptr;      // set by session_run, per pass
    job.changed_before = nullptr;
    guard.p = nullptr;                   // ownership passes to the caller
    *out = s;
    return PSXHIP_OK;
}

// HIP events around the speculate launch and around the verify passes of every run that speculates (i.e. the first run after a
// create / reset): bench.py's live kernel-level timing.  The events cost two extra packets per run; off by default.
extern "C" int psxhip_adpcm_session_set_timing(psxhip_adpcm_session_t* s, int on) {
    if (!s) return PSXHIP_EINVAL;
    if (on && !s->ev[0]) {
        if (hipSetDevice(s->device) != hipSuccess) return PSXHIP_EDEVICE;
        for (int i = 0; i < 3; i++)
            if (hipEventCreate(&s->ev[i]) != hipSuccess) { psxhip_set_error("adpcm_session_set_timing: hipEventCreate failed"); return PSXHIP_EDEVICE; }
    }
    s->timing = on != 0;
    return PSXHIP_OK;
}
extern "C" int psxhip_adpcm_session_last_timing(const psxhip_adpcm_session_t* s, float* speculate_ms, float* verify_ms) {
    if (!s) return PSXHIP_EINVAL;
    if (speculate_ms) *speculate_ms = s->spec_ms;
    if (verify_ms) *verify_ms = s->verify_ms;
    return PSXHIP_OK;
}
extern "C" const char* psxhip_adpcm_kernel_rev(void) { return PSXHIP_ADPCM_KERNEL_REV; }

extern "C" void psxhip_adpcm_session_reset(psxhip_adpcm_session_t* s) {
    if (s) s->speculated = false;        // the next run speculates again from scratch (same buffers, same chunk tables)
}

extern "C" void psxhip_adpcm_session_destroy(psxhip_adpcm_session_t* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    delete s;
}

extern "C" int psxhip_adpcm_session_run(psxhip_adpcm_session_t* s, const psxhip_adpcm_state_t* start_states,
                                        const uint8_t* start_known, int max_passes, psxhip_adpcm_state_t* final_states,
                                        int* any_change) {
    if (!s || !start_states) {
        psxhip_set_error("adpcm_session_run: NULL argument");
        return PSXHIP_EINVAL;
    }
    if (any_change) *any_change = 0;
    TRY(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    if (s->n_chains == 0) return 0;
    TRY(hipMemcpyAsync(s->d_cstates.p, start_states, sizeof(psxhip_adpcm_state_t) * s->n_chains, hipMemcpyHostToDevice, st));
    if (start_known) TRY(hipMemcpyAsync(s->d_known.p, start_known, (size_t)s->n_chains, hipMemcpyHostToDevice, st));
    else TRY(hipMemsetAsync(s->d_known.p, 1, (size_t)s->n_chains, st));
    int passes = 0;
    if (s->n_chunks) {
        // "some chunk's start state changed" is one word of device memory per pass.  Passes are launched in batches, back to
        // back: pass i + 1 looks at pass i's word when it starts and returns at once if nothing changed, so the host reads the
        // words once per batch -- no synchronise + launch round trip (40-50 us) per pass.  The words travel back through a
        // page-locked buffer of the session (a run is synchronous).
        constexpr int kBatchMax = 64;          // (the flags' room; batches grow 3, 6, 12, 16, 16 ...)
        int*& h_flags = s->h_flags;      // owned by the session (a buffer per calling thread leaked one per worker thread of the multi-device calls)
        if (!h_flags && hipHostMalloc((void**)&h_flags, kBatchMax * sizeof(int), hipHostMallocDefault) != hipSuccess) {
            h_flags = nullptr;
            psxhip_set_error("adpcm_session_run: no page-locked memory for the verify flags");
            return PSXHIP_ENOMEM;
        }
        int* d_flags = s->d_flags.as<int>();
        // XA's 4 filters fill 12 of a row's lanes: 12-lane rows, five chunks per wavefront; SPU's 5 filters need 16-lane rows
        const bool narrow = s->job.filter_count == 4;
        const int per = narrow ? 5 : 4;
        const dim3 grid((unsigned)((s->n_chunks + per - 1) / per)), block(64);
        const bool timed = s->timing && !s->speculated;
        if (!s->speculated) {
            s->job.changed = d_flags;
            s->job.changed_before = nullptr;
            if (timed) TRY(hipEventRecord(s->ev[0], st));
            if (narrow) hipLaunchKernelGGL((adpcm_chunks_kernel<false, 12>), grid, block, 0, st, s->job);
            else hipLaunchKernelGGL((adpcm_chunks_kernel<false, 16>), grid, block, 0, st, s->job);
            TRY(hipGetLastError());
            if (timed) TRY(hipEventRecord(s->ev[1], st));
            s->speculated = true;
            if (any_change) *any_change = 1;
        }
        // first batch: most material is done after "one pass that repairs + one that finds nothing"
        // (measured, NOTEBOOK round 6: with every batch 48 passes a short stream's whole verify phase is ONE batch, no host round trip
        //  in it -- the round trips cost nothing measurable)
        int batch = 3;
        for (bool done = false; !done;) {
            if (max_passes > 0 && passes + batch > max_passes) batch = max_passes - passes;
            if (batch < 1) {
                psxhip_set_error("adpcm_session_run: not converged after %d verify passes", passes);
                return PSXHIP_EINVAL;
            }
            TRY(hipMemsetAsync(d_flags, 0, kBatchMax * sizeof(int), st));
            for (int i = 0; i < batch; i++) {
                s->job.changed = d_flags + i;
                s->job.changed_before = i ? d_flags + i - 1 : nullptr;
                if (narrow) hipLaunchKernelGGL((adpcm_chunks_kernel<true, 12>), grid, block, 0, st, s->job);
                else hipLaunchKernelGGL((adpcm_chunks_kernel<true, 16>), grid, block, 0, st, s->job);
            }
            TRY(hipGetLastError());
            TRY(hipMemcpyAsync(h_flags, d_flags, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st));
            TRY(hipStreamSynchronize(st));
            for (int i = 0; i < batch && !done; i++) {
                passes++;                      // this pass ran
                if (h_flags[i]) { if (any_change) *any_change = 1; }
                else done = true;              // it changed nothing: the fixpoint; the passes behind it returned at once
            }
            batch = batch * 2 < 16 ? batch * 2 : 16;
        }
        if (timed) {
            TRY(hipEventRecord(s->ev[2], st));
            TRY(hipEventSynchronize(s->ev[2]));
            TRY(hipEventElapsedTime(&s->spec_ms, s->ev[0], s->ev[1]));
            TRY(hipEventElapsedTime(&s->verify_ms, s->ev[1], s->ev[2]));
        }
    }
    // chains without units keep their start state
    TRY(hipMemcpyAsync(s->d_final.p, s->d_cstates.p, sizeof(psxhip_adpcm_state_t) * s->n_chains, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(adpcm_gather_final_states_kernel, dim3((unsigned)((s->n_chains + 255) / 256)), dim3(256), 0, st,
                       s->job.chains, s->job.state_base, s->n_chains, s->job.unit_states, s->d_final.as<psxhip_adpcm_state_t>());
    TRY(hipGetLastError());
    if (final_states)
        TRY(hipMemcpyAsync(final_states, s->d_final.p, sizeof(psxhip_adpcm_state_t) * s->n_chains, hipMemcpyDeviceToHost, st));
    TRY(hipStreamSynchronize(st));
    return passes;
}

extern "C" int psxhip_adpcm_encode_chains_chunked(int device, const int16_t* d_samples, const psxhip_adpcm_chain_t* chains,
                                                  const int32_t* unit_base, int n_chains, int filter_count, int bits,
                                                  psxhip_adpcm_state_t* d_states, uint8_t* d_units, int chunk_units,
                                                  int warmup_units, int max_passes, void* stream) {
    if (!d_states) {
        psxhip_set_error("adpcm_encode_chains_chunked: bad argument");
        return PSXHIP_EINVAL;
    }
    if (n_chains == 0) return 0;
    psxhip_adpcm_session_t* s = nullptr;
    int rc = psxhip_adpcm_session_create(&s, device, d_samples, chains, unit_base, nullptr, n_chains, filter_count, bits, d_units,
                                         chunk_units, warmup_units, stream);
    if (rc) return rc;
    std::vector<psxhip_adpcm_state_t> st((size_t)n_chains);
    hipError_t e = hipMemcpy(st.data(), d_states, sizeof(psxhip_adpcm_state_t) * n_chains, hipMemcpyDeviceToHost);
    int passes = PSXHIP_EDEVICE;
    if (e == hipSuccess) {
        passes = psxhip_adpcm_session_run(s, st.data(), nullptr, max_passes, st.data(), nullptr);
        if (passes >= 0) e = hipMemcpy(d_states, st.data(), sizeof(psxhip_adpcm_state_t) * n_chains, hipMemcpyHostToDevice);
    }
    psxhip_adpcm_session_destroy(s);
    if (e != hipSuccess) {
        psxhip_set_error("adpcm_encode_chains_chunked: state copy failed: %s", hipGetErrorString(e));
        return PSXHIP_EDEVICE;
    }
    return passes;
}
#undef TRY

extern "C" int psxhip_spu_pack_device(int device, const uint8_t* d_units, int n_blocks, uint8_t* d_out, void* stream) {
    if (!d_units || !d_out || n_blocks < 0 || ((uintptr_t)d_out & 15) || ((uintptr_t)d_units & 3)) {
        psxhip_set_error("spu_pack: bad argument (d_out must be 16-byte aligned)");
        return PSXHIP_EINVAL;
    }
    int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_blocks == 0) return PSXHIP_OK;
    hipLaunchKernelGGL(spu_pack_kernel, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_units,
                       n_blocks, d_out);
    if (hipGetLastError() != hipSuccess) {
        psxhip_set_error("spu_pack: launch failed");
        return PSXHIP_EDEVICE;
    }
    return PSXHIP_OK;
}

extern "C" int psxhip_xa_assemble_device(int device, const uint8_t* d_units, int n_sectors, int format, int stereo,
                                         int frequency, int bits, int file_number, int channel_number, int first_lba,
                                         const uint8_t* d_eof_flags, uint8_t* d_out, void* stream) {
    return psxhip_xa_assemble_device_bits(device, d_units, n_sectors, format, stereo, frequency, bits, file_number, channel_number, first_lba,
                                          d_eof_flags, 0u, d_out, stream);
}

extern "C" int psxhip_xa_assemble_device_bits(int device, const uint8_t* d_units, int n_sectors, int format, int stereo,
                                              int frequency, int bits, int file_number, int channel_number, int first_lba,
                                              const uint8_t* d_eof_flags, uint32_t eof_bits, uint8_t* d_out, void* stream) {
    return psxhip_xa_assemble_scatter(device, d_units, n_sectors, format, stereo, frequency, bits, file_number, channel_number, first_lba,
                                      d_eof_flags, eof_bits, d_out, nullptr, 1, 0, 0, stream);
}

// ... n_streams streams of n_sectors sectors each (unit records units_stream_stride bytes apart, outputs out_stream_stride apart), every
// sector s written to slot d_dst_sector[s] of its stream's output (NULL: slot s), its header address first_lba + that slot
extern "C" int psxhip_xa_assemble_scatter(int device, const uint8_t* d_units, int n_sectors, int format, int stereo,
                                          int frequency, int bits, int file_number, int channel_number, int first_lba,
                                          const uint8_t* d_eof_flags, uint32_t eof_bits, uint8_t* d_out, const int32_t* d_dst_sector,
                                          int n_streams, size_t units_stream_stride, size_t out_stream_stride, void* stream) {
    if (!d_units || !d_out || n_sectors < 0 || n_streams < 1 || n_streams > 65535 || (format != 0 && format != 1) || (bits != 4 && bits != 8) ||
        ((uintptr_t)d_out & 3) || (out_stream_stride & 3) || (units_stream_stride & 3)) {
        psxhip_set_error("xa_assemble: bad argument");
        return PSXHIP_EINVAL;
    }
    int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_sectors == 0) return PSXHIP_OK;
    rc = xa_tables(device);
    if (rc) return rc;
    XaJob job;
    job.units = d_units;
    job.n_sectors = n_sectors;
    job.format = format;
    job.stereo = stereo;
    job.frequency = frequency;
    job.bits = bits;
    job.file_number = file_number;
    job.channel_number = channel_number;
    job.first_lba = first_lba;
    job.eof_flags = d_eof_flags;
    job.eof_bits = eof_bits;
    job.out = d_out;
    job.dst_sector = d_dst_sector;
    job.units_stream_stride = units_stream_stride;
    job.out_stream_stride = out_stream_stride;
    hipLaunchKernelGGL(xa_assemble_kernel, dim3((unsigned)n_sectors, (unsigned)n_streams), dim3(256), 0, (hipStream_t)stream, job);
    if (hipGetLastError() != hipSuccess) {
        psxhip_set_error("xa_assemble: launch failed");
        return PSXHIP_EDEVICE;
    }
    return PSXHIP_OK;
}


extern "C" int psxhip_str_video_sectors_launch(int device, const psxhip_str_video_job_t* a, void* stream) {
    if (!a || !a->d_bs || !a->d_res || !a->d_tab || !a->d_out || a->n_entries < 0 || a->n_streams < 1 || a->n_streams > 65535 ||
        (a->bs_stride & 3) || (a->bs_stream_stride & 3) || (a->out_stream_stride & 3) || ((uintptr_t)a->d_bs & 3) || ((uintptr_t)a->d_out & 3)) {
        psxhip_set_error("str_video_sectors: bad argument");
        return PSXHIP_EINVAL;
    }
    int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (a->n_entries == 0) return PSXHIP_OK;
    rc = xa_tables(device);
    if (rc) return rc;
    StrVideoJob job;
    job.bs = a->d_bs;
    job.bs_stride = a->bs_stride;
    job.bs_stream_stride = a->bs_stream_stride;
    job.res = a->d_res;
    job.frames_per_stream = a->frames_per_stream;
    job.tab = (const int4*)a->d_tab;
    job.n_entries = a->n_entries;
    job.format = a->format;
    job.sector_size = a->sector_size;
    job.xa_file = a->xa_file;
    job.xa_channel = a->xa_channel;
    job.video_id = a->video_id;
    job.width = a->width;
    job.height = a->height;
    job.out = a->d_out;
    job.out_stream_stride = a->out_stream_stride;
    hipLaunchKernelGGL(str_video_sector_kernel, dim3((unsigned)a->n_entries, (unsigned)a->n_streams), dim3(256), 0, (hipStream_t)stream, job);
    if (hipGetLastError() != hipSuccess) {
        psxhip_set_error("str_video_sectors: launch failed");
        return PSXHIP_EDEVICE;
    }
    return PSXHIP_OK;
}
