// mdec_split.inc -- ONE frame across MANY workgroups (included by mdec_kernels.hip: same tables, same quantiser, same DCT forms).
//
// The frame kernel above gives a frame to one workgroup: right when a launch has more frames than the chip has compute units, wrong
// for the reference's own call pattern -- encode_frame_bs, one frame per call (psxavenc/filefmt.c:641-647) -- where 255 of 256 CUs
// idle for 52 us.  This kernel is for launches of a FEW frames.  The reference encodes macroblocks column-major (mdec.c:689-690), so
// any run of consecutive macroblocks in that order is one contiguous piece of the frame's bitstream; BS v2 carries no state from one
// macroblock to the next, v3 only the DC predictors (mdec.c:454-479).  Hence:
//
//   * a frame is cut into SEGMENTS of M consecutive macroblocks (M = 1, 2, 4, 8 or 16), one workgroup of 16 wavefronts each;
//   * phase A: M wavefronts transform one macroblock each (the coefficients stay in LDS, in scan order);
//     v3: the quantised DC terms go to a per-frame table in HBM (biased, so that a word is never zero), every group reads all of
//     them and runs the three DPCM chains itself (the step-function scan of the frame kernel): it knows the deltas of its own blocks;
//   * phase B: the rate-control loop (mdec.c:663-723) as it is written -- "the first scale that fits" -- sixteen scales at a time:
//     wavefront (m, j) counts macroblock m's bits at its share of the round's scales; a group PUBLISHES its sixteen sums
//     (bits | non-zero coefficients << 32, never zero) in its own slots of the frame's workspace;
//   * every group then reads every group's slots -- a slot that still reads zero is looked at again: the data is its own arrival
//     signal -- and so holds, per scale, the frame's total and the bits of the segments before its own.  The first scale whose
//     stream fits is the reference's answer, exactly, because every scale below it was evaluated and did not.  No fit among
//     sixteen: the next sixteen (rare: scale > 16 is heavy noise; a first round is EIGHT scales when the previous call's answer was
//     at most 6).  Every group of a frame is resident (the host keeps segments <= CUs, and split launches of a device go one behind
//     the other), so waiting is safe, and it is bounded by a watchdog all the same.  While the sums travel, two wavefronts of every
//     macroblock already build its stream at the hinted scale and the one above it, each into a buffer of its own from bit 0;
//   * phase C: a macroblock's bit offset is the sum of the earlier segments' bits at the answer + the earlier macroblocks of its
//     segment; its stream (built ahead, or now) is funnel-shifted to that phase and OR-ed into the frame image in HBM (neighbours meet
//     inside a dword);
//   * what crosses groups crosses as device-scope atomics on words of its own (stores, loads, ORs): performed at the memory side,
//     no cache-wide write-back or invalidate anywhere -- and no word that many groups add to: device-scope atomics on ONE cache
//     line are served one after the other, ~10 ns each (the first version summed the totals with 16 atomic adds per group: 150
//     groups met after 25 us);
//   * the group of the frame's LAST segment waits for every group's done word, adds the header, writes the image out as the frame's row --
//     coalesced, zero tail included (the reference's memset, mdec.c:676); write-through stores and no atomics: the row may be
//     page-locked host memory whose CPU waits for the flag raised behind it -- and zeroes the workspace for the next launch.
//
// Results are identical to the frame kernel's and to the reference's loop by construction: same DCT forms (fdct8_pk), same
// quantiser (quant_mag), same tables, and the search is the reference's own ascending scan.
//
// Released frames.  A wait that outlasts the patience gives the frame up: its row is zero and its quant_scale PSXHIP_MDEC_QS_RELEASED
// (not 64: that is "fits nowhere"), counted once in psxhip_mdec_watchdog; the host-buffer entry points encode it again with the frame
// kernel.  Groups of a released frame may still come and publish into the workspace, so every group counts itself out and the last
// one out of a released frame zeroes the whole workspace (see `leave` below): no word of one launch reaches the next.
//
// Test switches (read when a context is created, psxhip_api.cpp):
//   PSXHIP_MDEC_SPLIT_WITHHOLD=frame:segment[:launches[:residue]] -- for the context's first `launches` split launches (default 1),
//     every other group of frame `frame` reads segment `segment`'s slots, DC words and done word as never there, without waiting
//     (segment: 0 .. segs - 1, `mid` = segs / 2, negative = from the end: -1 is the finisher's own).  The withheld group publishes
//     nothing and leaves; with `residue` it publishes its round-0 sums, its DC words and done = 2 and leaves, and the finisher does not
//     zero that segment's words -- what a group that comes after the finisher leaves, without timing.
//   PSXHIP_MDEC_SPLIT_PATIENCE=<ticks of the 100 MHz clock> -- the patience of every wait (default 20 000 000: 0.2 s).  A short one
//     makes real releases and real late groups on an idle GPU; it only shortens waits.

namespace {

struct SplitJob {
    const uint8_t* frames;
    uint8_t* out;
    psxhip_mdec_result_t* results;
    const int32_t* max_sizes;        // per-frame budgets or NULL
    size_t frame_stride, out_stride;
    int width, height, nx, ny, nmb;
    int n_frames, uniform_max_size, max_frame_size;
    int seg_mbs;                     // M
    int segs;                        // workgroups per frame: ceil(nmb / M)
    unsigned char* ws;               // workspace, ws_stride bytes per frame, all zero between launches:
    size_t ws_stride;                //   [64 B][slots 5 rounds x nmb x 16 x 8 B][DC words nmb x 3 x 4 B][image img_words x 4 B][done words nmb x 4 B]
    size_t ws_slots, ws_dcq, ws_img, ws_done;
    int img_words;
    unsigned* lost;                  // frames given up by the watchdog (never reset; psxhip_mdec_watchdog)
    int hint;                        // the answer of this context's previous one-frame call (0: none): where the speculative streams are built
    unsigned* done_flag;             // page-locked host word the last group stores done_seq into once the frame's row and result are written (one-frame calls), or NULL
    unsigned done_seq;
    unsigned long long patience;     // ticks a rendezvous waits (kSplitPatience; PSXHIP_MDEC_SPLIT_PATIENCE)
    int wh_frame, wh_seg, wh_residue;   // PSXHIP_MDEC_SPLIT_WITHHOLD (tests): segment wh_seg of frame wh_frame never arrives (wh_seg < 0: off)
};

__device__ __forceinline__ unsigned ld_agent(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long ld_agent64(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A published word (never zero), read when it is there: device-scope loads until it reads non-zero.  Returns 0 when the watchdog gives up.
template <typename T>
__device__ __forceinline__ T split_await(const T* p, unsigned long long patience) {
    T v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v) return v;
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        __builtin_amdgcn_s_sleep(2);
        v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v || wall_clock64() - t0 > patience) return v;
    }
}
// a word of the frame's row or result: written through to wherever the row lives (HBM, or the page-locked host block of a one-frame
// call, whose CPU looks at it as soon as the flag is up)
__device__ __forceinline__ void row_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
// this wavefront's device-scope atomics have been performed (their return values are in)
__device__ __forceinline__ void split_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ void split_put_bits(uint32_t* words, uint32_t pos, int len, uint32_t v) {
    const uint32_t w = pos >> 5, sh = pos & 31;
    const uint32_t top = v << (32 - len);
    const uint32_t hi = top >> sh, lo = __builtin_amdgcn_alignbit(top, 0u, sh);
    __hip_atomic_fetch_or(&words[w], hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (lo) __hip_atomic_fetch_or(&words[w + 1], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int CODEC>
__global__ __launch_bounds__(kSplitThreads, 8) void mdec_split_kernel(const SplitJob job) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = job.seg_mbs, segs = job.segs, nmb = job.nmb, ny = job.ny, W = job.width, H = job.height;
    const int f = (int)blockIdx.x / segs, seg = (int)blockIdx.x - f * segs;
    const int mb0 = seg * M;
    const int nm = nmb - mb0 < M ? nmb - mb0 : M;

    // ---- LDS
    size_t o = 0;
    int* sc = (int*)(smem + o);                 o += 96 * 4;
    uint16_t* l_len = (uint16_t*)(smem + o);    o += (BS_LUT_SIZE * 2 + 15) & ~15;
    uint32_t* l_code = (uint32_t*)(smem + o);   o += (BS_LUT_SIZE * 4 + 15) & ~15;
    int16_t* Z = (int16_t*)(smem + o);          o += (size_t)M * 6 * 64 * 2;
    int* mbbits = (int*)(smem + o);             o += (size_t)M * kSplitRound * 4;
    int16_t* dcl = (int16_t*)(smem + o);        o += (size_t)M * 8 * 2;
    uint32_t* wbuf = (uint32_t*)(smem + o);     o += (size_t)kSplitWaves * kSplitWbufWords * 4;      // per wavefront: a macroblock's stream from bit 0
    int16_t* T = (int16_t*)wbuf;                // (the DCT's transpose tiles, dead before the first stream is built)
    int16_t* dcv = (int16_t*)(smem + o);        if (CODEC != 0) o += ((size_t)nmb * 6 * 2 + 15) & ~15;
    int* dc_fn = (int*)(smem + o);
    enum { SC_LBITS = 0, SC_LNNZ = 16, SC_TOT = 32, SC_NNZ = 48, SC_PRE = 64, SC_DEAD = 80, SC_ANSWER, SC_LAST, SC_SINK, SC_EXIT, SC_COUNT = 96 };

    // ---- workspace of this frame
    unsigned char* wsf = job.ws + (size_t)f * job.ws_stride;
    unsigned long long* slots = (unsigned long long*)(wsf + job.ws_slots);       // [round][segment][16]
    unsigned* dcw = (unsigned*)(wsf + job.ws_dcq);                               // v3: [macroblock][3] two biased DC terms per word
    unsigned* img = (unsigned*)(wsf + job.ws_img);
    unsigned* done = (unsigned*)(wsf + job.ws_done);                             // [segment] 1: done, 2: done, released by the watchdog
    // PSXHIP_MDEC_SPLIT_WITHHOLD (tests): every other group of the frame reads the withheld segment's words as never there, without
    // waiting; the withheld group itself publishes nothing (or, with `residue`, its round-0 sums, its DC words and done = 2) and leaves
    const bool wh = job.wh_seg >= 0 && f == job.wh_frame, withheld = wh && seg == job.wh_seg;
    auto hidden = [&](int g) { return wh && !withheld && g == job.wh_seg; };
    const unsigned long long pat = job.patience;
    unsigned* exits = (unsigned*)wsf;                                            // groups of the frame that have left | 0x10000: released

    // Leaving.  A frame the finisher released may still have groups to come: they publish sums, DC words and done words, and OR image
    // bits, into a workspace the next launch reads as its own arrivals.  So every group counts itself out (the finisher adds 0x10000 when
    // it released the frame), and the last one out of a released frame returns the whole workspace to zero.  Split launches of a device
    // run one behind the other, so nothing of this launch is left when the next one starts.  (A frame that was not released was
    // tidied by its finisher, behind every group's done word: the last one out only resets the count.)
    auto leave = [&](unsigned inc) {
        split_drain();
        __syncthreads();
        if (tid == 0) {
            const unsigned now = __hip_atomic_fetch_add(exits, inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + inc;
            sc[SC_EXIT] = (now & 0xFFFFu) == (unsigned)segs ? (now >> 16 ? 2 : 1) : 0;
        }
        __syncthreads();
        const int last = sc[SC_EXIT];
        if (last == 2) {
            for (int i = tid; i < job.img_words; i += kSplitThreads) __hip_atomic_store(&img[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int r = 0; r < kSplitRounds; r++)
                for (int i = tid; i < segs * kSplitRound; i += kSplitThreads)
                    __hip_atomic_store(&slots[((size_t)r * nmb) * kSplitRound + i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (CODEC != 0)
                for (int i = tid; i < nmb * 3; i += kSplitThreads) __hip_atomic_store(&dcw[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int i = tid; i < segs; i += kSplitThreads) __hip_atomic_store(&done[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (last && tid == 0) __hip_atomic_store(exits, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };

    if (withheld && !job.wh_residue && seg != segs - 1) { leave(1u); return; }
    int max_size = job.max_sizes ? job.max_sizes[f] : job.uniform_max_size;
    const bool bad_budget = max_size < 8 || max_size > job.max_frame_size || (size_t)max_size > job.out_stride;
    if (bad_budget) max_size = 8;
    const int limit_bits = 16 * ((max_size - 8) >> 1);

    // ---- prologue.  Every global load the group needs before its first barrier is issued before the first one is waited for: this
    //      lane's pixels, its scan-order constants, the tables -- one round trip to memory, not three
    const int blk = lane >> 3, r8 = lane & 7;
    uint32_t pw[4] = {0u, 0u, 0u, 0u};          // the lane's pixel row: 16 bytes of interleaved chroma, or 8 of luma
    if (wid < nm && lane < 48) {
        const int mbe = mb0 + wid;
        const int fx = mbe / ny, fy = mbe - fx * ny;
        const uint8_t* frame = job.frames + (size_t)f * job.frame_stride;
        if (blk < 2) {
            const uint32_t* p = (const uint32_t*)(frame + (size_t)W * H + (size_t)W * (fy * 8 + r8) + (size_t)fx * 16);
            pw[0] = p[0]; pw[1] = p[1]; pw[2] = p[2]; pw[3] = p[3];
        } else {
            const int by = (blk - 2) >> 1, bx = (blk - 2) & 1;
            const uint32_t* p = (const uint32_t*)(frame + (size_t)W * (fy * 16 + by * 8 + r8) + (size_t)fx * 16 + bx * 8);
            pw[0] = p[0]; pw[1] = p[1];
        }
    }
    LaneConst lc;
    lc.lane = lane;
    lc.quant = (int)c_quant_zz[lane];
    lc.zsrc = (int)c_zagzig[lane];
    {
        constexpr int kTrips = (BS_LUT_SIZE + kSplitThreads - 1) / kSplitThreads;
        uint16_t a[kTrips];
        uint32_t c[kTrips];
#pragma unroll
        for (int j = 0; j < kTrips; j++) {
            const int i = tid + j * kSplitThreads;
            a[j] = i < BS_LUT_SIZE ? c_ac_len16[i] : (uint16_t)0;
            c[j] = i < BS_LUT_SIZE ? c_ac_code[i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kTrips; j++) {
            const int i = tid + j * kSplitThreads;
            if (i < BS_LUT_SIZE) { l_len[i] = a[j]; l_code[i] = c[j]; }
        }
        if (tid < 96) sc[tid] = 0;
    }

    // ---- phase A: DCT of the segment's macroblocks, one wavefront each (mdec.c:605-643)
    if (wid < nm) {
        const int mbe = mb0 + wid;
        int16_t* tile = T + (size_t)wid * (kSplitWbufWords * 2);
        int16_t* z = Z + (size_t)wid * 6 * 64;
        if (lane < 48) {
            uint32_t px[8];
            if (blk < 2) {
                // NV21: Cr (V) at even bytes, Cb (U) at odd bytes of the chroma row (mdec.c:627-628)
                const int sh = 8 * blk;
                px[0] = (pw[0] >> sh) & 0xFFu; px[1] = (pw[0] >> (16 + sh)) & 0xFFu;
                px[2] = (pw[1] >> sh) & 0xFFu; px[3] = (pw[1] >> (16 + sh)) & 0xFFu;
                px[4] = (pw[2] >> sh) & 0xFFu; px[5] = (pw[2] >> (16 + sh)) & 0xFFu;
                px[6] = (pw[3] >> sh) & 0xFFu; px[7] = (pw[3] >> (16 + sh)) & 0xFFu;
            } else {
                px[0] = pw[0] & 0xFFu; px[1] = (pw[0] >> 8) & 0xFFu; px[2] = (pw[0] >> 16) & 0xFFu; px[3] = pw[0] >> 24;
                px[4] = pw[1] & 0xFFu; px[5] = (pw[1] >> 8) & 0xFFu; px[6] = (pw[1] >> 16) & 0xFFu; px[7] = pw[1] >> 24;
            }
            int d[8];
            // the row pass on raw pixels: the level shift only moves output 0 (fdct8_pk)
            fdct8_pk<false>(px[0] | px[1] << 16, px[2] | px[3] << 16, px[7] | px[6] << 16, px[5] | px[4] << 16, d);
#pragma unroll
            for (int c = 0; c < 8; c++) tile[blk * kTileStride + c * 8 + r8] = (int16_t)d[c];
        }
        wave_sync();
        if (lane < 48) {
            // lane = (block, column): the column's eight row outputs are 16 contiguous bytes
            const uint4 q = *(const uint4*)&tile[blk * kTileStride + r8 * 8];
            int d[8];
            fdct8_pk<true>(q.x, q.y, __builtin_amdgcn_alignbit(q.w, q.w, 16), __builtin_amdgcn_alignbit(q.z, q.z, 16), d);
#pragma unroll
            for (int v = 0; v < 8; v++) tile[blk * kTileStride + v * 8 + r8] = (int16_t)d[v];      // raster order (the row outputs have been read)
        }
        wave_sync();
#pragma unroll
        for (int b = 0; b < 6; b++) z[b * 64 + lane] = tile[b * kTileStride + lc.zsrc];
        const int q = quant_dc((int)tile[(lane < 6 ? lane : 0) * kTileStride]);       // mdec.c:447-449
        if (lane < 6) dcl[wid * 8 + lane] = (int16_t)q;
        if (CODEC != 0) {
            // v3: the block's DC term for everybody, two to a word, biased by 513 (-512 .. 510 -> 1 .. 1023: a word is never zero)
            const unsigned lo = (unsigned)(q + 513), hi = (unsigned)(__shfl(q, (lane | 1) & 63, 64) + 513);
            if (lane < 6 && !(lane & 1))
                __hip_atomic_store(&dcw[mbe * 3 + (lane >> 1)], lo | (hi << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    bool alive = true;
    if (CODEC != 0) {
        // ---- v3: every group needs every block's DC term (mdec.c:454-479): all of them read, then the three chains here
        bool got = true;
        for (int i = tid; i < nmb * 3; i += kSplitThreads) {
            const unsigned v = hidden(i / 3 / M) ? 0u : split_await(&dcw[i], pat);
            got = got && v != 0u;
            dcv[2 * i] = (int16_t)((int)(v & 0xFFFFu) - 513);
            dcv[2 * i + 1] = (int16_t)((int)(v >> 16) - 513);
        }
        if (!got) sc[SC_DEAD] = 1;
        __syncthreads();
        // Element i of a chain maps last -> new_last; both kinds are step functions, a chain is an inclusive scan under composition
        // (the frame kernel's DC pre-pass, restated: chunks of 512 elements over the wavefronts, A: chunk totals, B: scan of the
        // totals, C: the value entering each lane's run, then the run)
        constexpr int kPerLane = 8, kChunk = 64 * kPerLane;
        const int cc = (nmb + kChunk - 1) / kChunk, cy = (4 * nmb + kChunk - 1) / kChunk, n_chunks = 2 * cc + cy;
        auto chunk_of = [&](int q, int& chain, int& base, int& count) {
            chain = q < cc ? 0 : (q < 2 * cc ? 1 : 2);
            base = (q - (chain == 0 ? 0 : (chain == 1 ? cc : 2 * cc))) * kChunk;
            count = chain == 2 ? 4 * nmb : nmb;
        };
        auto element = [&](int chain, int i, bool live, int& idx) -> StepFn {
            idx = chain == 2 ? ((i >> 2) * 6 + 2 + (i & 3)) : (i * 6 + chain);
            const int dc = live ? (int)dcv[idx] : 0;
            StepFn fn;
            if ((dc & 3) == 2) {
                fn.thr = dc; fn.lo = dc + 2; fn.hi = dc - 2;
            } else {
                const int a = dc < 0 ? -dc : dc;
                const int rq = ((a + 2) >> 2) << 2;
                fn.thr = 0; fn.lo = fn.hi = dc < 0 ? -rq : rq;
            }
            if (!live) { fn.thr = -100000; fn.lo = fn.hi = 0; }
            return fn;
        };
        auto lane_total = [&](int chain, int base, int count) -> StepFn {
            const int i0 = base + lane * kPerLane;
            int idx;
            StepFn fn = element(chain, i0, i0 < count, idx);
#pragma unroll
            for (int j = 1; j < kPerLane; j++) fn = compose(fn, element(chain, i0 + j, i0 + j < count, idx));
            return fn;
        };
        for (int q = wid; q < n_chunks; q += kSplitWaves) {
            int chain, base, count;
            chunk_of(q, chain, base, count);
            StepFn fn = lane_total(chain, base, count);
            scan_stepfn(fn, lane);
            if (lane == 63) { dc_fn[4 * q + 0] = fn.thr; dc_fn[4 * q + 1] = fn.lo; dc_fn[4 * q + 2] = fn.hi; }
        }
        __syncthreads();
        if (wid < 3) {
            const int q0 = wid == 0 ? 0 : (wid == 1 ? cc : 2 * cc), nq = wid == 2 ? cy : cc;
            int carry = 0;
            for (int b0 = 0; b0 < nq; b0 += 64) {
                const int j = b0 + lane;
                StepFn fn;
                fn.thr = -100000; fn.lo = fn.hi = 0;
                if (j < nq) { fn.thr = dc_fn[4 * (q0 + j) + 0]; fn.lo = dc_fn[4 * (q0 + j) + 1]; fn.hi = dc_fn[4 * (q0 + j) + 2]; }
                scan_stepfn(fn, lane);
                const int cur = carry < fn.thr ? fn.lo : fn.hi;
                const int before = __builtin_amdgcn_update_dpp(carry, cur, 0x138, 0xF, 0xF, false);
                if (j < nq) dc_fn[4 * (q0 + j) + 3] = before;
                carry = __builtin_amdgcn_readlane(cur, 63);
            }
        }
        __syncthreads();
        for (int q = wid; q < n_chunks; q += kSplitWaves) {
            int chain, base, count;
            chunk_of(q, chain, base, count);
            StepFn fn = lane_total(chain, base, count);
            scan_stepfn(fn, lane);
            const int cin = dc_fn[4 * q + 3];
            const int after = cin < fn.thr ? fn.lo : fn.hi;
            int prev = __builtin_amdgcn_update_dpp(cin, after, 0x138, 0xF, 0xF, false);
            const int i0 = base + lane * kPerLane;
            int deltas[kPerLane], idxs[kPerLane];
#pragma unroll
            for (int j = 0; j < kPerLane; j++) {
                const bool live = i0 + j < count;
                const StepFn e = element(chain, i0 + j, live, idxs[j]);
                const int cur = prev < e.thr ? e.lo : e.hi;
                int delta = (cur - prev) >> 2;
                if (CODEC == 2) {                        // v3dc wrap (mdec.c:469-474)
                    if (delta < -0x80) delta += 0x100;
                    else if (delta > 0x80) delta -= 0x100;
                }
                deltas[j] = delta;
                prev = cur;
            }
            // (a lane's elements are read before any of them is overwritten: element() reads dcv[])
#pragma unroll
            for (int j = 0; j < kPerLane; j++)
                if (i0 + j < count) dcv[idxs[j]] = (int16_t)deltas[j];
        }
    }
    __syncthreads();
    alive = sc[SC_DEAD] == 0;

    // ---- phase B: the reference's loop, sixteen scales at a time
    const int wpm = kSplitWaves / M;             // wavefronts per macroblock
    const int m = wid / wpm, j = wid - m * wpm;
    float cf[6];
    int dc_bits = 0;
    if (m < nm) {
#pragma unroll
        for (int b = 0; b < 6; b++) cf[b] = lane == 0 ? 0.0f : (float)Z[((size_t)m * 6 + b) * 64 + lane];
        if (CODEC == 0) dc_bits = 60;
        else {
            int len = 0;
            uint32_t code;
            if (lane < 6) dc_code<CODEC>((int)dcv[(mb0 + m) * 6 + lane], lane >= 2, &c_dc_plen[0][0], &c_dc_prefix[0][0], len, code);
            dc_bits = wave::reduce_add(lane < 6 ? len : 0);
        }
    }
    uint32_t* mybuf = wbuf + (size_t)wid * kSplitWbufWords;
    // this wavefront's macroblock coded at `scale` into its buffer, from bit 0 (mdec.c:441-510)
    auto emit_mb = [&](int scale) {
        const QuantK k = make_quant(lc.quant, scale);
        // three blocks at a time: their codes first (independent chains of look-ups), then their positions, then the writes
        uint32_t pos = 0u;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            int len[3];
            uint32_t code[3];
#pragma unroll
            for (int t = 0; t < 3; t++) {
                const int b = 3 * h + t;
                const int q = quant_mag(cf[b], k);
                const uint64_t nzm = wave::ballot(q != 0);
                const int run = run_before(nzm, lc);
                const uint32_t neg = cf[b] < 0.0f ? 1u : 0u;
                const uint32_t entry = l_code[lut_index(q, run)];
                len[t] = (int)(entry >> 24);
                code[t] = (entry & 0x1FFFFu) | neg;
                if (len[t] == BS_ESCAPE_BITS) {
                    // escape: 000001, run, 10-bit level (mdec.c:258) clamped to -512 .. 510 (mdec.c:260-267)
                    const int lim = 510 + 2 * (int)neg;
                    const int qc = q > lim ? lim : q;
                    const int sv = neg ? -qc : qc;
                    code[t] = (1u << 16) | ((uint32_t)run << 10) | ((uint32_t)sv & 0x3FFu);
                }
                if (len[t] == 0) code[t] = 0u;
                if (lane == 0) {
                    if (CODEC == 0) { len[t] = 10; code[t] = (uint32_t)(int)dcl[m * 8 + b] & 0x3FFu; }     // mdec.c:451-453
                    else dc_code<CODEC>((int)dcv[(mb0 + m) * 6 + b], b >= 2, &c_dc_plen[0][0], &c_dc_prefix[0][0], len[t], code[t]);
                }
            }
            int incl[3];
#pragma unroll
            for (int t = 0; t < 3; t++) incl[t] = wave::inclusive_scan_add(len[t]);
#pragma unroll
            for (int t = 0; t < 3; t++) {
                const int total = __builtin_amdgcn_readlane(incl[t], 63);
                if (len[t]) split_put_bits(mybuf, pos + (uint32_t)(incl[t] - len[t]), len[t], code[t]);
                if (lane == 0) split_put_bits(mybuf, pos + (uint32_t)total, 2, 2u);      // end of block (mdec.c:501-503)
                pos += (uint32_t)total + 2u;
            }
        }
    };
    int answer = 0, rounds_used = 0, cbase = 0, ncand = 1;
    // Rounds of scales, ascending from 1 (so "the first that fits" needs no proof about scales not looked at): sixteen at a time --
    // but eight in the first round when the previous call's answer was at most 6: a wavefront then counts one scale instead of two,
    // and only a frame whose answer jumps beyond 8 pays a second round.
    const bool first8 = job.hint >= 1 && job.hint <= 6 && wpm <= 8;
    int base = 0, cnt = 0, abase = 0;
    for (int round = 0; round < kSplitRounds && alive && !bad_budget; round++, base += cnt) {
        rounds_used = round + 1;
        cnt = round == 0 && first8 ? 8 : kSplitRound;
        const int spw = cnt / wpm;               // scales per wavefront in this round
        if (m < nm) {
            for (int i = 0; i < spw; i++) {
                const int sl = j * spw + i, s = base + 1 + sl;
                if (s > 63) break;
                const QuantK k = make_quant(lc.quant, s);
                int bits = 0, nnz = 0;
#pragma unroll
                for (int b = 0; b < 6; b++) {
                    const int q = quant_mag(cf[b], k);
                    const uint64_t nzm = wave::ballot(q != 0);
                    nnz += (int)__builtin_popcountll(nzm);
                    bits += (int)(l_len[lut_index(q, run_before(nzm, lc))] & 0xFFu);
                }
                bits = wave::reduce_add(bits) + dc_bits + 12;          // + six end-of-block codes
                if (lane == 0) {
                    mbbits[m * kSplitRound + sl] = bits;
                    atomicAdd(&sc[SC_LBITS + sl], bits);
                    atomicAdd(&sc[SC_LNNZ + sl], nnz);
                }
            }
        }
        __syncthreads();
        unsigned long long* rslots = slots + ((size_t)round * nmb) * kSplitRound;      // this round's slots: [segment][16]
        if (tid < cnt && base + 1 + tid <= 63)
            __hip_atomic_store(&rslots[seg * kSplitRound + tid], (unsigned long long)(unsigned)sc[SC_LBITS + tid] | ((unsigned long long)(unsigned)sc[SC_LNNZ + tid] << 32),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (withheld) { alive = false; break; }          // (a withheld group leaves behind its round-0 sums, waiting for nobody)
        // While the sums travel: every wavefront codes its macroblock at ONE candidate scale into its own buffer -- the first wavefronts of a
        // macroblock at cbase, cbase + 1 -- at the previous call's answer (neighbouring frames of a video mostly agree), or around
        // what this segment's own bits would mean for the frame.  A hit leaves only the placing for after the answer.
        {
            int center = job.hint;
            if (center < base + 1 || center > base + cnt) {
                center = base + cnt;
                for (int sl = cnt - 1; sl >= 0; sl--)
                    if ((long long)sc[SC_LBITS + sl] * nmb <= (long long)(limit_bits - 10) * nm) center = base + 1 + sl;
            }
            // candidates per macroblock: two wavefronts build streams (the centre and the scale above it) while the others wait for
            // the sums; a macroblock with one wavefront to itself (M = 16) builds one and waits afterwards
            ncand = wpm >= 4 ? 2 : 1;
            cbase = center;
            if (cbase > base + cnt - ncand + 1) cbase = base + cnt - ncand + 1;
            if (cbase < base + 1) cbase = base + 1;
            if (j < ncand) {
                // (this wavefront's buffer: its transpose tile of phase A, or an earlier round's stream)
                for (int i = lane; i < kSplitWbufWords; i += 64) mybuf[i] = 0u;
                wave_sync();
                if (m < nm && cbase + j <= 63) emit_mb(cbase + j);
            }
        }
        if (wpm == 1 || j >= ncand) {
            // every group's sums of this round: waiting thread a looks at scale a % 16 of segments a / 16, a / 16 + stride, ...
            const int aw = wpm == 1 ? tid : (m * (wpm - ncand) + (j - ncand)) * 64 + lane;
            const int n_aw = wpm == 1 ? kSplitThreads : M * (wpm - ncand) * 64;
            const int sl = aw & (kSplitRound - 1);
            int tot = 0, nnz = 0, pre = 0;
            bool got = true;
            if (sl < cnt && base + 1 + sl <= 63)
                for (int g = aw >> 4; g < segs; g += n_aw / kSplitRound) {
                    const unsigned long long v = hidden(g) ? 0ull : split_await(&rslots[g * kSplitRound + sl], pat);
                    got = got && v != 0ull;
                    tot += (int)(unsigned)v;
                    nnz += (int)(unsigned)(v >> 32);
                    pre += g < seg ? (int)(unsigned)v : 0;
                }
            if (!got) sc[SC_DEAD] = 1;
            tot += __shfl_xor(tot, 16, 64); nnz += __shfl_xor(nnz, 16, 64); pre += __shfl_xor(pre, 16, 64);
            tot += __shfl_xor(tot, 32, 64); nnz += __shfl_xor(nnz, 32, 64); pre += __shfl_xor(pre, 32, 64);
            if (lane < kSplitRound) { atomicAdd(&sc[SC_TOT + lane], tot); atomicAdd(&sc[SC_NNZ + lane], nnz); atomicAdd(&sc[SC_PRE + lane], pre); }
        }
        __syncthreads();
        alive = sc[SC_DEAD] == 0;
        {
            const bool fits = lane < cnt && base + 1 + lane <= 63 && (long long)sc[SC_TOT + lane] + 10 <= (long long)limit_bits;
            const uint64_t fm = wave::ballot(fits);
            answer = fm ? base + 1 + (int)__builtin_ctzll(fm) : 0;
        }
        abase = base;
        if (answer || !alive) break;
        __syncthreads();
        if (tid < 80) sc[tid] = 0;          // the round's sums
        __syncthreads();
    }

    // ---- phase C: this segment's macroblocks, shifted to their place in the frame image
    if (answer && alive) {
        const int sl = answer - abase - 1;
        const bool hit = answer >= cbase && answer < cbase + ncand;
        if (m < nm && j == (hit ? answer - cbase : 0)) {
            if (!hit) {
                for (int i = lane; i < kSplitWbufWords; i += 64) mybuf[i] = 0u;
                wave_sync();
                emit_mb(answer);
            }
            uint32_t nbits = (uint32_t)mbbits[m * kSplitRound + sl];
            if (mb0 + m == nmb - 1) {
                // end-of-frame code behind the frame's last macroblock (mdec.c:647-651,710)
                if (lane == 0) split_put_bits(mybuf, nbits, 10, CODEC == 0 ? 0x1FFu : 0x3FFu);
                nbits += 10u;
            }
            uint32_t P = 64u + (uint32_t)sc[SC_PRE + sl];          // image bit of the macroblock's first bit (two header dwords in front)
            for (int i = 0; i < m; i++) P += (uint32_t)mbbits[i * kSplitRound + sl];
            const uint32_t sh = P & 31u;
            const int g0 = (int)(P >> 5), ndw = (int)((sh + nbits + 31u) >> 5);
            uint32_t seen = 0u;
            for (int i = lane; i < ndw; i += 64) {
                // image dword g0 + i = buffer bits [32 i - sh, 32 i - sh + 32): the funnel of buffer dwords i - 1 and i
                const uint32_t prv = i > 0 ? mybuf[i - 1] : 0u, cur = mybuf[i];
                const uint32_t v = __builtin_amdgcn_alignbit(prv, cur, sh);
                if (v && g0 + i < job.img_words) seen |= __hip_atomic_fetch_or(&img[g0 + i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (seen == 0xFFFFFFFFu) sc[SC_SINK] = 1;          // (the ORs return: a wavefront that has their values knows they are performed)
        }
    }

    // ---- the frame's last segment's group completes the frame, once every group has said it is done: a word per group (a counter
    //      all groups add to is served one addition after the other at the memory side: the last of 150 arrivals waited ~1.5 us)
    split_drain();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(&done[seg], alive ? 1u : 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seg != segs - 1) { leave(1u); return; }
    {
        bool bad = false;
        for (int i = tid; i < segs; i += kSplitThreads) bad = bad || (hidden(i) ? 0u : split_await(&done[i], pat)) != 1u;      // (0: the watchdog; 2: a group it released)
        if (bad) sc[SC_DEAD] = 2;
    }
    __syncthreads();
    uint8_t* outp = job.out + (size_t)f * job.out_stride;
    uint32_t* o32 = (uint32_t*)outp;
    const bool tripped = sc[SC_DEAD] != 0;
    if (tripped && tid == 0) atomicAdd(job.lost, 1u);
    if (!answer || tripped) {
        // nothing fits (the reference asserts, mdec.c:723): quant_scale 64 -- or the watchdog gave up: PSXHIP_MDEC_QS_RELEASED, which
        // says nothing about the frame (the host paths encode it again with the frame kernel).  Zero output either way.
        if (!bad_budget) {
            for (int i = tid; i < (max_size >> 2); i += kSplitThreads) row_store(&o32[i], 0u);
            if (tid < (max_size & 3)) outp[(max_size & ~3) + tid] = 0;
        }
        const uint32_t qs = tripped && !bad_budget ? (uint32_t)PSXHIP_MDEC_QS_RELEASED : 64u;
        if (tid < 4) row_store((uint32_t*)&job.results[f] + tid, tid == 0 ? qs : 0u);
    } else {
        const int sl = answer - abase - 1;
        const int total_bits = sc[SC_TOT + sl] + 10, nnz = sc[SC_NNZ + sl];
        int hwords = nnz + 2 * nmb * 6 + 2;                      // mdec.c:497,507,719
        hwords = (hwords + 0x3F) & ~0x3F;                        // mdec.c:726
        const int blocks_used = (hwords + 1) >> 1;               // mdec.c:733
        int bytes_used = 8 + 2 * ((total_bits + 15) >> 4);
        bytes_used = (bytes_used + 3) & ~3;                      // mdec.c:736
        const int full = max_size >> 2, tail = max_size & 3;
        for (int i = tid; i < full + (tail ? 1 : 0); i += kSplitThreads) {
            uint32_t v = i < job.img_words ? ld_agent(&img[i]) : 0u;
            // image dwords hold two MSB-first 16-bit words; each is stored low byte first (mdec.c:321-333): rotate by 16
            uint32_t w = (v >> 16) | (v << 16);
            if (i == 0) w = ((uint32_t)blocks_used & 0xFFFFu) | (0x3800u << 16);                         // mdec.c:739-746
            if (i == 1) w = ((uint32_t)answer & 0xFFFFu) | ((CODEC == 0 ? 2u : 3u) << 16);              // mdec.c:747-754
            if (i < full) row_store(&o32[i], w);
            else for (int b = 0; b < tail; b++) outp[4 * i + b] = (uint8_t)(w >> (8 * b));
        }
        static_assert(sizeof(psxhip_mdec_result_t) == 16, "the result is stored as four words");
        if (tid < 4) row_store((uint32_t*)&job.results[f] + tid, (uint32_t)(tid == 0 ? answer : (tid == 1 ? bytes_used : (tid == 2 ? blocks_used : hwords))));
    }
    if (job.done_flag) {
        // the caller's CPU waits on this word instead of on the stream: row and result first (they are stores to the same host block;
        // every wavefront waits for its stores' acknowledgements, then the flag goes out behind them), then the flag -- the workspace is tidied after it
        // (the row's words are write-through stores: a wavefront whose stores are acknowledged has them in the host's memory; the
        //  odd bytes of a budget that is no multiple of 4 are plain byte stores and need the caches written back)
        if (max_size & 3) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        split_drain();
        __syncthreads();
        if (tid == 0) __hip_atomic_store(job.done_flag, job.done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // the workspace goes back to zero for the next launch: device-scope stores (the next launch's device-scope loads and ORs are
    // served at the memory side; a plain store could sit in this XCD's L2)
    // (WITHHOLD with `residue`: the withheld segment's words are left as a group that comes late leaves them)
    const int keep = wh && job.wh_residue ? job.wh_seg : -1;
    for (int i = tid; i < job.img_words; i += kSplitThreads) __hip_atomic_store(&img[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int r = 0; r < rounds_used; r++)
        for (int i = tid; i < segs * kSplitRound; i += kSplitThreads)
            if (i / kSplitRound != keep) __hip_atomic_store(&slots[((size_t)r * nmb) * kSplitRound + i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (CODEC != 0)
        for (int i = tid; i < nmb * 3; i += kSplitThreads)
            if (i / 3 / M != keep) __hip_atomic_store(&dcw[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int i = tid; i < segs; i += kSplitThreads)
        if (i != keep) __hip_atomic_store(&done[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    leave(tripped ? 0x10001u : 1u);
}

}  // namespace

extern "C" hipError_t psxhip_mdec_split_launch(const psxhip_mdec_split_t* a) {
    SplitJob job;
    memset(&job, 0, sizeof job);
    job.frames = a->d_frames; job.out = a->d_out; job.results = a->d_results; job.max_sizes = a->d_frame_max_sizes;
    job.frame_stride = a->frame_stride; job.out_stride = a->out_stride;
    job.width = a->width; job.height = a->height; job.nx = a->width / 16; job.ny = a->height / 16; job.nmb = job.nx * job.ny;
    job.n_frames = a->n_frames; job.uniform_max_size = a->uniform_max_size; job.max_frame_size = a->max_frame_size;
    job.seg_mbs = a->geo.seg_mbs; job.segs = a->geo.segs;
    job.ws = (unsigned char*)a->d_ws; job.ws_stride = a->geo.ws_stride;
    job.ws_slots = a->geo.ws_slots; job.ws_dcq = a->geo.ws_dcq; job.ws_img = a->geo.ws_img; job.ws_done = a->geo.ws_done; job.img_words = a->geo.img_words;
    job.lost = a->d_lost;
    job.done_flag = a->d_done_flag; job.done_seq = a->done_seq; job.hint = a->hint;
    job.patience = a->patience ? a->patience : kSplitPatience;
    job.wh_frame = a->wh_frame; job.wh_seg = a->wh_seg < a->geo.segs ? a->wh_seg : -1; job.wh_residue = a->wh_residue;
    const dim3 grid((unsigned)(a->geo.segs * a->n_frames)), block((unsigned)kSplitThreads);
    hipStream_t st = (hipStream_t)a->stream;
    switch (a->codec) {
    case 0: hipLaunchKernelGGL((mdec_split_kernel<0>), grid, block, a->geo.lds_bytes, st, job); break;
    case 1: hipLaunchKernelGGL((mdec_split_kernel<1>), grid, block, a->geo.lds_bytes, st, job); break;
    default: hipLaunchKernelGGL((mdec_split_kernel<2>), grid, block, a->geo.lds_bytes, st, job); break;
    }
    return hipGetLastError();
}
