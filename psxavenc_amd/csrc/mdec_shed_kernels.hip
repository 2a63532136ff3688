// mdec_shed_kernels.hip -- "psxhip MDEC shed v1" on the device (the rule's text is mdec_shed_core.h): after a plain
// encode chose scale N for a frame, try it at M = N - 1 with small AC levels zeroed until it fits, and keep that when its distortion
// in the coefficient domain is below the plain encode's.
//
//   analyse  one wavefront per macroblock, lane = zig-zag position: gather, FDCT, the levels at M and N, and per lane the sums of
//            D_plain, D at step 0, the AC bits and count at step 0, and for each magnitude class the change in bits, count and
//            distortion that the step at this lane's position makes -- prev / next survivor from ballot masks, nothing crosses lanes
//            but the next survivor's magnitude.  Reduced per workgroup in LDS, then added to the frame's sums with 64-bit integer
//            atomics: exact, whatever the order.  All 63 K candidates cost this one pass.
//   decide   one workgroup per frame: the DC codes (a serial chain per component in v3), the running sums over t = 1 .. 63 K, first
//            fit, acceptance; the result and the refine record; a refined frame's row is zeroed and gets its header here.
//   emit     one workgroup per refined frame: block bit lengths at t*, their offsets in the encoder's block order, and the codes
//            OR-ed into the zeroed row (32-bit atomics; the one halfword a budget of 4 k + 2 or 4 k + 3 bytes has behind its last whole
//            dword is collected in the workspace and stored on its own, so that nothing outside the budget is touched).
//
// Throughput is unmeasured (tools/gpu_mdec_shed_probe.py records it): a launch of a few small frames fills a few CUs, the FDCT runs on
// 48 of a wavefront's 64 lanes without the frame kernel's packed arithmetic, and the emit takes one workgroup per frame.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bs_vlc_lut.h"

__device__ uint16_t shed_dev_ac_len16_lut[BS_LUT_SIZE];
__device__ uint32_t shed_dev_ac_code_lut[BS_LUT_SIZE];
__device__ uint8_t shed_dev_zagzig[64], shed_dev_quant_zz[64];
__device__ uint8_t shed_dev_dc_chroma_prefix[8], shed_dev_dc_chroma_plen[8], shed_dev_dc_luma_prefix[8], shed_dev_dc_luma_plen[8];

#define SHED_DEVICE
#include "mdec_shed_core.h"
#include "psxhip_shed_internal.h"
#include "wave_ops.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
static_assert(kShedAnalyseMbs % kWaves == 0, "a workgroup's macroblocks are dealt evenly to its wavefronts");
static_assert(kShedRows == 13, "mdec_shed_workspace sizes the sums for 13 rows");

struct FrameView {
    const uint8_t* px;
    uint8_t* row;
    int budget;             // 0: not a budget this call takes
    int scale;              // the plain result's quant_scale
};

__device__ FrameView frame_view(const psxhip_mdec_shed_job_t& j, int f) {
    FrameView v;
    v.px = j.d_frames + (size_t)f * j.frame_stride;
    v.row = j.d_out + (size_t)f * j.out_stride;
    const int b = j.d_frame_max_sizes ? j.d_frame_max_sizes[f] : j.uniform_max_size;
    v.budget = (b >= 8 && b <= j.max_frame_size && (size_t)b <= j.out_stride) ? b : 0;
    v.scale = j.d_results[f].quant_scale;
    return v;
}

// Macroblock e (the encoder's order: column by column) of the frame into the wavefront's tile: six blocks of 64 coefficients in
// raster order.  Every wavefront of the workgroup calls this the same number of times (it holds workgroup barriers); e < 0: idle.
__device__ void macroblock_coefs(const psxhip_mdec_shed_job_t& j, const uint8_t* px, int e, int16_t* tile) {
    const int lane = wave::lane_id();
    if (e >= 0) {
        const int ny = j.height >> 4, w = j.width;
        const int fx = e / ny, fy = e - fx * ny;
        const int y = lane >> 3, x = lane & 7;
        const uint8_t* c = px + (size_t)w * j.height + (size_t)w * (fy * 8 + y) + 2 * (fx * 8 + x);
        const uint8_t* l = px + (size_t)w * (fy * 16 + y) + fx * 16 + x;
        tile[0 * 64 + lane] = (int16_t)(c[0] - 128);
        tile[1 * 64 + lane] = (int16_t)(c[1] - 128);
        tile[2 * 64 + lane] = (int16_t)(l[0] - 128);
        tile[3 * 64 + lane] = (int16_t)(l[8] - 128);
        tile[4 * 64 + lane] = (int16_t)(l[8 * w] - 128);
        tile[5 * 64 + lane] = (int16_t)(l[8 * w + 8] - 128);
    }
    __syncthreads();
    if (e >= 0 && lane < 48) shed_fdct_1d(tile + (lane >> 3) * 64 + (lane & 7) * 8, 1, false);
    __syncthreads();
    if (e >= 0 && lane < 48) shed_fdct_1d(tile + (lane >> 3) * 64 + (lane & 7), 8, true);
    __syncthreads();
}

// ------------------------------------------------------------------------------------------ analyse
__global__ __launch_bounds__(kThreads) void mdec_shed_analyse_kernel(const psxhip_mdec_shed_job_t j) {
    __shared__ int16_t tiles[kWaves][6 * 64];
    __shared__ unsigned long long sums[kShedRows][64];
    const int f = blockIdx.x / j.groups_per_frame, g = blockIdx.x - f * j.groups_per_frame;
    const FrameView v = frame_view(j, f);
    if (!v.budget || !shed_frame_eligible(v.scale)) return;          // (uniform over the workgroup)
    const int lane = wave::lane_id(), wv = threadIdx.x >> 6;
    const int M = v.scale - 1, N = v.scale;
    for (int i = threadIdx.x; i < kShedRows * 64; i += kThreads) (&sums[0][0])[i] = 0;

    long long d_plain = 0, d_base = 0, dist[kShedMaxMagnitude] = {0, 0, 0};
    int bits0 = 0, nnz0 = 0, dbits[kShedMaxMagnitude] = {0, 0, 0}, dcnt[kShedMaxMagnitude] = {0, 0, 0};
    const int zz = shed_dev_zagzig[lane], q = shed_dev_quant_zz[lane];
    int16_t* dc_level = (int16_t*)(j.d_ws + (size_t)f * j.ws.stride + j.ws.dc_level);

    for (int k = 0; k < kShedAnalyseMbs / kWaves; k++) {
        int e = g * kShedAnalyseMbs + k * kWaves + wv;
        if (e >= j.nmb) e = -1;
        macroblock_coefs(j, v.px, e, tiles[wv]);
        if (e < 0) continue;
        for (int i = 0; i < 6; i++) {
            const int F = tiles[wv][i * 64 + zz];
            if (lane == 0) dc_level[e * 6 + i] = (int16_t)shed_dc_level(F);
            const int lvM = lane ? shed_ac_level(F, lane, M) : 0, lvN = lane ? shed_ac_level(F, lane, N) : 0;
            const int a = lvM < 0 ? -lvM : lvM;
            if (lane) {
                d_plain += shed_sq((long long)F - lvN * q * N);
                d_base += shed_sq((long long)F - lvM * q * M);
            }
            const uint64_t nz = wave::ballot(a >= 1);
            int run;
            if (a) {
                shed_neighbours(lane, nz, 0, &run);
                bits0 += shed_len(run, a);
                nnz0++;
            }
            uint64_t ge = nz;
#pragma unroll
            for (int m = 1; m <= kShedMaxMagnitude; m++) {
                const uint64_t gt = wave::ballot(a > m);
                const int next = shed_neighbours(lane, ge, gt, &run);
                const int a_next = __shfl(a, next, 64);
                if (a == m) {
                    dbits[m - 1] += shed_bit_delta(lane, m, run, next, a_next);
                    dcnt[m - 1]++;
                    dist[m - 1] += shed_dist_gain(F, lvM * q * M);
                }
                ge = gt;
            }
        }
    }
    __syncthreads();
    atomicAdd(&sums[SHED_D_PLAIN][lane], (unsigned long long)d_plain);
    atomicAdd(&sums[SHED_D_BASE][lane], (unsigned long long)d_base);
    atomicAdd(&sums[SHED_BITS0][lane], (unsigned long long)(long long)bits0);
    atomicAdd(&sums[SHED_NNZ0][lane], (unsigned long long)(long long)nnz0);
#pragma unroll
    for (int m = 0; m < kShedMaxMagnitude; m++) {
        atomicAdd(&sums[SHED_DBITS + m][lane], (unsigned long long)(long long)dbits[m]);
        atomicAdd(&sums[SHED_DCNT + m][lane], (unsigned long long)(long long)dcnt[m]);
        atomicAdd(&sums[SHED_DDIST + m][lane], (unsigned long long)dist[m]);
    }
    __syncthreads();
    unsigned long long* acc = (unsigned long long*)(j.d_ws + (size_t)f * j.ws.stride + j.ws.acc);
    for (int i = threadIdx.x; i < kShedRows * 64; i += kThreads) {
        const unsigned long long s = (&sums[0][0])[i];
        if (s) atomicAdd(&acc[i], s);
    }
}

// ------------------------------------------------------------------------------------------ decide
__global__ __launch_bounds__(kThreads) void mdec_shed_decide_kernel(const psxhip_mdec_shed_job_t j) {
    __shared__ long long dc_bits[3];
    __shared__ int refined, blocks_used;
    const int f = blockIdx.x, nblk = j.nmb * 6;
    const FrameView v = frame_view(j, f);
    uint8_t* ws = j.d_ws + (size_t)f * j.ws.stride;
    psxhip_mdec_shed_decision_t* dec = (psxhip_mdec_shed_decision_t*)(ws + j.ws.decision);
    const bool eligible = v.budget && shed_frame_eligible(v.scale);
    if (!eligible) {
        if (threadIdx.x == 0 && j.d_refine) j.d_refine[f] = psxhip_mdec_refine_t{0, 0, 0, 0};
        return;
    }
    const int16_t* dc_level = (const int16_t*)(ws + j.ws.dc_level);
    uint32_t* dc_code = (uint32_t*)(ws + j.ws.dc_code);
    if (threadIdx.x < 3) dc_bits[threadIdx.x] = 0;
    if (j.codec == 0) {
        int last = 0;
        for (int b = threadIdx.x; b < nblk; b += kThreads) dc_code[b] = shed_dc_code(0, 2, dc_level[b], &last);
        if (threadIdx.x == 0) dc_bits[0] = 10ll * nblk;
    } else if (threadIdx.x < 3) {
        // v3: a component's DC is coded against its own running value, whose rounding feeds back -- one serial chain each
        const int comp = threadIdx.x;
        int last = 0;
        long long bits = 0;
        for (int e = 0; e < j.nmb; e++)
            for (int i = comp < 2 ? comp : 2; i < (comp < 2 ? comp + 1 : 6); i++) {
                const uint32_t c = shed_dc_code(j.codec, comp, dc_level[e * 6 + i], &last);
                dc_code[e * 6 + i] = c;
                bits += c >> 24;
            }
        dc_bits[comp] = bits;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const ShedDecision d = shed_decide((const int64_t*)(ws + j.ws.acc), dc_bits[0] + dc_bits[1] + dc_bits[2], nblk, v.budget, j.max_magnitude);
        int32_t res[4] = {0, 0, 0, 0};
        if (d.refined) {
            shed_result(d, nblk, v.scale - 1, res);
            j.d_results[f] = psxhip_mdec_result_t{res[0], res[1], res[2], res[3]};
        }
        dec->step = d.step;
        dec->blocks_used = res[2];
        dec->bits = d.bits;
        dec->tail = 0;
        if (j.d_refine) j.d_refine[f] = psxhip_mdec_refine_t{d.step, d.count, d.d_plain, d.d_shed};
        refined = d.refined;
        blocks_used = res[2];
    }
    __syncthreads();
    if (!refined) return;
    // the row: zero up to the budget, then the header (the emit kernel ORs the codes in)
    uint32_t* row32 = (uint32_t*)v.row;
    const int dwords = v.budget >> 2;
    for (int i = threadIdx.x; i < dwords; i += kThreads) row32[i] = i >= 2 ? 0u : (i == 0 ? ((uint32_t)blocks_used & 0xFFFFu) | 0x38000000u
                                                                                     : (uint32_t)(v.scale - 1) | (j.codec == 0 ? 2u : 3u) << 16);
    if (threadIdx.x < (v.budget & 3)) v.row[(dwords << 2) + threadIdx.x] = 0;
}

// ------------------------------------------------------------------------------------------ emit
struct RowSink {
    uint32_t* row32;
    unsigned int* tail;
    int whole;              // halfwords in the budget's whole dwords
    __device__ void or16(int hw, uint32_t v) {
        if (hw < whole) atomicOr(row32 + (hw >> 1), v << ((hw & 1) * 16));
        else atomicOr(tail, v);          // (a fitting stream reaches at most the one halfword behind them)
    }
};

// the shed levels of a block at step t: this lane's level, the masks of the survivors, and the bits of this lane's code
__device__ int shed_lane_code(int F, int lane, int M, int step, int* level) {
    const int lv = lane ? shed_ac_level(F, lane, M) : 0;
    const int a = lv < 0 ? -lv : lv;
    const bool keep = a && !shed_gone(a, lane, step);
    const uint64_t nz = wave::ballot(keep);
    *level = keep ? lv : 0;
    if (!keep) return 0;
    int run;
    shed_neighbours(lane, nz, 0, &run);
    return run;
}

__global__ __launch_bounds__(kThreads) void mdec_shed_emit_kernel(const psxhip_mdec_shed_job_t j) {
    __shared__ int16_t tiles[kWaves][6 * 64];
    __shared__ unsigned int part[kThreads];
    const int f = blockIdx.x, nblk = j.nmb * 6;
    uint8_t* ws = j.d_ws + (size_t)f * j.ws.stride;
    psxhip_mdec_shed_decision_t* dec = (psxhip_mdec_shed_decision_t*)(ws + j.ws.decision);
    const int step = dec->step;
    if (step == 0) return;                                           // (uniform: not refined, or not taken at all)
    const FrameView v = frame_view(j, f);                            // (its scale is M already: the decide kernel rewrote the result)
    const int M = v.scale;
    const int lane = wave::lane_id(), wv = threadIdx.x >> 6;
    const int zz = shed_dev_zagzig[lane];
    const uint32_t* dc_code = (const uint32_t*)(ws + j.ws.dc_code);
    uint32_t* block_off = (uint32_t*)(ws + j.ws.block_off);
    const int trips = (j.nmb + kWaves - 1) / kWaves;

    // bits per block
    for (int k = 0; k < trips; k++) {
        int e = k * kWaves + wv;
        if (e >= j.nmb) e = -1;
        macroblock_coefs(j, v.px, e, tiles[wv]);
        if (e < 0) continue;
        for (int i = 0; i < 6; i++) {
            int lv;
            const int run = shed_lane_code(tiles[wv][i * 64 + zz], lane, M, step, &lv);
            const int bits = wave::reduce_add(lv ? shed_len(run, lv < 0 ? -lv : lv) : 0);
            if (lane == 0) block_off[e * 6 + i] = (dc_code[e * 6 + i] >> 24) + (uint32_t)bits + 2u;
        }
    }
    __threadfence();
    __syncthreads();
    // ... to offsets, in the encoder's block order: each thread a stretch of blocks
    const int per = (nblk + kThreads - 1) / kThreads, b0 = threadIdx.x * per, b1 = b0 + per < nblk ? b0 + per : nblk;
    unsigned int sum = 0;
    for (int b = b0; b < b1; b++) sum += block_off[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int run = 0;
        for (int i = 0; i < kThreads; i++) {
            const unsigned int s = part[i];
            part[i] = run;
            run += s;
        }
    }
    __syncthreads();
    sum = part[threadIdx.x];
    for (int b = b0; b < b1; b++) {
        const unsigned int s = block_off[b];
        block_off[b] = sum;
        sum += s;
    }
    __threadfence();
    __syncthreads();

    // the codes
    RowSink sink = {(uint32_t*)v.row, &dec->tail, (v.budget >> 2) * 2};
    for (int k = 0; k < trips; k++) {
        int e = k * kWaves + wv;
        if (e >= j.nmb) e = -1;
        macroblock_coefs(j, v.px, e, tiles[wv]);
        if (e < 0) continue;
        for (int i = 0; i < 6; i++) {
            int lv;
            const int run = shed_lane_code(tiles[wv][i * 64 + zz], lane, M, step, &lv);
            const uint32_t code = lane ? (lv ? shed_ac_code(run, lv) : 0u) : dc_code[e * 6 + i];
            const int len = (int)(code >> 24);
            const int end = wave::inclusive_scan_add(len);
            const long long at = (long long)block_off[e * 6 + i] + end - len;
            if (len) shed_put(sink, at, len, code & 0xFFFFFFu);
            if (lane == 63) shed_put(sink, at + len, 2, 2u);         // end of block
        }
    }
    if (threadIdx.x == 0) shed_put(sink, dec->bits - 10, 10, shed_end_code(j.codec));
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0 && (v.budget & 2)) *(volatile uint16_t*)(v.row + (v.budget & ~3)) = (uint16_t)__hip_atomic_load(&dec->tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

extern "C" hipError_t psxhip_mdec_shed_upload_tables(void) {
    hipError_t e;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(shed_dev_ac_len16_lut), bs_ac_len16_lut, sizeof(bs_ac_len16_lut))) != hipSuccess) return e;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(shed_dev_ac_code_lut), bs_ac_code_lut, sizeof(bs_ac_code_lut))) != hipSuccess) return e;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(shed_dev_zagzig), bs_zagzig, sizeof(bs_zagzig))) != hipSuccess) return e;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(shed_dev_quant_zz), bs_quant_zz, sizeof(bs_quant_zz))) != hipSuccess) return e;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(shed_dev_dc_chroma_prefix), bs_dc_chroma_prefix, 8)) != hipSuccess) return e;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(shed_dev_dc_chroma_plen), bs_dc_chroma_plen, 8)) != hipSuccess) return e;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(shed_dev_dc_luma_prefix), bs_dc_luma_prefix, 8)) != hipSuccess) return e;
    return hipMemcpyToSymbol(HIP_SYMBOL(shed_dev_dc_luma_plen), bs_dc_luma_plen, 8);
}

// the three kernels over n_frames frames, in order on `stream`; the workspace's sums are zero
extern "C" hipError_t psxhip_mdec_shed_launch(const psxhip_mdec_shed_job_t* j, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mdec_shed_analyse_kernel, dim3((unsigned)(j->n_frames * j->groups_per_frame)), dim3(kThreads), 0, s, *j);
    hipLaunchKernelGGL(mdec_shed_decide_kernel, dim3((unsigned)j->n_frames), dim3(kThreads), 0, s, *j);
    hipLaunchKernelGGL(mdec_shed_emit_kernel, dim3((unsigned)j->n_frames), dim3(kThreads), 0, s, *j);
    return hipGetLastError();
}
