// mdec_decode_kernels.hip -- the decoder's kernels for gfx950: bitstream -> levels (mdec_parse_kernel), levels -> NV21 pixels
// (mdec_reconstruct_kernel, "psxhip MDEC reconstruct v1"), and the per-frame sum of squared errors of two
// sets of frames (mdec_sse_kernel).
//
// Parse.  A frame is ONE serial chain of variable-length codes: where a code starts is known only once the one before it has been
// read.  So the parallelism is across frames -- one wavefront per frame -- and inside a 64-bit window of the stream: each lane
// fetches the 32 bits that start at ITS bit offset of the window and looks up the AC code (and, for v3, the DC size class) that
// would start there, 64 table lookups in LDS at once; then a wave-uniform walk picks the offsets where codes really start, taking
// each lane's bits and table entry with v_readlane and running mdec_parse_step() (mdec_parse.h, the text the CPU test runs) on
// scalar registers.  The lookup latency is paid once per window instead of once per code.  The block being read lives in one VGPR,
// lane k holding coefficient k; an end of block stores it as one 128-byte row, zeros included.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BS_DEC_TABLE static __device__ const
#include "mdec_parse.h"
#include "psxhip_decode_internal.h"

namespace {

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__global__ __launch_bounds__(64) void mdec_parse_kernel(const psxhip_mdec_parse_job_t j) {
    __shared__ uint16_t s_ac[BS_DEC_AC_SIZE];
    __shared__ uint16_t s_dc[256];                                   // luma | chroma << 8
    const int lane = (int)threadIdx.x;
    for (int i = lane; i < BS_DEC_AC_SIZE; i += 64) s_ac[i] = bs_dec_ac[i];
    for (int i = lane; i < 256; i += 64) s_dc[i] = (uint16_t)(bs_dec_dc_luma[i] | (bs_dec_dc_chroma[i] << 8));
    __syncthreads();

    const int f = (int)blockIdx.x;
    const uint8_t* bs = j.d_bs + (size_t)f * j.bs_stride;
    int64_t size = j.d_sizes ? (int64_t)uniform(j.d_sizes[f]) : (int64_t)j.uniform_size;
    if (size > (int64_t)j.bs_stride) size = (int64_t)j.bs_stride;
    uint32_t h0 = 0, h1 = 0;
    if (size >= 8) {
        h0 = (uint32_t)uniform((int)((const uint32_t*)bs)[0]);
        h1 = (uint32_t)uniform((int)((const uint32_t*)bs)[1]);
    }
    MdecParse st;
    mdec_parse_begin(st, h0, h1, size, j.nblk, j.wrap);
    const uint8_t* payload = bs + 8;
    int16_t* out = j.d_levels ? j.d_levels + (size_t)f * (size_t)j.nblk * 64 : nullptr;
    const bool v3 = st.version == 3;
    int lv = 0;                                                       // coefficient `lane` of the block being read

    while (st.status == MDEC_PARSE_OK && st.phase != MDEC_PHASE_DONE) {
        const uint32_t base = st.pos;
        const uint32_t v_lane = mdec_parse_peek32(payload, st.nbytes, base + (uint32_t)lane);
        uint32_t e_lane = s_ac[mdec_parse_ac_index(v_lane)];
        if (v3) e_lane |= (uint32_t)s_dc[mdec_parse_dc_index(v_lane)] << 16;
        while (st.status == MDEC_PARSE_OK && st.phase != MDEC_PHASE_DONE && st.pos - base < 64u) {
            const int at = (int)(st.pos - base);
            const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)v_lane, at);
            const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)e_lane, at);
            const MdecSym s = mdec_parse_step(st, v, e & 0xFFFFu, e >> 16);
            if (s.kind == MDEC_SYM_DC) {
                lv = lane == 0 ? s.level : 0;
            } else if (s.kind == MDEC_SYM_AC) {
                lv = lane == s.k ? s.level : lv;
            } else if (s.kind == MDEC_SYM_EOB) {
                if (out) out[(size_t)s.blk * 64 + lane] = (int16_t)lv;
            }
        }
    }
    if (lane == 0) {
        psxhip_mdec_decoded_t d;
        d.status = st.status;
        d.quant_scale = st.quant_scale;
        d.version = st.version;
        d.bits_consumed = st.status == MDEC_PARSE_OK ? (int32_t)st.pos : 0;
        j.d_decoded[f] = d;
    }
}

// ---- psxhip MDEC reconstruct v1: one wavefront per macroblock, lane = pixel (y, x) of the 8x8 block, six blocks in turn.
// Rows then columns, the partner values fetched across lanes; every product and sum fits 32 bits (tests/test_mdec_recon_ref.py
// computes the worst case).
constexpr int kSat = 1 << 14;

__global__ __launch_bounds__(256) void mdec_reconstruct_kernel(const psxhip_mdec_recon_job_t j) {
    const int lane = (int)(threadIdx.x & 63u);
    const int nx = j.width / 16, ny = j.height / 16, nmb = nx * ny;
    const int64_t g = (int64_t)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (g >= (int64_t)j.n_frames * nmb) return;
    const int f = uniform((int)(g / nmb)), m = uniform((int)(g % nmb));
    if (j.d_decoded[f].status != PSXHIP_DEC_OK) return;
    const uint32_t qs = (uint32_t)j.d_decoded[f].quant_scale;
    const int scale = (int)(qs < (uint32_t)kSat ? qs : (uint32_t)kSat);      // beyond it every non-zero product saturates anyway
    const int fx = m / ny, fy = m % ny;
    const int y = lane >> 3, x = lane & 7;
    int cx[8], cy[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
        cx[u] = bs_dec_idct[u * 8 + x];
        cy[u] = bs_dec_idct[u * 8 + y];
    }
    const int z = bs_dec_zigzag[lane];
    const int q = lane == 0 ? 16 : (int)bs_dec_quant[lane] * scale;            // <= 83 * 2^14
    const int16_t* lvp = j.d_levels + ((size_t)f * nmb + m) * 6 * 64;
    uint8_t* frame = j.d_frames + (size_t)f * j.frame_stride;
    const size_t w = (size_t)j.width;
    int cr = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        int f8 = (int)lvp[i * 64 + z] * q;
        f8 = f8 < -kSat ? -kSat : (f8 > kSat - 1 ? kSat - 1 : f8);
        int acc = 1 << 14;
#pragma unroll
        for (int u = 0; u < 8; u++) acc += __shfl(f8, (lane & 56) | u, 64) * cx[u];
        const int t = acc >> 15;
        acc = 1 << 15;
#pragma unroll
        for (int v = 0; v < 8; v++) acc += __shfl(t, v * 8 + x, 64) * cy[v];
        int p = (acc >> 16) + 128;
        p = p < 0 ? 0 : (p > 255 ? 255 : p);
        if (i == 0) {
            cr = p;
        } else if (i == 1) {
            *(uint16_t*)(frame + w * (size_t)j.height + w * (size_t)(fy * 8 + y) + 2 * (size_t)(fx * 8 + x)) = (uint16_t)(cr | (p << 8));
        } else {
            frame[w * (size_t)(fy * 16 + ((i - 2) >> 1) * 8 + y) + (size_t)(fx * 16 + ((i - 2) & 1) * 8 + x)] = (uint8_t)p;
        }
    }
}

// ---- SSE: dwords of both frames, squared byte differences summed in 64 bits, one atomic add per wavefront and plane
__device__ __forceinline__ uint32_t sq_diff(uint32_t a, uint32_t b, int byte) {
    const int d = (int)((a >> (8 * byte)) & 255u) - (int)((b >> (8 * byte)) & 255u);
    return (uint32_t)(d * d);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void mdec_sse_kernel(const uint8_t* a, const uint8_t* b, size_t stride, int wh, int n_frames,
                                                       unsigned long long* sse) {
    const int luma_words = wh / 4, words = luma_words + wh / 8;
    for (int f = (int)blockIdx.y; f < n_frames; f += (int)gridDim.y) {
        const uint32_t* pa = (const uint32_t*)(a + (size_t)f * stride);
        const uint32_t* pb = (const uint32_t*)(b + (size_t)f * stride);
        unsigned long long sy = 0, scb = 0, scr = 0;
        for (int i = (int)(blockIdx.x * 256u + threadIdx.x); i < words; i += (int)(gridDim.x * 256u)) {
            const uint32_t wa = pa[i], wb = pb[i];
            const uint32_t even = sq_diff(wa, wb, 0) + sq_diff(wa, wb, 2), odd = sq_diff(wa, wb, 1) + sq_diff(wa, wb, 3);
            if (i < luma_words) {
                sy += even + odd;
            } else {                                   // NV21: Cr (V) first
                scr += even;
                scb += odd;
            }
        }
        sy = wave_sum(sy); scb = wave_sum(scb); scr = wave_sum(scr);
        if ((threadIdx.x & 63u) == 0) {
            if (sy) atomicAdd(&sse[(size_t)f * 3 + 0], sy);
            if (scb) atomicAdd(&sse[(size_t)f * 3 + 1], scb);
            if (scr) atomicAdd(&sse[(size_t)f * 3 + 2], scr);
        }
    }
}

}  // namespace

extern "C" hipError_t psxhip_mdec_parse_launch(const psxhip_mdec_parse_job_t* j, void* stream) {
    if (j->n_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(mdec_parse_kernel, dim3((unsigned)j->n_frames), dim3(64), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}

extern "C" hipError_t psxhip_mdec_reconstruct_launch(const psxhip_mdec_recon_job_t* j, void* stream) {
    if (j->n_frames <= 0) return hipSuccess;
    const int64_t waves = (int64_t)j->n_frames * (j->width / 16) * (j->height / 16);
    hipLaunchKernelGGL(mdec_reconstruct_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}

extern "C" hipError_t psxhip_mdec_sse_launch(const uint8_t* d_a, const uint8_t* d_b, size_t frame_stride, int width, int height,
                                             int n_frames, unsigned long long* d_sse, void* stream) {
    if (n_frames <= 0) return hipSuccess;
    const int wh = width * height;
    const int words = wh / 4 + wh / 8;
    const int gx = words / 256 / 8 < 1 ? 1 : (words / 256 / 8 > 32 ? 32 : words / 256 / 8);
    hipLaunchKernelGGL(mdec_sse_kernel, dim3((unsigned)gx, (unsigned)(n_frames < 32768 ? n_frames : 32768)), dim3(256), 0,
                       (hipStream_t)stream, d_a, d_b, frame_stride, wh, n_frames, d_sse);
    return hipGetLastError();
}
