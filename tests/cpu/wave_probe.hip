// tests/cpu/wave_probe.hip -- TEST INFRASTRUCTURE: small, well-defined kernels that exercise every cross-lane operation the reader
// kernels use, with plain-numpy answers in the tests.  One text, two builds:
//   * by g++ behind the stand-in tests/cpu/hip_lanes (tests/cpu/wave_probe_lanes.cpp, tests/test_wave_model_cpu.py): the wavefront
//     model's own test, under the host sanitizers, in three lane orders;
//   * by hipcc for gfx950 into a stand-alone program (tests/test_gpu_wave_probe.py): the same bytes from the MI355X, which pins the
//     stand-in's reading of the shuffles' edges and of the DPP controls to the hardware.
//
//   wave_probe <in> <out> [order [seed]]
// in:  int32 {rows, n_masks, n_tiles, n_groups}, then x[rows][64] int32, y[rows][64] int64, masks[n_masks][2] uint64 (a predicate
//      mask and an arbitrary one), tiles[n_tiles][256] int32, atom[n_groups][256] uint32
// out: out32[kSlots32][rows][64] int32, out64[kSlots64][rows][64] uint64, m32[kMaskSlots32][n_masks][64] int32,
//      m64[n_masks][64] uint64, tiles_out[n_tiles][256] int32, atomics[kAtomics] uint64
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../psxavenc_amd/csrc/wave_ops.h"

namespace {

// ---- slots of out32 / out64
enum {
    S_SCAN = 0, S_REDUCE, S_POPC_BELOW, S_FIRST, S_ANY, S_ALL_ODD,
    S_UP0, S_UP1, S_UP2, S_UP31, S_UP32, S_UP63, S_UP64,
    S_DOWN0, S_DOWN1, S_DOWN2, S_DOWN31, S_DOWN32, S_DOWN63, S_DOWN64,
    S_XOR1, S_XOR5, S_XOR32, S_XOR63,
    S_SHFL0, S_SHFL63, S_SHFL_ROT, S_SHFL_WRAP, S_SHFL_DATA,
    S_UP3_W16, S_DOWN3_W16, S_XOR9_W16, S_SHFL5_W16,
    S_READLANE0, S_READLANE37, S_READLANE63,
    S_DPP_QUAD_B1, S_DPP_QUAD_4E, S_DPP_QUAD_1B_OLD, S_DPP_SHR1, S_DPP_SHR2, S_DPP_SHR3, S_DPP_SHR4_E, S_DPP_SHR8_C, S_DPP_SHR1_OLD,
    S_DPP_SHR15_OLD, S_DPP_MIRROR, S_DPP_HALF_MIRROR, S_DPP_BCAST15_A, S_DPP_BCAST31_C, S_DPP_BCAST15_OLD, S_DPP_BCAST31_OLD,
    S_DPP_SHR4_E_BOUND,
    kSlots32
};
enum { T_BALLOT = 0, T_MIN64, T_UP1, T_UP64, T_DOWN1, T_DOWN33, T_XOR32, T_SHFL_ROT, kSlots64 };
enum { M_BALLOT_LO = 0, M_BALLOT_HI, M_MBCNT, M_POPC_BELOW, M_POPCLL, M_FFSLL, M_CLZLL, M_ANY, kMaskSlots32 };
enum { A_ADD_INT = 0, A_ADD_U32, A_ADD_U64, A_SUB_INT, A_MIN_U32, A_MIN_INT, A_MAX_U32, A_MAX_INT, A_OR_U32, A_LDS_ADD, A_LDS_MAX, A_LDS_MIN,
       A_LDS_OR, kAtomics };

#define DPP(old, x, ctrl, rows, banks, bound) __builtin_amdgcn_update_dpp(old, x, ctrl, rows, banks, bound)

__global__ __launch_bounds__(64) void probe_wave_kernel(const int* x, const long long* y, int rows, int* out32, unsigned long long* out64) {
    const int lane = (int)threadIdx.x, r = (int)blockIdx.x;
    const int v = x[r * 64 + lane];
    const long long w = y[r * 64 + lane];
    const int old = -1000 - lane;
#define OUT32(slot, value) out32[((size_t)(slot) * rows + r) * 64 + lane] = (value)
#define OUT64(slot, value) out64[((size_t)(slot) * rows + r) * 64 + lane] = (unsigned long long)(value)
    OUT32(S_SCAN, wave::inclusive_scan_add(v));
    OUT32(S_REDUCE, wave::reduce_add(v));
    const uint64_t odd = wave::ballot((v & 1) != 0);
    OUT64(T_BALLOT, odd);
    OUT32(S_POPC_BELOW, wave::popc_below(odd));
    OUT32(S_FIRST, wave::broadcast_first(v));
    OUT32(S_ANY, __any(v != 0));
    OUT32(S_ALL_ODD, (int)__popcll(__ballot(v & 1)));
    OUT64(T_MIN64, wave::reduce_min_u64((uint64_t)w ^ 0x8000000000000000ull));

    OUT32(S_UP0, __shfl_up(v, 0, 64));       OUT32(S_UP1, __shfl_up(v, 1, 64));       OUT32(S_UP2, __shfl_up(v, 2, 64));
    OUT32(S_UP31, __shfl_up(v, 31, 64));     OUT32(S_UP32, __shfl_up(v, 32, 64));     OUT32(S_UP63, __shfl_up(v, 63, 64));
    OUT32(S_UP64, __shfl_up(v, 64, 64));
    OUT32(S_DOWN0, __shfl_down(v, 0, 64));   OUT32(S_DOWN1, __shfl_down(v, 1, 64));   OUT32(S_DOWN2, __shfl_down(v, 2, 64));
    OUT32(S_DOWN31, __shfl_down(v, 31, 64)); OUT32(S_DOWN32, __shfl_down(v, 32, 64)); OUT32(S_DOWN63, __shfl_down(v, 63, 64));
    OUT32(S_DOWN64, __shfl_down(v, 64, 64));
    OUT32(S_XOR1, __shfl_xor(v, 1, 64));     OUT32(S_XOR5, __shfl_xor(v, 5, 64));     OUT32(S_XOR32, __shfl_xor(v, 32, 64));
    OUT32(S_XOR63, __shfl_xor(v, 63, 64));
    OUT32(S_SHFL0, __shfl(v, 0, 64));        OUT32(S_SHFL63, __shfl(v, 63, 64));      OUT32(S_SHFL_ROT, __shfl(v, (lane * 7 + 3) & 63, 64));
    OUT32(S_SHFL_WRAP, __shfl(v, lane + 64 + 1, 64));                                  // a source past 63 wraps: (lane + 1) & 63
    OUT32(S_SHFL_DATA, __shfl(v, v & 63, 64));
    OUT32(S_UP3_W16, __shfl_up(v, 3, 16));   OUT32(S_DOWN3_W16, __shfl_down(v, 3, 16));
    OUT32(S_XOR9_W16, __shfl_xor(v, 9, 16)); OUT32(S_SHFL5_W16, __shfl(v, 5, 16));
    OUT32(S_READLANE0, __builtin_amdgcn_readlane(v, 0));
    OUT32(S_READLANE37, __builtin_amdgcn_readlane(v, 37));
    OUT32(S_READLANE63, __builtin_amdgcn_readlane(v, 63));

    OUT64(T_UP1, __shfl_up(w, 1, 64));       OUT64(T_UP64, __shfl_up(w, 64, 64));
    OUT64(T_DOWN1, __shfl_down(w, 1, 64));   OUT64(T_DOWN33, __shfl_down((unsigned long long)w, 33, 64));
    OUT64(T_XOR32, __shfl_xor(w, 32, 64));   OUT64(T_SHFL_ROT, __shfl(w, (lane * 5 + 1) & 63, 64));

    // the DPP controls of wave_ops.h, each with the masks it uses there and once with a visible `old`
    OUT32(S_DPP_QUAD_B1, DPP(0, v, 0xB1, 0xF, 0xF, true));
    OUT32(S_DPP_QUAD_4E, DPP(0, v, 0x4E, 0xF, 0xF, true));
    OUT32(S_DPP_QUAD_1B_OLD, DPP(old, v, 0x1B, 0x5, 0x9, false));
    OUT32(S_DPP_SHR1, DPP(0, v, 0x111, 0xF, 0xF, true));
    OUT32(S_DPP_SHR2, DPP(0, v, 0x112, 0xF, 0xF, true));
    OUT32(S_DPP_SHR3, DPP(0, v, 0x113, 0xF, 0xF, true));
    OUT32(S_DPP_SHR4_E, DPP(0, v, 0x114, 0xF, 0xE, false));
    OUT32(S_DPP_SHR8_C, DPP(0, v, 0x118, 0xF, 0xC, false));
    OUT32(S_DPP_SHR1_OLD, DPP(old, v, 0x111, 0xF, 0xF, false));
    OUT32(S_DPP_SHR15_OLD, DPP(old, v, 0x11F, 0xF, 0xF, false));
    OUT32(S_DPP_MIRROR, DPP(0, v, 0x140, 0xF, 0xF, true));
    OUT32(S_DPP_HALF_MIRROR, DPP(0, v, 0x141, 0xF, 0xF, true));
    OUT32(S_DPP_BCAST15_A, DPP(0, v, 0x142, 0xA, 0xF, false));
    OUT32(S_DPP_BCAST31_C, DPP(0, v, 0x143, 0xC, 0xF, false));
    OUT32(S_DPP_BCAST15_OLD, DPP(old, v, 0x142, 0xF, 0xF, false));
    OUT32(S_DPP_BCAST31_OLD, DPP(old, v, 0x143, 0xF, 0xF, false));
    OUT32(S_DPP_SHR4_E_BOUND, DPP(old, v, 0x114, 0xF, 0xE, true));
#undef OUT32
#undef OUT64
}

// ballots and mbcnt on sparse masks: lane l votes bit l of masks[m][0]; masks[m][1] is counted as it is
__global__ __launch_bounds__(64) void probe_mask_kernel(const unsigned long long* masks, int n_masks, int* m32, unsigned long long* m64) {
    const int lane = (int)threadIdx.x, m = (int)blockIdx.x;
    const unsigned long long pred = masks[2 * m], any = masks[2 * m + 1];
    const bool p = (pred >> lane) & 1ull;
    const unsigned long long b = __ballot(p);
    const uint64_t b2 = wave::ballot(p);
#define M32(slot, value) m32[((size_t)(slot) * n_masks + m) * 64 + lane] = (value)
    M32(M_BALLOT_LO, (int)(uint32_t)b);
    M32(M_BALLOT_HI, (int)(uint32_t)(b >> 32));
    m64[(size_t)m * 64 + lane] = b2;
    M32(M_MBCNT, (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(any >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)any, 5u)));
    M32(M_POPC_BELOW, wave::popc_below(any));
    M32(M_POPCLL, (int)__popcll(any));
    M32(M_FFSLL, (int)__ffsll((unsigned long long)any));
    M32(M_CLZLL, (int)__clzll((long long)any));
    M32(M_ANY, __any(p));
#undef M32
}

// a 16 x 16 transpose through LDS by four wavefronts, then a reversal: a barrier in front of every read of what other wavefronts wrote
// and in front of every write over what they read
__global__ __launch_bounds__(256) void probe_transpose_kernel(const int* in, int* out) {
    __shared__ int tile[256];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    tile[tid] = in[b * 256 + tid];
    __syncthreads();
    const int v = tile[(tid & 15) * 16 + (tid >> 4)];
    __syncthreads();
    tile[255 - tid] = v;
    __syncthreads();
    out[b * 256 + tid] = tile[tid];
}

// every atomic the reader kernels use, on global memory and on LDS; only the final values count
__global__ __launch_bounds__(256) void probe_atomic_kernel(const uint32_t* atom, unsigned long long* res) {
    __shared__ int l_add;
    __shared__ uint32_t l_max, l_min, l_or;
    const int tid = (int)threadIdx.x;
    const uint32_t a = atom[blockIdx.x * 256 + tid];
    if (tid == 0) { l_add = 0; l_max = 0; l_min = 0xFFFFFFFFu; l_or = 0; }
    __syncthreads();
    atomicAdd((int*)&res[A_ADD_INT], (int)(a & 0xFFFF) - 30000);
    atomicAdd((uint32_t*)&res[A_ADD_U32], a >> 12);
    atomicAdd(&res[A_ADD_U64], (unsigned long long)a << 8);
    atomicSub((int*)&res[A_SUB_INT], (int)(a & 0xFFF));
    atomicMin((uint32_t*)&res[A_MIN_U32], a);
    atomicMin((int*)&res[A_MIN_INT], (int)a);
    atomicMax((uint32_t*)&res[A_MAX_U32], a);
    atomicMax((int*)&res[A_MAX_INT], (int)a);
    if ((a & 7u) == 0u) atomicOr((uint32_t*)&res[A_OR_U32], 1u << (a >> 27));
    atomicAdd(&l_add, (int)(a & 0xFF));
    atomicMax(&l_max, a);
    atomicMin(&l_min, a);
    atomicOr(&l_or, 1u << (tid & 31));
    __syncthreads();
    if (tid == 0) {
        atomicAdd((int*)&res[A_LDS_ADD], l_add);
        atomicMax((uint32_t*)&res[A_LDS_MAX], l_max);
        atomicMin((uint32_t*)&res[A_LDS_MIN], l_min);
        atomicOr((uint32_t*)&res[A_LDS_OR], l_or & a);
    }
}

template <typename T>
bool read_all(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

#define CHECK(expr)                                                              \
    do {                                                                         \
        const hipError_t e_ = (expr);                                            \
        if (e_ != hipSuccess) {                                                  \
            fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));           \
            return 10;                                                           \
        }                                                                        \
    } while (0)

template <typename T>
hipError_t to_device(T** d, const std::vector<T>& h, size_t n_out) {
    // (a block of exactly the bytes the kernels may touch: the host sanitizers see its end)
    const size_t n = h.empty() ? n_out : h.size();
    hipError_t e = hipMalloc((void**)d, n * sizeof(T));
    if (e == hipSuccess && !h.empty()) e = hipMemcpy(*d, h.data(), n * sizeof(T), hipMemcpyHostToDevice);
    if (e == hipSuccess && h.empty()) e = hipMemset(*d, 0xEE, n * sizeof(T));
    return e;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
#ifdef HIP_LANES_WAVES
    if (argc > 3) hip_lanes::order = atoi(argv[3]);
    if (argc > 4) hip_lanes::seed = strtoull(argv[4], nullptr, 10);
#endif
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t head[4];
    if (fread(head, sizeof head, 1, in) != 1) return 3;
    const int rows = head[0], n_masks = head[1], n_tiles = head[2], n_groups = head[3];
    if (rows < 1 || n_masks < 1 || n_tiles < 1 || n_groups < 1 || rows > 4096 || n_masks > 4096 || n_tiles > 256 || n_groups > 256) return 3;
    std::vector<int> x, tiles;
    std::vector<long long> y;
    std::vector<unsigned long long> masks;
    std::vector<uint32_t> atom;
    if (!read_all(in, x, (size_t)rows * 64) || !read_all(in, y, (size_t)rows * 64) || !read_all(in, masks, (size_t)n_masks * 2) ||
        !read_all(in, tiles, (size_t)n_tiles * 256) || !read_all(in, atom, (size_t)n_groups * 256))
        return 3;
    fclose(in);

    int *d_x, *d_tiles, *d_out32, *d_m32, *d_tiles_out;
    long long* d_y;
    unsigned long long *d_masks, *d_out64, *d_m64, *d_res;
    uint32_t* d_atom;
    const size_t n32 = (size_t)kSlots32 * rows * 64, n64 = (size_t)kSlots64 * rows * 64, nm32 = (size_t)kMaskSlots32 * n_masks * 64,
                 nm64 = (size_t)n_masks * 64, nt = (size_t)n_tiles * 256;
    CHECK(to_device(&d_x, x, 0));
    CHECK(to_device(&d_y, y, 0));
    CHECK(to_device(&d_masks, masks, 0));
    CHECK(to_device(&d_tiles, tiles, 0));
    CHECK(to_device(&d_atom, atom, 0));
    CHECK(to_device(&d_out32, std::vector<int>(), n32));
    CHECK(to_device(&d_out64, std::vector<unsigned long long>(), n64));
    CHECK(to_device(&d_m32, std::vector<int>(), nm32));
    CHECK(to_device(&d_m64, std::vector<unsigned long long>(), nm64));
    CHECK(to_device(&d_tiles_out, std::vector<int>(), nt));
    // the atomics' start values: zero, but the minima start from all ones and the signed ones from their type's ends
    std::vector<unsigned long long> res(kAtomics, 0ull);
    res[A_SUB_INT] = 1000000ull;
    res[A_MIN_U32] = 0xFFFFFFFFull;
    res[A_MIN_INT] = 0x7FFFFFFFull;
    res[A_MAX_INT] = 0x80000000ull;
    res[A_LDS_MIN] = 0xFFFFFFFFull;
    CHECK(to_device(&d_res, res, 0));

    hipLaunchKernelGGL(probe_wave_kernel, dim3((unsigned)rows), dim3(64), 0, nullptr, d_x, d_y, rows, d_out32, d_out64);
    hipLaunchKernelGGL(probe_mask_kernel, dim3((unsigned)n_masks), dim3(64), 0, nullptr, d_masks, n_masks, d_m32, d_m64);
    hipLaunchKernelGGL(probe_transpose_kernel, dim3((unsigned)n_tiles), dim3(256), 0, nullptr, d_tiles, d_tiles_out);
    hipLaunchKernelGGL(probe_atomic_kernel, dim3((unsigned)n_groups), dim3(256), 0, nullptr, d_atom, d_res);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());

    std::vector<int> out32(n32), m32(nm32), tiles_out(nt);
    std::vector<unsigned long long> out64(n64), m64(nm64);
    CHECK(hipMemcpy(out32.data(), d_out32, n32 * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(out64.data(), d_out64, n64 * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(m32.data(), d_m32, nm32 * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(m64.data(), d_m64, nm64 * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(tiles_out.data(), d_tiles_out, nt * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(res.data(), d_res, kAtomics * 8, hipMemcpyDeviceToHost));
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    if (fwrite(out32.data(), 4, n32, out) != n32 || fwrite(out64.data(), 8, n64, out) != n64 || fwrite(m32.data(), 4, nm32, out) != nm32 ||
        fwrite(m64.data(), 8, nm64, out) != nm64 || fwrite(tiles_out.data(), 4, nt, out) != nt || fwrite(res.data(), 8, kAtomics, out) != kAtomics)
        return 5;
    (void)hipFree(d_x); (void)hipFree(d_y); (void)hipFree(d_masks); (void)hipFree(d_tiles); (void)hipFree(d_atom); (void)hipFree(d_out32);
    (void)hipFree(d_out64); (void)hipFree(d_m32); (void)hipFree(d_m64); (void)hipFree(d_tiles_out); (void)hipFree(d_res);
    return fclose(out) ? 5 : 0;
}
