// tests/cpu/hip_lanes/hip/hip_runtime.h -- TEST INFRASTRUCTURE, NOT HIP: a stand-in of this name for the host compiler, so that the
// text of a kernel file compiles unchanged with g++ and runs on the CPU under -fsanitize=address,undefined (tests/cpu/*_lanes.cpp;
// the include path puts this folder first).  It has two forms.
//
// Without HIP_LANES_WAVES it holds what the barrier-free kernel files (psxavenc_amd/csrc/{ingest,display,strspu,synth}_kernels.hip)
// use and no more: the function qualifiers as empty words, dim3 and the four index variables, uint4 / int4, the byte permute the
// kernels pack with, and a hipLaunchKernelGGL that calls the kernel once per lane.  A lane runs to its end before the next one
// starts, in the order the program chose (hip_lanes::order): ascending, descending, or a seeded shuffle of all (workgroup, lane)
// pairs of the launch.  A kernel whose lanes do not talk to each other gives the same bytes in all three.
//
// With HIP_LANES_WAVES defined in front of the kernel file's text (the reader side: {disc_read,str_demux,strspu_demux,mdec_decode,
// adpcm_decode}_kernels.hip) the launch goes through the wavefront model of hip_lanes_waves.h instead: a workgroup's lanes are
// fibers that are resumed round by round, held at __syncthreads and at every cross-lane operation, with LDS, atomics, __constant__
// and the small CPU "device" of hip_lanes_device.h that the modules' host layer needs.  That file says what the model guarantees,
// what it reports and what it cannot see.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct alignas(16) uint4 { uint32_t x, y, z, w; };
struct alignas(16) int4 { int32_t x, y, z, w; };

typedef int hipError_t;
enum { hipSuccess = 0 };
typedef struct hip_lanes_stream* hipStream_t;
inline hipError_t hipGetLastError() { return hipSuccess; }
inline const char* hipGetErrorString(hipError_t) { return "hip_lanes"; }

inline dim3 threadIdx, blockIdx, blockDim, gridDim;

// v_perm_b32: byte i of the result is picked by byte i of sel from the eight bytes {hi, lo} (0 .. 3: lo, 4 .. 7: hi), 12: a zero byte.
// (The selectors 8 .. 11 and 13 .. 15 -- sign bits and 0xff -- are not used by this project's kernels and read as zero here.)
inline uint32_t hip_lanes_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t s = (sel >> (8 * i)) & 255u;
        if (s < 8) out |= (uint32_t)((both >> (8 * s)) & 255u) << (8 * i);
    }
    return out;
}
#define __builtin_amdgcn_perm hip_lanes_perm

namespace hip_lanes {

enum { ASCENDING = 0, DESCENDING = 1, SHUFFLED = 2 };
inline int order = ASCENDING;
inline uint64_t seed = 1;          // of the shuffle; every launch draws its own permutation from it
inline uint64_t launches = 0, lanes_run = 0;

inline uint64_t next_random(uint64_t& s) {      // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// lane `at` of the launch, counted x fastest: thread x, y, z, then workgroup x, y, z
inline void place(uint64_t at, dim3 grid, dim3 block) {
    threadIdx.x = (unsigned)(at % block.x); at /= block.x;
    threadIdx.y = (unsigned)(at % block.y); at /= block.y;
    threadIdx.z = (unsigned)(at % block.z); at /= block.z;
    blockIdx.x = (unsigned)(at % grid.x); at /= grid.x;
    blockIdx.y = (unsigned)(at % grid.y); at /= grid.y;
    blockIdx.z = (unsigned)at;
}

template <typename Lane>
void run_grid(dim3 grid, dim3 block, Lane lane) {
    const uint64_t total = (uint64_t)grid.x * grid.y * grid.z * block.x * block.y * block.z;
    gridDim = grid;
    blockDim = block;
    launches++;
    lanes_run += total;
    if (order == SHUFFLED) {
        std::vector<uint32_t> perm(total);      // (a launch of this project's tests stays far below 2^32 lanes)
        for (uint64_t i = 0; i < total; i++) perm[i] = (uint32_t)i;
        uint64_t s = seed + launches;
        for (uint64_t i = total; i > 1; i--) std::swap(perm[i - 1], perm[next_random(s) % i]);
        for (uint64_t i = 0; i < total; i++) {
            place(perm[i], grid, block);
            lane();
        }
        return;
    }
    for (uint64_t i = 0; i < total; i++) {
        place(order == DESCENDING ? total - 1 - i : i, grid, block);
        lane();
    }
}

template <typename Kernel, typename... Args>
void launch(Kernel kernel, dim3 grid, dim3 block, const Args&... args) {
    run_grid(grid, block, [&] { kernel(args...); });
}

}  // namespace hip_lanes

// (dynamic LDS bytes and the stream are taken and ignored: the launch has run when this returns)
#ifdef HIP_LANES_WAVES
#include "../hip_lanes_device.h"
#include "../hip_lanes_waves.h"
#define hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, ...) \
    do { (void)(lds_bytes); (void)(stream); hip_lanes::launch_waves(kernel, grid, block, __VA_ARGS__); } while (0)
#else
#define hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, ...) \
    do { (void)(lds_bytes); (void)(stream); hip_lanes::launch(kernel, grid, block, __VA_ARGS__); } while (0)
#endif
