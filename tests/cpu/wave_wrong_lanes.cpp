// tests/cpu/wave_wrong_lanes.cpp -- TEST INFRASTRUCTURE: deliberately wrong kernels, one per report of the stand-in's wavefront
// model (tests/cpu/hip_lanes/hip_lanes_waves.h) and of the host sanitizers behind it.  tests/test_wave_model_cpu.py demands the
// specific report for each.  CPU only: this text is never built for a device and never run on one.
//
//   wave_wrong_lanes <case> [order [seed]]
#define HIP_LANES_WAVES 1
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace {

// a barrier inside a branch one wavefront skips, met by the others' barrier further down
__global__ void barrier_in_branch_kernel(int* out) {
    __shared__ int s[256];
    const int tid = (int)threadIdx.x;
    s[tid] = tid;
    if (tid >= 64) __syncthreads();
    out[tid] = s[255 - tid];
    __syncthreads();
}

// a barrier inside a branch half a wavefront skips: the other half goes on to a collective
__global__ void barrier_and_collective_kernel(int* out) {
    const int tid = (int)threadIdx.x;
    if (tid < 32) __syncthreads();
    out[tid] = __shfl_xor(tid, 1, 64);
}

// one collective met from two call sites
__global__ void two_sites_kernel(int* out) {
    const int tid = (int)threadIdx.x;
    int v;
    if (tid & 1) v = __shfl_xor(tid, 2, 64);
    else
        v = __shfl_xor(tid, 2, 64);
    out[tid] = v;
}

// a shuffle from a lane that has returned
__global__ void returned_lane_kernel(int* out) {
    const int tid = (int)threadIdx.x;
    if (tid == 5) return;
    out[tid] = __shfl(tid, 5, 64);
}

// readlane of a lane the workgroup does not have
__global__ void missing_lane_kernel(int* out) {
    const int tid = (int)threadIdx.x;
    out[tid] = __builtin_amdgcn_readlane(tid, 40);
}

// an LDS index one past its array
__global__ void lds_past_kernel(int* out) {
    __shared__ int s[64];
    __shared__ int t[64];
    const int tid = (int)threadIdx.x;
    volatile int* p = s;
    p[tid + 1] = tid;
    t[tid] = 0;
    __syncthreads();
    out[tid] = p[tid] + t[tid];
}

// a global read one past a heap block
__global__ void global_past_kernel(const int* in, int* out) {
    const int tid = (int)threadIdx.x;
    out[tid] = in[tid + 1];
}

// LDS that nobody wrote reaches the output: other bytes in every order and for every seed
__global__ void lds_unwritten_kernel(int* out) {
    __shared__ int s[64];
    out[threadIdx.x] = s[threadIdx.x];
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (argc > 2) hip_lanes::order = atoi(argv[2]);
    if (argc > 3) hip_lanes::seed = strtoull(argv[3], nullptr, 10);
    int *in = nullptr, *out = nullptr;
    if (hipMalloc(&in, 64 * sizeof(int)) != hipSuccess || hipMalloc(&out, 256 * sizeof(int)) != hipSuccess) return 4;
    memset(in, 0, 64 * sizeof(int));
    memset(out, 0, 256 * sizeof(int));
    const char* c = argv[1];
    if (!strcmp(c, "barrier_in_branch")) hipLaunchKernelGGL(barrier_in_branch_kernel, dim3(1), dim3(256), 0, nullptr, out);
    else if (!strcmp(c, "barrier_and_collective")) hipLaunchKernelGGL(barrier_and_collective_kernel, dim3(1), dim3(64), 0, nullptr, out);
    else if (!strcmp(c, "two_sites")) hipLaunchKernelGGL(two_sites_kernel, dim3(1), dim3(64), 0, nullptr, out);
    else if (!strcmp(c, "returned_lane")) hipLaunchKernelGGL(returned_lane_kernel, dim3(1), dim3(64), 0, nullptr, out);
    else if (!strcmp(c, "missing_lane")) hipLaunchKernelGGL(missing_lane_kernel, dim3(1), dim3(32), 0, nullptr, out);
    else if (!strcmp(c, "lds_past")) hipLaunchKernelGGL(lds_past_kernel, dim3(1), dim3(64), 0, nullptr, out);
    else if (!strcmp(c, "global_past")) hipLaunchKernelGGL(global_past_kernel, dim3(1), dim3(64), 0, nullptr, in, out);
    else if (!strcmp(c, "lds_unwritten")) hipLaunchKernelGGL(lds_unwritten_kernel, dim3(2), dim3(64), 0, nullptr, out);
    else return 2;
    fwrite(out, sizeof(int), 256, stdout);
    (void)hipFree(in);
    (void)hipFree(out);
    return 0;
}
