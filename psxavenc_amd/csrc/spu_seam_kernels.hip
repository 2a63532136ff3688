// spu_seam_kernels.hip -- "psxhip SPU loop seam v1" on the device for MI355X (gfx950), hand-written HIP.
// spu_seam_step_kernel runs between the body passes of mode STEADY and decides, per looping entry, whether the pass just made is a
// fixed point; spu_seam_report_kernel judges a bank's loop seams from its bytes.  The arithmetic of both is spu_seam_core.h's, which
// host code compiles as well; here is the mapping: a chain is serial, so a lane takes one entry and the parallelism is across
// entries.  No LDS, no scratch, no waits on other workgroups; every loop is bounded by the entry's data blocks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psxhip_spu_seam_internal.h"
#include "spu_seam_core.h"

namespace {

__global__ __launch_bounds__(64) void spu_seam_step_kernel(const psxhip_spu_seam_step_job_t job) {
    const int j = (int)(blockIdx.x * 64 + threadIdx.x);
    if (j >= job.n_body) return;
    const int intro = job.body_intro[j];
    psxhip_adpcm_state_t s0;
    s0.prev1 = 0;
    s0.prev2 = 0;
    if (intro >= 0) s0 = job.first_states[intro];
    spu_seam_step(job.k, job.passes, s0, job.body_units[j], job.chains + j, job.states + j, job.start + j, job.outcome + job.body_entry[j]);
}

__global__ __launch_bounds__(64) void spu_seam_report_kernel(const psxhip_spu_seam_report_job_t job) {
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= job.n_entries) return;
    spu_seam_report_entry(job.rows[i], job.bank, job.pcm, job.seam + i);
}

}  // namespace

extern "C" hipError_t psxhip_spu_seam_step_launch(const psxhip_spu_seam_step_job_t* j, void* stream) {
    hipLaunchKernelGGL(spu_seam_step_kernel, dim3((unsigned)((j->n_body + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}

extern "C" hipError_t psxhip_spu_seam_report_launch(const psxhip_spu_seam_report_job_t* j, void* stream) {
    hipLaunchKernelGGL(spu_seam_report_kernel, dim3((unsigned)((j->n_entries + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}
