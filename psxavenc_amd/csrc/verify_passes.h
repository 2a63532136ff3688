// verify_passes.h -- the host side of speculate-and-verify along time, shared by the ADPCM encoder's session
// (psxhip_adpcm_encode.cpp) and the chunked decoder (psxhip_adpcm_decode.cpp): run verify passes until one changes nothing.
#pragma once
#include "psxhip_internal.h"

// the flag words of a batch, on the device and wherever the caller reads them back
constexpr int kVerifyBatchMax = 16;

// "Some chunk's start state changed" is one word of device memory per pass.  Passes are launched in batches, back to back:
// pass i + 1 looks at pass i's word when it starts and returns at once if nothing changed, so the host reads the words once
// per batch -- no synchronise + launch round trip (40-50 us) per pass.
//   launch(changed, changed_before)   launches one verify pass on `st` (changed_before: NULL for a batch's first pass)
//   d_flags, h_flags                  kVerifyBatchMax words each; h_flags is host memory the batch's words are copied to
//   max_passes                        <= 0: until the fixpoint
// Returns the passes that ran up to and including the first that changed nothing (*any_change: one of them changed
// something), or a negative PSXHIP_E* with the error text set -- "<who>: not converged after N verify passes" when
// max_passes ran out (PSXHIP_EINVAL).  The stream is at rest when it returns a count.
template <class Launch>
int run_verify_passes(Launch&& launch, int* d_flags, int* h_flags, hipStream_t st, int max_passes, const char* who, bool* any_change) {
    int passes = 0;
    *any_change = false;
    // first batch: most material is done after "one pass that repairs + one that finds nothing"
    // (measured, NOTEBOOK round 6: with every batch 48 passes a short stream's whole verify phase is ONE batch, no host round trip
    //  in it -- the round trips cost nothing measurable)
    int batch = 3;
    for (bool done = false; !done;) {
        if (max_passes > 0 && passes + batch > max_passes) batch = max_passes - passes;
        if (batch < 1) {
            psxhip_set_error("%s: not converged after %d verify passes", who, passes);
            return PSXHIP_EINVAL;
        }
        HIP_TRY(hipMemsetAsync(d_flags, 0, kVerifyBatchMax * sizeof(int), st), PSXHIP_EDEVICE);
        for (int i = 0; i < batch; i++) HIP_TRY(launch(d_flags + i, i ? d_flags + i - 1 : nullptr), PSXHIP_EDEVICE);
        HIP_TRY(hipMemcpyAsync(h_flags, d_flags, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
        HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
        for (int i = 0; i < batch && !done; i++) {
            passes++;                      // this pass ran
            if (h_flags[i]) *any_change = true;
            else done = true;              // it changed nothing: the fixpoint; the passes behind it returned at once
        }
        batch = batch * 2 < kVerifyBatchMax ? batch * 2 : kVerifyBatchMax;
    }
    return passes;
}
