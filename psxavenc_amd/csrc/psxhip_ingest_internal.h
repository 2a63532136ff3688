// psxhip_ingest_internal.h -- glue between the picture ingest's C-ABI layer (psxhip_ingest.cpp) and its kernels
// (ingest_kernels.hip).  C++ only: a job carries ingest_core.h's description of the source by value.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/psxav_hip.h"
#include "ingest_core.h"

/* bumped with every change to the ingest kernels: profiles/ is keyed by it */
#define PSXHIP_INGEST_KERNEL_REV "ingest-k1.0"

struct psxhip_ingest_job_t {
    IngestDesc d;
    const uint8_t* d_src;
    size_t src_stride;
    int n_src;
    const int32_t* d_src_index;      // or NULL: output picture i is made from source picture i
    int first, n_out;                // the launch makes output pictures first .. first + n_out - 1
    uint8_t* d_out;
    size_t out_stride;
    int out_format;                  // PSXHIP_PIX_*
};
// a checked job (psxhip_ingest.cpp): output pictures are a grid dimension, cut into launches of at most 65 535
extern "C" hipError_t psxhip_ingest_launch(const psxhip_ingest_job_t* j, void* stream);
