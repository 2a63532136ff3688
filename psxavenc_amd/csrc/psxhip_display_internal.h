// psxhip_display_internal.h -- glue between the display back-end's C-ABI layer (psxhip_display.cpp, and psxhip_decode.cpp's
// decode-and-display entry) and its kernels (display_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/psxav_hip.h"
#include "picture_plan.h"          /* the job, and psxhip_display_check */

/* bumped with every change to the display kernels: profiles/ is keyed by it */
#define PSXHIP_DISPLAY_KERNEL_REV "disp-k1.0"

#ifdef __cplusplus
extern "C" {
#endif

/* a checked job (psxhip_display_check): frames are a grid dimension, cut into launches of at most 65 535 */
hipError_t psxhip_display_launch(const psxhip_display_job_t *j, void *stream);

#ifdef __cplusplus
}
#endif
