// psxhip_display_internal.h -- glue between the display back-end's C-ABI layer (psxhip_display.cpp, and psxhip_decode.cpp's
// decode-and-display entry) and its kernels (display_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/psxav_hip.h"

/* bumped with every change to the display kernels: profiles/ is keyed by it */
#define PSXHIP_DISPLAY_KERNEL_REV "disp-k1.0"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
	const uint8_t *d_frames;
	size_t frame_stride;
	const psxhip_mdec_decoded_t *d_decoded;     /* or NULL: every frame is converted */
	uint8_t *d_dst;
	size_t dst_pitch, dst_stride;
	int width, height, n_frames;
	int out_format;                             /* PSXHIP_OUT_* */
	uint32_t options;                           /* PSXHIP_DISPLAY_* */
} psxhip_display_job_t;
/* a checked job (psxhip_display_check): frames are a grid dimension, cut into launches of at most 65 535 */
hipError_t psxhip_display_launch(const psxhip_display_job_t *j, void *stream);

#ifdef __cplusplus
}

/* the argument rules of "psxhip display v1", which need no device (sizes, format, options, pitch and stride; device_pointers: also
 * the pointers' alignment and that the pictures do not overlap the frames): PSXHIP_OK, or PSXHIP_EINVAL with the error text set,
 * `who` naming the entry point */
int psxhip_display_check(const char *who, const psxhip_display_job_t *j, bool device_pointers);
#endif
