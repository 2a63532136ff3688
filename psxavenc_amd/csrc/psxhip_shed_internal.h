// psxhip_shed_internal.h -- glue between the host layer (psxhip_api.cpp) and the refinement's kernels (mdec_shed_kernels.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/psxav_hip.h"
#include "mdec_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a frame's verdict in its workspace (MdecShedWs::decision): zero until the decide kernel has taken the frame */
typedef struct {
	int32_t step;                /* t* of a refined frame, else 0 */
	int32_t blocks_used;
	int64_t bits;                /* the refined stream's bits, the end code included */
	uint32_t tail;               /* the halfword behind the budget's last whole dword, collected by the emit kernel */
	uint32_t reserved;
} psxhip_mdec_shed_decision_t;

typedef struct {
	const uint8_t *d_frames;
	uint8_t *d_out;
	psxhip_mdec_result_t *d_results;
	psxhip_mdec_refine_t *d_refine;       /* or NULL */
	const int32_t *d_frame_max_sizes;     /* or NULL */
	size_t frame_stride, out_stride;
	int width, height, codec, nmb;
	int n_frames, uniform_max_size, max_frame_size, max_magnitude;
	int groups_per_frame;                 /* mdec_shed_analyse_groups(nmb) */
	uint8_t *d_ws;                        /* n_frames x ws.stride bytes; [0, ws.zeroed) of each frame's is zero */
	MdecShedWs ws;
} psxhip_mdec_shed_job_t;

hipError_t psxhip_mdec_shed_upload_tables(void);
hipError_t psxhip_mdec_shed_launch(const psxhip_mdec_shed_job_t *j, void *stream);

#ifdef __cplusplus
}
#endif
