// picture_plan.h -- what the picture front ends' host layer (psxhip_scaler.cpp, psxhip_ingest.cpp, psxhip_display.cpp; the display
// check is psxhip_decode.cpp's too) derives from a call's arguments alone: what every entry point refuses, with which text and in
// which order; the scaler's filter banks, its tile with the LDS total (scaler_layout.h), the vertical segments and the cut of a call
// into launches; the ingest's matrix and plane rules.  Arithmetic and refusals only (no HIP), like adpcm_plan.h and mdec_plan.h:
// picture_plan.cpp builds with a host compiler alone and links against nothing but psxhip_set_error (tests/test_picture_plan_cpu.py
// does so, under the host sanitizers); the launch files only execute these plans.  A plan function returns PSXHIP_OK, or PSXHIP_EINVAL
// with the error text set.  Pointers come as numbers: nothing here reads through one, except the caller's host arrays (planes, pts).
// The three planners of the C ABI that need no device (psxhip_ingest_recommend, _fit, _pace) and psxhip_display_row_bytes are
// defined in picture_plan.cpp as they stand in include/psxav_hip.h; nothing else here is part of the library's surface.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/psxav_hip.h"
#include "ingest_core.h"
#include "scaler_layout.h"

extern "C" void psxhip_set_error(const char* fmt, ...);          // (psxhip_api.cpp; psxhip_internal.h declares it beside HIP)

/* the display back-end's job (display_kernels.hip; checked by psxhip_display_check) */
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

#pragma GCC visibility push(hidden)

// "<who>: <what>" as the error text; PSXHIP_EINVAL
int picture_bad(const char* who, const char* what);

// ---------------------------------------------------------------------------------------------- the scaler
// psxhip_scaler_create's first refusal
int scaler_geometry_check(int src_format, int src_width, int src_height, int dst_width, int dst_height);

// one separable filter bank on the host: the specification's integer arithmetic (see the header of oracle/frontend_oracle.c for
// the same text as prose; the two are written independently and compared tap by tap in tests/test_gpu_frontend.py)
struct HostBank {
    int taps = 0, taps4 = 0;
    std::vector<int32_t> left;
    std::vector<int16_t> coef;
    std::vector<uint32_t> digits;       // see psxhip_scaler_bank_t::digits
};
bool make_bank(int src, int dst, HostBank* b);          // false: the filter shrinks by more than 16x (more than 64 taps)
// lh, lv, ch, cv of a geometry that passed the check, or the ">16x" refusal of the first bank that has one
int scaler_design_banks(int src_format, int src_width, int src_height, int dst_width, int dst_height, HostBank h[4]);

// The tile: the largest of kScalerShapes whose LDS working set (scaler_lds) leaves room for at least two workgroups per CU, else the
// smallest if one fits.  `forced` (PSXHIP_SCALER_TILE's text, or NULL; tests): only that shape, taken if one workgroup fits a CU --
// every shape can be run on purpose.  Fills the job's TW, TH, reg_*, creg_*, tiles_x, tiles_y and the banks' taps / taps4, and
// *lds_bytes; or one of the three refusals.
constexpr int kScalerShapes[4][2] = {{64, 16}, {32, 16}, {32, 8}, {16, 8}};
int scaler_choose_tile(const HostBank h[4], bool yuv, int dst_width, int dst_height, size_t lds_per_cu, const char* forced,
                       psxhip_scaler_job_t* j, size_t* lds_bytes);
// the LDS regions of a chosen tile (the total sized as the host sizes it: t_rows for all tiles_y tiles)
inline ScalerLds scaler_job_lds(const psxhip_scaler_job_t& j, bool yuv) { return scaler_lds(j, yuv, j.tiles_y); }

// Vertical segments per band: a band walks the picture top to bottom; a small batch is cut into segments until the chip has ~4
// workgroups per CU (each segment re-reads the rows its first tile reaches).  `override_` (PSXHIP_SCALER_VSEGS's text, or NULL;
// experiments) replaces the count; either way 1 .. tiles_y.
int scaler_vsegs(int n_cus, int tiles_x, int tiles_y, int n_frames, const char* override_);
// frames are gridDim.y: a call is cut into launches of at most this many
constexpr int kScalerLaunchFrames = 65535;
inline int scaler_launch_frames(int n_frames, int f0) { return n_frames - f0 < kScalerLaunchFrames ? n_frames - f0 : kScalerLaunchFrames; }

// psxhip_scaler_convert_device / _host in front of their HIP calls; *go: there is something to do.  (The host entry has no strides:
// it passes the sizes themselves.)
int scaler_convert_check(const char* who, bool handle, uintptr_t src, uintptr_t dst, int n_frames, bool device_entry, size_t src_stride,
                         size_t frame_stride, size_t src_bytes, int dst_width, int dst_height, bool* go);

// ---------------------------------------------------------------------------------------------- the picture ingest
struct IngestPlan {
    IngestDesc d;           // the source, with the matrix in exact integers
    int out_format;
    size_t src_bytes;       // from the picture's first byte to the end of its last plane
    size_t out_bytes;
};
// psxhip_ingest_create behind its handle pointer: the source's rules, the planes, the matrix
int ingest_create_plan(int src_format, int width, int height, const psxhip_ingest_plane_t* planes, int n_planes, int matrix, int full_range,
                       int out_format, uint32_t options, IngestPlan* out);
// the argument rules of a conversion (p: the handle's plan, or NULL); *go: there is something to do
int ingest_check(const char* who, const IngestPlan* p, uintptr_t src, size_t src_stride, int n_src, int n_out, uintptr_t dst, size_t out_stride,
                 bool device_pointers, bool* go);

// ---------------------------------------------------------------------------------------------- the display back-end
#pragma GCC visibility pop
/* the argument rules of "psxhip display v1", which need no device (sizes, format, options, pitch and stride; device_pointers: also
 * the pointers' alignment and that the pictures do not overlap the frames): PSXHIP_OK, or PSXHIP_EINVAL with the error text set,
 * `who` naming the entry point */
int psxhip_display_check(const char *who, const psxhip_display_job_t *j, bool device_pointers);
