// scaler_layout.h -- the scaler's job (what psxhip_scaler.cpp hands frontend_kernels.hip) and the LDS working set of scaler_kernel:
// the one carve both sides read.  The kernel places its regions by scaler_lds(); the host's tile choice (picture_plan.cpp) sizes a
// launch by the same function's total.  Constants and arithmetic only, no HIP: the kernel and a host compiler read the same text
// (PSX_LAYOUT_HD: the pattern of mdec_layout.h), so a region added here moves both.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PSX_LAYOUT_HD __host__ __device__ inline
#else
#define PSX_LAYOUT_HD inline
#endif

typedef struct {              /* one separable filter bank on the device */
	const int32_t *left;      /* [n] */
	const int16_t *coef;      /* [n * taps] */
	const uint32_t *digits;   /* [n * 2 * taps4] horizontal banks: the taps as two balanced int8 digits (c = 256 h + l), four taps
	                           *                 to a dword, zero-padded to taps4 dwords: first the l dwords, then the h dwords */
	int taps, taps4;
} psxhip_scaler_bank_t;

typedef struct {
	const uint8_t *src;
	size_t src_stride;
	uint8_t *out;
	size_t frame_stride;
	int sw, sh, dw, dh;
	int limited;              /* YUV input in MPEG range: expand on the intermediates */
	psxhip_scaler_bank_t lh, lv, ch, cv;      /* luma / chroma, horizontal / vertical */
	int csw, csh;             /* chroma source plane size (sw/2 x sh/2 for YUV420P, sw x sh for RGB) */
	int TW, TH;               /* luma tile; the chroma tile is TW/2 x TH/2 */
	int tiles_x, tiles_y;
	int vsegs;                /* vertical segments per band (blockIdx.z): each re-reads the rows its first tile reaches */
	int reg_rows, reg_cols;   /* LDS region capacity per plane (RGB: the union of the luma and chroma reach; YUV: luma) */
	int creg_rows, creg_cols; /* ... of a chroma plane (YUV) */
} psxhip_scaler_job_t;

// + 8 per plane: the horizontal pass reads a window as whole dwords, up to 7 bytes past the last tap (zero digits there)
constexpr int kScalerPlanePad = 8;
// bytes the total keeps behind the last region
constexpr int kScalerLdsSlack = 16;
// t_rows holds four dwords per tile of the longest segment.  The host sizes it for ALL tiles_y tiles (one segment), whatever vsegs a
// call then takes: the total is fixed when the handle is made, the segments per call.
constexpr int kScalerTileRowBytes = 16;

// byte offsets of the regions from the start of the dynamic LDS, in the order they lie; every one a multiple of four
struct ScalerLds {
    int plane_bytes, cplane_bytes;      // a luma / a chroma byte plane, rounded up to 16
    int ring_l, ring_c;                 // rows the rings of intermediates hold
    int v_words;                        // dwords of one tile's vertical tables: TH + TH/2 left entries, then the taps as int16 pairs
    int p0, p1, p2;                     // the three byte planes (the rows a tile adds)
    int tmp_l;                          // int16 [ring_l][TW]
    int tmp_c;                          // int16 [2][ring_c][TW/2]
    int g_lh, g_ch;                     // digit dwords [TW][2 * lh.taps4], [TW/2][2 * ch.taps4]
    int l_lh, l_ch;                     // int32 [TW], [TW/2]
    int v_tab;                          // two copies of the vertical tables, taken in turn
    int t_rows;                         // int32 [seg_tiles][4]
    int total;                          // ... and kScalerLdsSlack
};

// yuv: YUV420P (its chroma planes have a region of their own size), else RGB24 (three planes of the union reach);
// seg_tiles: tiles of the longest segment (only t_rows' length and the total depend on it)
PSX_LAYOUT_HD ScalerLds scaler_lds(const psxhip_scaler_job_t& j, bool yuv, int seg_tiles) {
    ScalerLds s;
    const int TW = j.TW, TH = j.TH, CW = TW >> 1, CH = TH >> 1;
    s.plane_bytes = (j.reg_rows * j.reg_cols + kScalerPlanePad + 15) & ~15;
    s.cplane_bytes = yuv ? ((j.creg_rows * j.creg_cols + kScalerPlanePad + 15) & ~15) : s.plane_bytes;
    s.ring_l = j.reg_rows;
    s.ring_c = yuv ? j.creg_rows : j.reg_rows;
    s.v_words = TH + CH + (TH * j.lv.taps + CH * j.cv.taps + 1) / 2;
    s.p0 = 0;
    s.p1 = s.p0 + s.plane_bytes;
    s.p2 = s.p1 + s.cplane_bytes;
    s.tmp_l = s.p2 + s.cplane_bytes;
    s.tmp_c = s.tmp_l + 2 * s.ring_l * TW;
    s.g_lh = s.tmp_c + 2 * 2 * s.ring_c * CW;
    s.g_ch = s.g_lh + 4 * TW * 2 * j.lh.taps4;
    s.l_lh = s.g_ch + 4 * CW * 2 * j.ch.taps4;
    s.l_ch = s.l_lh + 4 * TW;
    s.v_tab = s.l_ch + 4 * CW;
    s.t_rows = s.v_tab + 4 * 2 * s.v_words;
    s.total = s.t_rows + kScalerTileRowBytes * seg_tiles + kScalerLdsSlack;
    return s;
}
