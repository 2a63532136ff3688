/*
 * psxav_hip.h -- batched, device-resident extensions of the psxavenc hot path for MI355X (gfx950).
 *
 * The reference API encodes one frame / one 28-sample block per synchronous call
 * (psxavenc/mdec.h:65-74, libpsxav/libpsxav.h:73-101).  A kernel launch + copy per call costs
 * more than the work itself, so the throughput surface is batched: N frames (or N independent
 * ADPCM chains) per call, buffers already resident in HBM, asynchronous on a caller stream.
 * The per-call drop-in functions in psxav_mdec.h / psxav_audio.h are thin wrappers over these.
 *
 * Plain C ABI: pointers, sizes, ints.  Functions return 0 on success or a negative PSXHIP_E*
 * code; psxhip_last_error() gives the text for the calling thread.  "d_" parameters are device
 * pointers (hipMalloc / torch CUDA tensors), everything else is host memory.  `stream` is a
 * hipStream_t passed as void* (NULL = the null stream).
 */
#ifndef PSXAV_HIP_H
#define PSXAV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
	PSXHIP_OK = 0,
	PSXHIP_EINVAL = -1,     /* bad argument (size not a multiple of 16, NULL pointer, ...) */
	PSXHIP_EDEVICE = -2,    /* HIP runtime error / no gfx950 device */
	PSXHIP_ENOMEM = -3,
	PSXHIP_ENOFIT = -4      /* some frame does not fit its budget at any quant scale < 64 (the
	                           reference asserts here, psxavenc/mdec.c:723) */
};

int psxhip_device_count(void);
const char *psxhip_last_error(void);
const char *psxhip_version(void);

/* ---------------------------------------------------------------- MDEC BS frame encoder ---- */

/* what encode_frame_bs leaves in mdec_encoder_state_t (psxavenc/mdec.c:719-736) */
typedef struct {
	int32_t quant_scale;         /* 1..63; 64 = no scale fits (bytes_used = 0 then, and the frame_max_size bytes of its row are zero); PSXHIP_MDEC_QS_RELEASED: see below */
	int32_t bytes_used;          /* bitstream bytes incl. the 8-byte header, rounded up to 4 */
	int32_t blocks_used;         /* MDEC command word count */
	int32_t uncomp_hwords_used;  /* rounded up to 64 */
} psxhip_mdec_result_t;

/* quant_scale of a frame the split kernel's watchdog released (psxhip_mdec_encode_frames_device / _batches_device only): its
 * workgroups did not all arrive in time, so nothing is known about the frame -- the row is zero, the other fields are 0.  It is
 * not "does not fit": encode the frame again (the host-buffer entry points do that by themselves, through the frame kernel). */
#define PSXHIP_MDEC_QS_RELEASED 65

typedef struct psxhip_mdec_ctx psxhip_mdec_ctx_t;

/* codec: 0 = BS v2, 1 = v3, 2 = v3dc (bs_codec_t, psxavenc/args.h:61-65).
 * width/height: multiples of 16 (psxavenc/mdec.c:601-602), at most 1024 each.
 * max_frame_size: largest per-frame byte budget that will be passed (sizes the LDS staging).
 * A frame's working set (budget + min(budget, 8 KiB) + ~30 bytes per macroblock + ~37 KiB) must fit the CU's 160 KiB
 * LDS, else PSXHIP_EINVAL: e.g. 640x512 (the reference CLI's maximum, args.c:410-421) works up to 84 668-byte budgets;
 * psxhip_mdec_query_geometry() tells before creating a context. */
int psxhip_mdec_create(psxhip_mdec_ctx_t **ctx, int device, int codec, int width, int height,
                       int max_frame_size);
void psxhip_mdec_destroy(psxhip_mdec_ctx_t *ctx);

/* Encode n_frames NV21 frames (frame i at d_frames + i*frame_stride, w*h*3/2 bytes each) into
 * d_out + i*out_stride.  Exactly frame_max_size bytes are written per frame: header, bitstream,
 * zero fill -- what psxavenc/mdec.c:676,739-754 leave in frame_output.  d_frame_max_sizes may be
 * NULL, then every frame uses uniform_max_size.  d_frames, d_out, frame_stride and out_stride
 * must be 4-byte aligned.  Asynchronous on `stream`; results land in d_results[i].
 * Launches on ONE context must be stream-ordered (same stream, or ordered by events): the context owns the
 * frame hand-out counters the kernel uses.  Use one context per concurrent stream (or two launch lanes, psxhip_mdec_set_lanes).
 * Per-frame budgets (device memory, not vetted by the host) outside [8, min(the context's max_frame_size,
 * out_stride)] make that frame's result quant_scale 64 and write nothing.
 * Launches of at most 12 frames (PSXHIP_MDEC_SPLIT_MAX) cut every frame across many workgroups (csrc/mdec_split.inc: the
 * reference's call pattern is ONE frame per call, psxavenc/filefmt.c:641-647) -- same bytes, same results, same ordering rules.  Such
 * launches of one process are ordered one behind the other per device; a frame whose workgroups could not all become resident
 * within 0.2 s (another PROCESS holding the device's compute units) comes back with quant_scale PSXHIP_MDEC_QS_RELEASED and a zero
 * row, and is counted by psxhip_mdec_watchdog.  The host-buffer entry points (psxhip_mdec_encode_frames_host, encode_frame_bs,
 * the STR and multi-device calls) encode such a frame again through the one-workgroup kernel and return its exact bytes. */
int psxhip_mdec_encode_frames_device(psxhip_mdec_ctx_t *ctx, const uint8_t *d_frames, size_t frame_stride,
                                     int n_frames, const int32_t *d_frame_max_sizes, int uniform_max_size,
                                     uint8_t *d_out, size_t out_stride, psxhip_mdec_result_t *d_results,
                                     void *stream);

/* Several batches, ONE launch.  The reference's caller is one in-order loop over frames (psxavenc/filefmt.c:641-647); a caller
 * that holds a few batches -- four 1000-frame chunks of a file, say -- hands them over together and gets the behaviour of one
 * large batch (frames of all batches are drawn from one ticket counter: no launch boundary between them, the tail of one batch
 * is filled by the head of the next) without concatenating its buffers.  Bytes and results are those of one
 * psxhip_mdec_encode_frames_device call per batch.  frame_stride, out_stride and uniform_max_size are common to the batches; a
 * batch's d_frame_max_sizes may be NULL (uniform_max_size applies).  More than PSXHIP_MDEC_MAX_BATCHES batches are issued as
 * several launches.  Batches with n_frames == 0 are skipped. */
#define PSXHIP_MDEC_MAX_BATCHES 8
typedef struct {
	const uint8_t *d_frames;              /* n_frames NV21 frames, frame_stride apart */
	int32_t n_frames;
	int32_t reserved;
	const int32_t *d_frame_max_sizes;     /* [n_frames] or NULL */
	uint8_t *d_out;                       /* n_frames rows, out_stride apart */
	psxhip_mdec_result_t *d_results;      /* [n_frames] */
} psxhip_mdec_batch_t;
int psxhip_mdec_encode_batches_device(psxhip_mdec_ctx_t *ctx, const psxhip_mdec_batch_t *batches, int n_batches,
                                      size_t frame_stride, int uniform_max_size, size_t out_stride, void *stream);

/* Launch lanes.  With one lane (the default) a launch is an ordinary stream operation: it starts when everything before it on
 * `stream` is done, and everything after it on `stream` sees its results -- so consecutive launches of an in-order caller
 * (filefmt.c:641-647 is one) run strictly one after the other, and the GPU idles through every launch's tail (8 % at 1000
 * frames of 320x240: a launch ends when its slowest CU does).  With two lanes the context owns two sets of frame hand-out
 * counters and two internal streams, and psxhip_mdec_encode_frames_device / _batches_device on a caller stream S become:
 *   - INPUTS are stream-ordered: launch k starts when everything enqueued on S before call k is done;
 *   - RESULTS lag one call: when call k returns, S is ordered behind launches 0 .. k-1; launch k itself is ordered into S by the
 *     next encode call on the context or by psxhip_mdec_fence(ctx, S).  A caller that reads launch k's output (or reuses its
 *     input or output buffers) must have called one of the two first -- i.e. it double-buffers, which is what lets the head of
 *     launch k+1 fill the tail of launch k.
 * Bytes never depend on the number of lanes.  lanes: 1 or 2.  Switching waits for the context's outstanding launches, and so do
 * the host-buffer entry points of the same context (psxhip_mdec_encode_frames_host*, encode_frame_bs): they use both lanes, on the
 * context's own streams.  With ONE lane a device-path launch runs on the caller's stream with lane 0's hand-out counters and nothing
 * orders a later host-buffer call (encode_frame_bs included) behind it: a caller that mixes the two on one context synchronises
 * its stream first -- the rule above (launches on one context are stream-ordered) applies to the host entry points too. */
int psxhip_mdec_set_lanes(psxhip_mdec_ctx_t *ctx, int lanes);
/* order `stream` behind every launch of the context issued so far (a no-op with one lane) */
int psxhip_mdec_fence(psxhip_mdec_ctx_t *ctx, void *stream);
/* Waits for the context's launches and returns, in *lost, how often a watchdog gave a frame up: the retry queue's (a workgroup that
 * reserved a queue slot never filled it within about a second: a faulted or preempted workgroup -- that launch's results are
 * incomplete), and the split kernel's (a frame whose workgroups did not all arrive within 0.2 s: reported as
 * PSXHIP_MDEC_QS_RELEASED, or encoded again by the host-buffer entry points).  Each released frame counts once.  Never reset. */
int psxhip_mdec_watchdog(psxhip_mdec_ctx_t *ctx, unsigned *lost);

/* Same, host buffers: H2D, kernel, D2H, synchronise.  frame_max_sizes may be NULL (uniform).
 * Returns PSXHIP_ENOFIT if any frame could not be fitted (its result has quant_scale 64).  A frame the split kernel's watchdog
 * released is encoded again through the frame kernel: it never comes back as 64 or PSXHIP_MDEC_QS_RELEASED here.
 * The batch moves in chunks over two streams (the copies of one chunk overlap the kernel of the next).  Pageable `frames`
 * / `out` go through pinned staging buffers (a multi-threaded CPU copy per chunk); buffers that are page-locked --
 * hipHostMalloc, hipHostRegister or psxhip_host_register() below -- are read and written by DMA directly. */
int psxhip_mdec_encode_frames_host(psxhip_mdec_ctx_t *ctx, const uint8_t *frames, int n_frames,
                                   const int32_t *frame_max_sizes, int uniform_max_size, uint8_t *out,
                                   size_t out_stride, psxhip_mdec_result_t *results);

/* Refinement, "psxhip MDEC shed v1" (DESIGN.md section 21).  The encoder's first-fit loop picks the smallest scale N whose stream fits and
 * leaves unused whatever lies between that stream and the budget.  This call, made AFTER an encode on the same frames, rows and
 * results, tries every frame with 1 < N < 64 at M = N - 1: AC levels are zeroed in shed steps t = 1 .. 63 * max_magnitude (step t
 * zeroes every |level| <= m - 1, and every |level| <= m at zig-zag positions >= p, with m = 1 + (t - 1) / 63 and
 * p = 64 - ((t - 1) % 63 + 1)); t* is the first step whose stream fits the frame's budget by the encoder's own rule; the frame is
 * refined when the squared error of its AC coefficients against their reconstruction is then below the plain encode's.  A refined
 * frame's row is what encode_frame_bs would write for the shed levels at scale M (all frame_max_size bytes), and its result matches;
 * every other frame's row and result stay bit for bit as they were.  The DC is never touched.
 *   max_magnitude  1 .. 3
 *   d_refine       (may be NULL) one record per frame
 * Arguments, alignment rules and the vetting of per-frame budgets are those of psxhip_mdec_encode_frames_device; a frame whose
 * budget is outside the allowed range is left as it was.  Asynchronous on `stream`, nothing is read back; the call orders `stream`
 * behind every launch of the context first (as psxhip_mdec_fence does), so it is correct with one or two launch lanes.  The
 * workspace belongs to the context and grows on demand: calls on one context must be stream-ordered.  Refining rows that were refined
 * already is the caller's error (the result's scale is no longer the plain encode's).  PSXHIP_EINVAL, with the rule in the error text,
 * for a call outside these rules. */
typedef struct {
	int32_t shed_step;           /* t*, 0 = untouched or declined */
	int32_t shed_count;          /* AC levels zeroed (0 unless refined) */
	int64_t d_plain;             /* sum (F - R_N)^2 over the frame's AC coefficients; 0 when untouched or when no step fits */
	int64_t d_shed;              /* the same against the shed levels at scale M, at t* */
} psxhip_mdec_refine_t;
int psxhip_mdec_refine_frames_device(psxhip_mdec_ctx_t *ctx, const uint8_t *d_frames, size_t frame_stride, int n_frames,
                                     const int32_t *d_frame_max_sizes, int uniform_max_size, int max_magnitude,
                                     uint8_t *d_out, size_t out_stride, psxhip_mdec_result_t *d_results,
                                     psxhip_mdec_refine_t *d_refine, void *stream);
/* psxhip_mdec_encode_frames_host with the refinement between the kernel and the copy back: H2D, encode, refine, D2H, synchronise.
 * refine: (may be NULL) [n_frames].  A frame the split kernel's watchdog released is encoded again through the frame kernel and
 * comes back unrefined. */
int psxhip_mdec_encode_refine_frames_host(psxhip_mdec_ctx_t *ctx, const uint8_t *frames, int n_frames,
                                          const int32_t *frame_max_sizes, int uniform_max_size, int max_magnitude, uint8_t *out,
                                          size_t out_stride, psxhip_mdec_result_t *results, psxhip_mdec_refine_t *refine);
/* revision of the refinement's kernels */
const char *psxhip_mdec_shed_kernel_rev(void);

/* The 8x8 forward DCT alone, exactly as the frame kernel computes it: blocks = n_blocks * 64 level-shifted samples
 * (-128..127, raster order; what psxavenc/mdec.c:619-633 hands to AVDCT.fdct), coefs = the 64 coefficients per block
 * in raster order (the in-place result of mdec.c:640).  The FDCT is the one piece of the path the reference takes from
 * FFmpeg; tools/check_fdct_vs_ffmpeg.c uses this entry point to diff the device arithmetic against a real libavcodec. */
int psxhip_mdec_fdct_host(int device, const int16_t *blocks, int n_blocks, int16_t *coefs);

/* Name and grid of the kernel the last encode call launched (for bench.py's roofline block). */
const char *psxhip_mdec_kernel_name(void);

/* What a geometry costs, before creating a context for it.  A frame's working set lives in the CU's
 * 160 KiB LDS: the macroblock staging area (max_frame_size) + the frame image (whole, or one 8 KiB tile at a time when
 * that is what fits) + ~30 bytes per macroblock + ~37 KiB (two workgroups per CU when twice that fits, else one).  fits == 0 means psxhip_mdec_create would return PSXHIP_EINVAL; max_frame_size_limit
 * is the largest budget this frame size supports (320x240: 109 644 bytes, 640x480: 86 700, 640x512: 84 668). */
typedef struct {
	int32_t fits;
	int32_t groups_per_cu;          /* frames in flight per compute unit (2 or 1) */
	int32_t wavefronts_per_group;
	int32_t frames_in_flight;       /* persistent grid size = compute units * groups_per_cu */
	int32_t max_frame_size_limit;
	int32_t image_tile_bytes;       /* bytes of the frame image assembled in LDS at a time: the whole budget, or 8 / 4 / 2 KiB */
	int64_t lds_bytes_per_group;
	int64_t lds_bytes_per_cu;
} psxhip_mdec_geometry_t;
int psxhip_mdec_query_geometry(int device, int codec, int width, int height, int max_frame_size,
                               psxhip_mdec_geometry_t *out);

/* Diagnostics: when the context was created with PSXHIP_MDEC_STATS=1 in the environment, the kernel counts
 * [0] frames encoded, [1] passes over frames (1 per frame when the pilot's prediction held), [2..7] histogram of
 * passes per frame (0, 1, 2, 3, 4, >= 5).  Copies min(n, PSXHIP_MDEC_STATS_TOTAL) entries; zeros otherwise. */
#define PSXHIP_MDEC_STATS 8
/* after those, 4 entries per workgroup (the first PSXHIP_MDEC_TRACE_GROUPS groups of the last launch): start and end
 * time (100 MHz wall clock), frames encoded, reserved */
#define PSXHIP_MDEC_TRACE_GROUPS 1024
/* and then 16 time sums over all groups (100 MHz ticks).  Of each group's first thread, per phase: 0 ticket/idle, 1 reset +
 * DC pre-pass, 2 pilot, 3 passes over the frame, 4 offset scan + merge, 5 header + write-out.  Over all wavefronts: 6 time
 * spent waiting at group barriers, 7 residency; 8..13 the barrier time by barrier (frame start, DC pre-pass + pilot,
 * checkpoint, end of pass, search step, merge + write-out).  Word 2 of a group's trace record: frames | ticks from group
 * entry to the end of its prologue << 8 | ticks to the end of its first frame << 32. */
#define PSXHIP_MDEC_STATS_PHASE0 (PSXHIP_MDEC_STATS + 4 * PSXHIP_MDEC_TRACE_GROUPS)
/* and one word per frame of the last launch (the first PSXHIP_MDEC_TRACE_FRAMES frames): first guess | first checkpoint
 * verdict << 8 (7 bits) | bit 15: the frame's last pass stopped counting the scale below at its checkpoint (v2: its count was a
 * mixed lower bound) | answer << 16 | passes << 24 | from bit 32 one byte per pass for the first four: emit scale, or count
 * scale | 0x40; | 0x80 stopped at the checkpoint */
#define PSXHIP_MDEC_TRACE_FRAMES 2048
#define PSXHIP_MDEC_STATS_FRAME0 (PSXHIP_MDEC_STATS_PHASE0 + 16)
#define PSXHIP_MDEC_STATS_TOTAL (PSXHIP_MDEC_STATS_FRAME0 + PSXHIP_MDEC_TRACE_FRAMES)
int psxhip_mdec_read_stats(psxhip_mdec_ctx_t *ctx, unsigned long long *out, int n, int reset);

/* ---------------------------------------------------------------- MDEC BS frame decoder ---- */

/* The way back: bitstream -> quantised levels -> NV21 pixels, and the per-frame sum of squared errors of two sets of frames -- a
 * preview of what a player shows, a quality figure per frame, and a verify step that keeps up with the encoder.  The reference has
 * no decoder; the syntax is its encoder's (psxavenc/mdec.c:441-510), the reconstruction arithmetic is this library's own, in
 * integers ("psxhip MDEC reconstruct v1").  Arbitrary bytes are safe to decode: every read is bounded by the
 * frame's byte count, bits past the end read as 0, and a frame that does not parse gets a status, not a fault. */
enum {
	PSXHIP_DEC_OK = 0,
	PSXHIP_DEC_EHEADER = -1,      /* fewer than 8 bytes, or bytes 2..3 are not 00 38 */
	PSXHIP_DEC_EVERSION = -2,     /* version neither 2 nor 3 */
	PSXHIP_DEC_EPREMATURE = -3,   /* v2: the end code where a block's DC belongs */
	PSXHIP_DEC_EDC = -4,          /* v3: no DC size class starts with these bits */
	PSXHIP_DEC_EAC = -5,          /* no AC code starts with these bits */
	PSXHIP_DEC_EOVERRUN = -6,     /* a run leads past coefficient 63 */
	PSXHIP_DEC_EENDCODE = -7,     /* the blocks are not followed by the end code (0x1FF for v2, 0x3FF for v3) */
	PSXHIP_DEC_ETRUNCATED = -8    /* the end code lies past the frame's last byte */
};

typedef struct {
	int32_t status;              /* PSXHIP_DEC_*: the first error in stream order */
	int32_t quant_scale;         /* the header's field (0 when the magic is wrong) */
	int32_t version;             /* 2 or 3 (the header's field when it is neither; 0 when the magic is wrong) */
	int32_t bits_consumed;       /* payload bits up to and including the end code; 0 unless status is PSXHIP_DEC_OK */
} psxhip_mdec_decoded_t;

typedef struct psxhip_mdec_decoder psxhip_mdec_decoder_t;

/* width/height: multiples of 16, at most 1024 each.  dc_wrap: non-zero = v3 DC values wrap to 10 bits (streams of codec v3dc). */
int psxhip_mdec_decoder_create(psxhip_mdec_decoder_t **dec, int device, int width, int height, int dc_wrap);
void psxhip_mdec_decoder_destroy(psxhip_mdec_decoder_t *dec);

/* Decode n_frames bitstreams (frame i: d_bs_sizes[i] bytes at d_bs + i*bs_stride; d_bs_sizes NULL = uniform_size bytes each; a
 * size above bs_stride counts as bs_stride) -- rows as psxhip_mdec_encode_frames_device writes them, bytes_used or the whole
 * budget as the size.  d_bs and bs_stride must be 4-byte aligned.  Results:
 *   d_decoded[i]  always
 *   d_levels      (may be NULL) frame i's (width/16)*(height/16)*6 blocks of 64 int16 levels in zig-zag order, blocks in stream
 *                 order (macroblocks column-major; Cr, Cb, Y0..Y3), at d_levels + i*blocks*64
 *   d_frames      (may be NULL) the reconstructed NV21 frame at d_frames + i*frame_stride, the layout the encoder reads; 4-byte
 *                 aligned.  With d_levels NULL the levels pass through a workspace the context owns (grown on demand).
 * A frame whose status is not PSXHIP_DEC_OK leaves its levels unspecified and its pixels untouched; nothing outside the frame's own
 * rows is written.  Asynchronous on `stream`, nothing is read back; calls on one context must be stream-ordered. */
int psxhip_mdec_decode_frames_device(psxhip_mdec_decoder_t *dec, const uint8_t *d_bs, size_t bs_stride,
                                     const int32_t *d_bs_sizes, int uniform_size, int n_frames, int16_t *d_levels,
                                     uint8_t *d_frames, size_t frame_stride, psxhip_mdec_decoded_t *d_decoded, void *stream);
/* Same, host buffers (levels and frames back to back, either may be NULL): H2D, kernels, D2H, synchronise. */
int psxhip_mdec_decode_frames_host(psxhip_mdec_decoder_t *dec, const uint8_t *bs, size_t bs_stride, const int32_t *bs_sizes,
                                   int uniform_size, int n_frames, int16_t *levels, uint8_t *frames,
                                   psxhip_mdec_decoded_t *decoded);
/* d_sse[i][0..2] = sum of squared differences of frame i of d_a and of d_b over the Y, Cb and Cr samples: exact integers,
 * independent of the order of summation.  PSNR is the caller's arithmetic: 10 log10(255^2 * samples / sse).  Pointers and
 * frame_stride 4-byte aligned; asynchronous on `stream`. */
int psxhip_mdec_sse_device(int device, const uint8_t *d_a, const uint8_t *d_b, size_t frame_stride, int width, int height,
                           int n_frames, uint64_t *d_sse, void *stream);
/* revision of the decoder's kernels (profiles are keyed by it) */
const char *psxhip_mdec_decode_kernel_rev(void);

/* ---------------------------------------------------------------- display back-end: NV21 -> RGB ---- */

/* The decoder's last stage: NV21 frames, as the reconstruct kernel writes them, to pixels that can be shown -- 24-bit RGB, RGBX, or
 * the PlayStation frame buffer's 15-bit pixels, which is what the MDEC itself hands out.  It is the inverse of the front-end's
 * RGB24 -> NV21 for video, as the ADPCM decoder is for audio.  The arithmetic is this library's own, in integers ("psxhip display
 * v1"; >> is arithmetic), and the kernel is held to it bit for bit:
 *   chroma  replicate (default): pixel (x, y) takes chroma sample (x >> 1, y >> 1), as the MDEC does.
 *           PSXHIP_DISPLAY_CHROMA_BILINEAR: centre siting, per channel on the bytes: kx = x >> 1, fx = kx - 1 (even x) or kx + 1
 *           (odd x), ky and fy likewise from y, fx and fy clamped to the plane;
 *           v = (9 c[ky][kx] + 3 c[ky][fx] + 3 c[fy][kx] + c[fy][fx] + 8) >> 4 -- one rounding, not two passes.
 *   matrix  BT.601 full range, cr = Cr - 128, cb = Cb - 128, each result clamped to 0 .. 255:
 *           R = (65536 Y + 91881 cr + 32768) >> 16
 *           G = (65536 Y - 22553 cb - 46802 cr + 32768) >> 16
 *           B = (65536 Y + 116130 cb + 32768) >> 16
 *   RGB555  c5 = c8 >> 3, or with PSXHIP_DISPLAY_DITHER c5 = clamp(c8 + D[y & 3][x & 3], 0, 255) >> 3, the PlayStation GPU's
 *           table D = {-4, 0, -3, 1}, {2, -2, 3, -1}, {-3, 1, -4, 0}, {3, -1, 2, -2}; the pixel is the little-endian 16-bit word
 *           r5 | g5 << 5 | b5 << 10 | m << 15, m = 1 with PSXHIP_DISPLAY_MASK_BIT. */
enum {
	PSXHIP_OUT_RGB24 = 0,         /* bytes R, G, B (the scaler's PSXHIP_PIX_RGB24): 3 * width bytes a row */
	PSXHIP_OUT_RGBX32 = 1,        /* bytes R, G, B, 255: 4 * width */
	PSXHIP_OUT_RGB555 = 2         /* 16-bit pixels: 2 * width */
};
enum {
	PSXHIP_DISPLAY_CHROMA_BILINEAR = 1,
	PSXHIP_DISPLAY_DITHER = 2,    /* PSXHIP_OUT_RGB555 only */
	PSXHIP_DISPLAY_MASK_BIT = 4   /* PSXHIP_OUT_RGB555 only */
};

/* bytes of one row of pixels; 0 on a bad format */
size_t psxhip_display_row_bytes(int out_format, int width);
/* Convert n_frames NV21 frames (frame i at d_frames + i*frame_stride; width, height multiples of 16 in 16 .. 1024).  Picture i
 * starts at d_dst + i*dst_stride, its row y at + y*dst_pitch; dst_pitch >= the row bytes, dst_stride >= (height - 1)*dst_pitch + the
 * row bytes.  Only the row bytes of each row are written: what lies between rows and between pictures keeps its contents, so a
 * picture can be placed inside a larger surface.  d_frames, frame_stride, d_dst, dst_pitch and dst_stride are 4-byte aligned; d_dst
 * must not overlap d_frames.  With d_decoded (may be NULL; the decoder's records) a frame whose status is not PSXHIP_DEC_OK is
 * skipped and its picture keeps its contents.  PSXHIP_DISPLAY_DITHER or PSXHIP_DISPLAY_MASK_BIT with another format than
 * PSXHIP_OUT_RGB555, or an unknown option bit, is PSXHIP_EINVAL.  Asynchronous on `stream`. */
int psxhip_display_convert_device(int device, const uint8_t *d_frames, size_t frame_stride, int width, int height, int n_frames,
                                  const psxhip_mdec_decoded_t *d_decoded, int out_format, uint32_t options,
                                  uint8_t *d_dst, size_t dst_pitch, size_t dst_stride, void *stream);
/* Same, host buffers, frames and pictures back to back: H2D, kernel, D2H, synchronise. */
int psxhip_display_convert_host(int device, const uint8_t *frames, int width, int height, int n_frames, int out_format,
                                uint32_t options, uint8_t *dst);
/* psxhip_mdec_decode_frames_device followed by the conversion, gated by d_decoded: bitstreams in, pictures out, on the caller's
 * stream.  The NV21 frames pass through a workspace the context owns (grown on demand); nothing is read back.  The picture of a
 * frame that does not parse keeps its contents. */
int psxhip_mdec_decode_display_device(psxhip_mdec_decoder_t *dec, const uint8_t *d_bs, size_t bs_stride, const int32_t *d_bs_sizes,
                                      int uniform_size, int n_frames, psxhip_mdec_decoded_t *d_decoded, int out_format,
                                      uint32_t options, uint8_t *d_dst, size_t dst_pitch, size_t dst_stride, void *stream);
/* revision of the display kernels (profiles are keyed by it) */
const char *psxhip_display_kernel_rev(void);

/* ---------------------------------------------------------------- SPU / XA ADPCM ----------- */

/* carried state of one channel: the last two DECODED samples (libpsxav/adpcm.c:135-136).  The
 * reference's qerr is never updated and mse is per-trial scratch (adpcm.c:107,131-132). */
typedef struct {
	int32_t prev1, prev2;
} psxhip_adpcm_state_t;

/* One independent encoder chain: `n_units` consecutive 28-sample sound units read from
 * d_samples + sample_offset with stride `pitch` (int16 elements); chain-local samples at index
 * >= sample_limit read as zero without touching memory (what the reference gets from its zero-padded
 * input, adpcm.c:65,110 and decoding.c:497-503).  Unit u of the chain is written to record
 * unit_base[c] + u * unit_stride, so the L/R chains of a stereo XA stream interleave into encode order. */
typedef struct {
	int64_t sample_offset;   /* element offset into d_samples */
	int32_t pitch;           /* 1 = mono / planar, 2 = interleaved stereo */
	int32_t sample_limit;    /* valid samples of this chain from sample_offset on */
	int32_t n_units;         /* sound units to encode */
	int32_t unit_stride;     /* record stride, normally 1 (2 for the halves of a stereo pair) */
} psxhip_adpcm_chain_t;

#define PSXHIP_ADPCM_RECORD_BYTES 32   /* 8-bit codes: byte 0: (shift & 15) | filter << 4; bytes 1..3: zero; bytes 4..31: the 28 codes.  Also the upper bound of a record's size */
#define PSXHIP_ADPCM_RECORD_BYTES_4BIT 16   /* 4-bit codes (SPU, 4-bit XA): the layout of an SPU block (adpcm.c:367-372): header, 0, 14 bytes of two codes each (even sample low) */
#define PSXHIP_ADPCM_RECORD_SIZE(bits) ((bits) == 4 ? PSXHIP_ADPCM_RECORD_BYTES_4BIT : PSXHIP_ADPCM_RECORD_BYTES)   /* bytes between the records of consecutive unit indices */

/* Encode n_chains independent chains.  filter_count 5 (SPU) or 4 (XA); bits 4 or 8 (shift range
 * 12 / 8, adpcm.c:29-34).  Output: one record per unit (PSXHIP_ADPCM_RECORD_SIZE(bits) bytes apart, see above) in d_units; d_states[c]
 * is read and updated.  Result per unit == libpsxav/adpcm.c:142-191 encode().  Only the records of the chains' units are written.
 * d_units is 16-byte aligned when bits == 4 (a 4-bit record is stored, and read by psxhip_spu_pack_device and the sector builders, as
 * one 16-byte word -- the decoder's entry points ask the same of it) and 4-byte aligned when bits == 8; psxhip_adpcm_session_create
 * and psxhip_adpcm_encode_chains_chunked likewise.  Anything else is PSXHIP_EINVAL. */
int psxhip_adpcm_encode_chains_device(int device, const int16_t *d_samples, const psxhip_adpcm_chain_t *d_chains,
                                      const int32_t *d_unit_base, int n_chains, int filter_count, int bits,
                                      psxhip_adpcm_state_t *d_states, uint8_t *d_units, void *stream);

/* Same result as psxhip_adpcm_encode_chains_device, but parallel ALONG each chain ("speculate and verify"):
 * chains are cut into chunks of `chunk_units` sound units, every chunk is encoded concurrently from a guessed
 * start state (obtained by running `warmup_units` units before the chunk from a zero state), then verify
 * passes re-encode any chunk whose guess differs from its predecessor's actual end state, until a pass changes
 * nothing.  The fixpoint equals the serial encode bit for bit; the guesses only affect speed.  `chains` and
 * `unit_base` are HOST arrays here (the chunk tables are built on the host); the call synchronises.  d_states is read and written
 * in the order of `stream`, like d_samples and d_units: earlier asynchronous work on that stream that updates it is waited for.
 * max_passes <= 0: no limit (the worst case is one chunk per pass).  Returns the number of verify passes
 * (>= 1) or a negative error. */
int psxhip_adpcm_encode_chains_chunked(int device, const int16_t *d_samples, const psxhip_adpcm_chain_t *chains,
                                       const int32_t *unit_base, int n_chains, int filter_count, int bits,
                                       psxhip_adpcm_state_t *d_states, uint8_t *d_units, int chunk_units,
                                       int warmup_units, int max_passes, void *stream);

/* The same machinery as a persistent session, for sharding chains ALONG TIME across GPUs: a rank that owns units
 * [a, b) of a chain does not know the state at `a` until its predecessor has finished.  lead_units[c] > 0 makes the
 * session guess chain c's start state from up to `warmup_units` units located BEFORE the chain's sample_offset
 * (they must be readable); psxhip_adpcm_session_run() (re)verifies everything against the start states passed in --
 * call it again with corrected states after exchanging final states with the neighbour rank; it returns the
 * number of verify passes and sets *any_change when any record was (re)written.  The fixpoint over all ranks
 * (no rank changed) equals the serial encode.  See psxavenc_amd/parallel.py: encode_chains_time_sharded(). */
typedef struct psxhip_adpcm_session psxhip_adpcm_session_t;
int psxhip_adpcm_session_create(psxhip_adpcm_session_t **session, int device, const int16_t *d_samples,
                                const psxhip_adpcm_chain_t *chains, const int32_t *unit_base,
                                const int32_t *lead_units, int n_chains, int filter_count, int bits, uint8_t *d_units,
                                int chunk_units, int warmup_units, void *stream);
/* start_known (optional, [n_chains]): 0 = start_states[c] is not known yet -> keep the warm-up guess for chain c. */
int psxhip_adpcm_session_run(psxhip_adpcm_session_t *session, const psxhip_adpcm_state_t *start_states,
                             const uint8_t *start_known, int max_passes, psxhip_adpcm_state_t *final_states,
                             int *any_change);
/* Measurement: HIP events around the speculate launch and around the verify passes of every run that speculates (the first run
 * after create / reset); _last_timing returns the last such run's two durations in milliseconds.  Off by default. */
int psxhip_adpcm_session_set_timing(psxhip_adpcm_session_t *session, int on);
int psxhip_adpcm_session_last_timing(const psxhip_adpcm_session_t *session, float *speculate_ms, float *verify_ms);
/* revision of the ADPCM kernels (profiles/pmc_index.json is keyed by it, like the frame kernel's in psxhip_version()) */
const char *psxhip_adpcm_kernel_rev(void);
/* forget the speculative encode: the next psxhip_adpcm_session_run starts over (the samples may have changed) */
void psxhip_adpcm_session_reset(psxhip_adpcm_session_t *session);
void psxhip_adpcm_session_destroy(psxhip_adpcm_session_t *session);

/* Pack n_blocks unit records into 16-byte SPU blocks (adpcm.c:367-372).  d_units and d_out 16-byte aligned. */
int psxhip_spu_pack_device(int device, const uint8_t *d_units, int n_blocks, uint8_t *d_out, void *stream);

/* Assemble XA sectors from unit records in encode order (adpcm.c:193-233,266-332): sector s takes
 * records [s * 18 * U, (s+1) * 18 * U), U = 8 (4-bit) or 4 (8-bit) units per sound group.  Writes
 * 2336 (.xa, format 0) or 2352 (XACD, format 1) bytes per sector incl. sync, BCD time code,
 * subheaders and the form-2 EDC (libpsxav/cdrom.c:28-41,55-74,102-110); bytes the reference leaves
 * unwritten are zero.  d_eof_flags (optional): non-zero entries set the EOF submode bit
 * (psx_audio_xa_encode_finalize, adpcm.c:334-340). */
int psxhip_xa_assemble_device(int device, const uint8_t *d_units, int n_sectors, int format, int stereo,
                              int frequency, int bits, int file_number, int channel_number, int first_lba,
                              const uint8_t *d_eof_flags, uint8_t *d_out, void *stream);

/* Host-buffer batches.  n_streams independent streams, stream i at samples + i*stream_stride
 * (elements), samples_per_stream samples each read with `pitch`; states[i] is carried in and out.
 * SPU: stream i's 16 * ceil(n/28) bytes go to out + i*out_stride.  Returns bytes per stream or < 0. */
int psxhip_spu_encode_streams_host(int device, const int16_t *samples, int n_streams, int64_t stream_stride,
                                   int pitch, int samples_per_stream, psxhip_adpcm_state_t *states,
                                   uint8_t *out, int64_t out_stride);
/* XA: stereo streams are interleaved L,R (samples_per_stream counts per channel); states[2*i] /
 * states[2*i+1] are the left / right channel states; lbas[i] is the first sector's LBA.  finalize != 0
 * sets EOF on each stream's last sector.  Returns bytes per stream (whole sectors) or < 0. */
int psxhip_xa_encode_streams_host(int device, int format, int stereo, int frequency, int bits, int file_number,
                                  int channel_number, const int16_t *samples, int n_streams, int64_t stream_stride,
                                  int samples_per_stream, const int32_t *lbas, psxhip_adpcm_state_t *states,
                                  uint8_t *out, int64_t out_stride, int finalize);

/* ---- "psxhip ADPCM beam v1" (DESIGN.md section 22): a delayed decision inside the sound unit ----
 * The reference's encoder rounds every sample to the nearest code and ignores that a code also moves the predictor for the rest of
 * the unit.  The beam encoder tries the reference's own (filter, shift) candidates, but inside each keeps up to `beam` paths: path 0
 * is the reference's greedy one, the others the smallest-error children (codes q0, q0 - 1, q0 + 1 of every kept path) of the step
 * before.  A candidate's result is its best path, the unit's the first candidate with the smallest error.  Integers only; the rule
 * is stated in full in DESIGN.md and held bit for bit to tests/adpcm_beam_ref.py.
 *   beam == 1 is libpsxav/adpcm.c:142-191 bit for bit (the bytes of psxhip_adpcm_encode_chains_device).
 *   For every unit the winner's squared error is <= the reference encoder's for the same unit FROM THE SAME STATE.  That is a
 *   guarantee per unit, not per chain: behind the first unit that differs the two encoders carry different states.
 * The records are those of the plain encoder (PSXHIP_ADPCM_RECORD_SIZE(bits)) and go to the same packers, sector builders and
 * decoder.  The per-call drop-ins (psx_audio_spu_encode, psx_audio_xa_encode), the STR / STRSPU muxers, psxhip_spu_file_* and the
 * multi-device calls do not take a beam in this revision. */
#define PSXHIP_ADPCM_BEAM_MAX_WIDTH 4
/* The contract of psxhip_adpcm_encode_chains_device (asynchronous on `stream`, d_units' alignment, only the chains' records written).
 * beam 1 .. 4.  d_unit_err (optional, 4-byte aligned): one uint32_t per record index, the winner's squared error (saturating at
 * 2^32 - 1, which the winner never reaches), written for the chains' units only.  Anything else is PSXHIP_EINVAL. */
int psxhip_adpcm_beam_encode_chains_device(int device, const int16_t *d_samples, const psxhip_adpcm_chain_t *d_chains,
                                           const int32_t *d_unit_base, int n_chains, int filter_count, int bits, int beam,
                                           psxhip_adpcm_state_t *d_states, uint8_t *d_units, uint32_t *d_unit_err, void *stream);
/* psxhip_adpcm_encode_chains_chunked with the beam encoder: the same chunk tables and verify passes (the scheme is right for any
 * unit encoder that is a function of state and samples); the result is the serial beam call's bit for bit.  beam 1 .. 4. */
int psxhip_adpcm_beam_encode_chains_chunked(int device, const int16_t *d_samples, const psxhip_adpcm_chain_t *chains,
                                            const int32_t *unit_base, int n_chains, int filter_count, int bits,
                                            psxhip_adpcm_state_t *d_states, uint8_t *d_units, int beam, int chunk_units,
                                            int warmup_units, int max_passes, void *stream);
/* Which unit encoder a session's speculate and verify launches run: 0 the plain one (the default), 1 .. 4 the beam.  Valid before
 * the session's first run or after psxhip_adpcm_session_reset; otherwise PSXHIP_EINVAL (a session's records come from one encoder). */
int psxhip_adpcm_session_set_beam(psxhip_adpcm_session_t *session, int beam);
/* psxhip_spu_encode_streams_host / psxhip_xa_encode_streams_host with the beam encoder (beam 1 .. 4): the same serial / chunked
 * choice and the same packers. */
int psxhip_spu_encode_streams_host_beam(int device, const int16_t *samples, int n_streams, int64_t stream_stride,
                                        int pitch, int samples_per_stream, psxhip_adpcm_state_t *states,
                                        uint8_t *out, int64_t out_stride, int beam);
int psxhip_xa_encode_streams_host_beam(int device, int format, int stereo, int frequency, int bits, int file_number,
                                       int channel_number, const int16_t *samples, int n_streams, int64_t stream_stride,
                                       int samples_per_stream, const int32_t *lbas, psxhip_adpcm_state_t *states,
                                       uint8_t *out, int64_t out_stride, int finalize, int beam);
/* revision of adpcm_beam_kernels.hip */
const char *psxhip_adpcm_beam_kernel_rev(void);

/* ---------------------------------------------------------------- SPU / XA ADPCM decoder --- */

/* The way back: unit records (or SPU blocks, or XA sectors) -> int16 PCM, and the sums of squared errors of two sample sets per
 * sound unit and per chain -- an audio preview, an SNR figure per stream, a verify step behind encode + assemble, a decoder for
 * existing .xa / .vag material.  The arithmetic is "psxhip ADPCM decode v1" (DESIGN.md section 12), in integers: the reconstruction
 * inside the reference's encoder (libpsxav/adpcm.c:120-124, carried state :135-136).  For a unit with header byte h and codes c[i]:
 * R = 12 (4-bit) or 8 (8-bit), s = h & 15, f = h >> 4 (& 3 when filter_count is 4), (k1, k2) = filter f's taps (0, 0 for f >= 5),
 * t = sext16((c[i] << R) & 0xFFFF) >> s, d = clamp(t + ((k1 p1 + k2 p2 + 32) >> 6), -32768, 32767), then p2 = p1, p1 = d.
 * Any bytes decode: a filter number >= 5 and a shift > R are reported in the unit's flag byte, the formula is applied all the same. */
#define PSXHIP_ADPCM_FLAG_BAD_FILTER 1   /* unit flag: filter number >= 5 (decoded with k1 = k2 = 0) */
#define PSXHIP_ADPCM_FLAG_BAD_SHIFT 2    /* unit flag: shift above 12 (4-bit) / 8 (8-bit) */

/* Decode n_chains chains, each serially.  The input is unit records in exactly the encoder's layout and geometry: unit u of chain c
 * is the record unit_base[c] + u * unit_stride, PSXHIP_ADPCM_RECORD_SIZE(bits) bytes apart; a 4-bit record is an SPU block, so an
 * SPU / VAG body decodes as it lies (byte 1, the loop flags, is ignored).  d_units must be 16-byte aligned.  The output is int16
 * PCM written where the encoder would have read it (sample_offset, pitch, sample_limit, n_units of the same psxhip_adpcm_chain_t):
 * chain-local samples at index >= sample_limit are decoded -- they feed the state -- but NOT stored.  d_states[c] is read and
 * updated (values within int16 are the caller's contract; the encoder produces no others).  Optional outputs:
 *   d_unit_flags  one byte per record index: PSXHIP_ADPCM_FLAG_*
 *   d_tail        28 samples per chain (4-byte aligned): all of the unit that sample_limit cuts (unit sample_limit / 28 when
 *                 sample_limit is no multiple of 28), for psxhip_adpcm_sse_device; chains without such a unit leave theirs untouched
 * filter_count 5 (SPU) or 4 (XA); bits 4 or 8; 8 bits with filter_count 5 is PSXHIP_EINVAL.  Asynchronous on `stream`. */
int psxhip_adpcm_decode_chains_device(int device, const uint8_t *d_units, const psxhip_adpcm_chain_t *d_chains,
                                      const int32_t *d_unit_base, int n_chains, int filter_count, int bits,
                                      psxhip_adpcm_state_t *d_states, int16_t *d_samples, uint8_t *d_unit_flags, int16_t *d_tail,
                                      void *stream);

/* Same result, parallel ALONG each chain (speculate and verify, like psxhip_adpcm_encode_chains_chunked): chains are cut into chunks
 * of chunk_units units; every chunk but a chain's first guesses its start state by decoding up to warmup_units units in front of it
 * from a zero state; all chunks are decoded at once; verify passes decode again, from the truth, every chunk whose assumed start
 * differs from its predecessor's end, until a pass changes nothing.  The fixpoint equals the serial decode whatever the guesses were
 * -- and the passes are needed: with filter 1 and all codes 0 the states 0, 8 and -7 are all fixed points, so a wrong guess can
 * survive for ever.  `chains` and `unit_base` are HOST arrays; the call synchronises.  chunk_units <= 0: chosen by the library;
 * warmup_units < 0: 64.  max_passes <= 0: no limit (the worst case is one chunk per pass).  Returns the number of verify passes
 * (>= 1; 0 when there is nothing to decode) or a negative error.  When max_passes runs out before a pass changed nothing, the call
 * returns PSXHIP_EINVAL ("not converged"), d_states is left as it was, and d_samples / d_unit_flags / d_tail hold a decode that is
 * not verified: chunks behind a wrong guess may be wrong.  Call again with more passes. */
int psxhip_adpcm_decode_chains_chunked(int device, const uint8_t *d_units, const psxhip_adpcm_chain_t *chains,
                                       const int32_t *unit_base, int n_chains, int filter_count, int bits,
                                       psxhip_adpcm_state_t *d_states, int16_t *d_samples, uint8_t *d_unit_flags, int16_t *d_tail,
                                       int chunk_units, int warmup_units, int max_passes, void *stream);

/* Sums of squared errors of two int16 sample sets under one chain table: d_unit_sse (optional; needs d_unit_base) gets one sum
 * (a - b)^2 per sound unit at its record index -- uint64, a unit can pass 2^32 -- and d_chain_sums (optional) [c][0] = sum (a - b)^2,
 * [c][1] = sum b^2 over the chain: exact integers, independent of the order of summation.  dB are the caller's: 10 log10([1] / [0])
 * is the SNR of a against b.  Samples at index >= sample_limit take part as the encoder sees them: b reads as 0 without touching
 * memory; a is what the decoder computed there, which it did not store -- d_a_tail (optional) is the d_tail of the decode call, and
 * gives a for the unit sample_limit cuts; elsewhere past the limit (and without d_a_tail) a reads as 0 too.  With d_a the decode of
 * what was encoded from d_b, under the same chains, a unit's sum is the reference's state->mse after that unit (adpcm.c:131-132).
 * Asynchronous on `stream`. */
int psxhip_adpcm_sse_device(int device, const int16_t *d_a, const int16_t *d_a_tail, const int16_t *d_b,
                            const psxhip_adpcm_chain_t *d_chains, int n_chains, uint64_t *d_unit_sse, const int32_t *d_unit_base,
                            uint64_t *d_chain_sums, void *stream);

/* The inverse of psxhip_xa_assemble_device: n_sectors sectors of 2336 (format 0) or 2352 (format 1) bytes -> unit records in encode
 * order, sector s giving records [s * 18 * U, (s + 1) * 18 * U), U = 8 (4-bit) or 4 (8-bit).  d_sector_status (optional) gets per
 * sector the bits below; a sector with bits set is disassembled all the same.  Pointers 4-byte aligned; asynchronous. */
#define PSXHIP_XA_STATUS_HEADER_COPY 1   /* a sound group's header copy differs: bytes 4..7 against 0..3, or 12..15 against 8..11 */
#define PSXHIP_XA_STATUS_SUBHEADER 2     /* the two subheaders differ */
#define PSXHIP_XA_STATUS_CODING 4        /* the coding byte disagrees with the call's stereo / frequency / bits */
#define PSXHIP_XA_STATUS_EDC 8           /* the EDC is non-zero and wrong (a sector with EOF set may carry the EDC of the sector
                                            without EOF: psx_audio_xa_encode_finalize leaves it so, adpcm.c:334-340) */
int psxhip_xa_disassemble_device(int device, const uint8_t *d_sectors, int n_sectors, int format, int stereo, int frequency,
                                 int bits, uint8_t *d_units, int32_t *d_sector_status, void *stream);

/* Host-buffer conveniences mirroring the encode ones.  SPU: stream i's n_blocks 16-byte blocks at blocks + i * in_stride (bytes) ->
 * 28 * n_blocks samples at samples + i * out_stride (elements); states[i] is carried in and out.  Returns samples per stream or < 0. */
int psxhip_spu_decode_streams_host(int device, const uint8_t *blocks, int n_streams, int64_t in_stride, int n_blocks,
                                   psxhip_adpcm_state_t *states, int16_t *samples, int64_t out_stride);
/* XA: stream i's n_sectors sectors at sectors + i * in_stride (bytes) -> samples per channel = n_sectors * (4-bit ? 4032 : 2016) /
 * (stereo ? 2 : 1), interleaved L,R when stereo, at samples + i * out_stride (elements); states[2 * i] / states[2 * i + 1] are the
 * left / right channel states (mono: states[i]).  sector_status (optional): [n_streams][n_sectors] PSXHIP_XA_STATUS_* bits.
 * Returns samples per channel and stream or < 0. */
int psxhip_xa_decode_streams_host(int device, int format, int stereo, int frequency, int bits, const uint8_t *sectors, int n_streams,
                                  int64_t in_stride, int n_sectors, psxhip_adpcm_state_t *states, int16_t *samples, int64_t out_stride,
                                  int32_t *sector_status);
/* Measurement: with the calling thread's switch on, psxhip_adpcm_decode_chains_chunked puts HIP events around its speculate launch
 * and around its verify passes; _last_timing returns the thread's last such call's two durations in milliseconds.  Off by default. */
int psxhip_adpcm_decode_set_timing(int on);
int psxhip_adpcm_decode_last_timing(float *speculate_ms, float *verify_ms);
/* revision of the ADPCM decoder's kernels (profiles are keyed by it) */
const char *psxhip_adpcm_decode_kernel_rev(void);

/* The host-buffer ADPCM entry points keep their device scratch buffers per calling thread between calls (the reference
 * calls them once per 28 samples / once per sector); this releases the calling thread's. */
void psxhip_release_scratch(void);

/* Page-lock a caller-owned host buffer (hipHostRegister) so that the *_host entry points move it by DMA without a
 * staging copy; worth it for buffers that live across many calls (registration costs about as much as copying the
 * buffer once).  Unregister before freeing the memory. */
int psxhip_host_register(void *p, size_t bytes);
int psxhip_host_unregister(void *p);

/* ---------------------------------------------------------------- several devices behind one call ---- */

/* The reference's host side is one C loop (psxavenc/filefmt.c:633-662 over frames, :450-503 over sectors): a C caller has
 * no ranks to shard over, so these entry points take a device LIST and shard inside the call -- one host thread, one
 * encoder context and one pair of pinned staging buffers per list entry.  Frames (mdec.c:678-686: every attempt resets all
 * bit / DC state) and XA streams (adpcm.c:202-209: a state per channel) are independent units, so the bytes are those of
 * the single-device call whatever the schedule.  A device may be listed more than once.  The host-buffer path is bound by
 * the PCIe link of each device (about 440 k 320x240 frames/s), which is what several devices multiply. */

/* contiguous block partition of n_units over `world` workers: the first n_units % world workers get one unit more
 * (the same partition psxavenc_amd/parallel.py:shard_range uses across ranks) */
void psxhip_shard_range(int64_t n_units, int rank, int world, int64_t *first, int64_t *count);

/* host-side ticket queue: [0, n_units) handed out in ranges of ticket_units, in order, each exactly once, to any number
 * of threads (one atomic counter in host memory; no device collective).  _next returns 0 when the queue is empty. */
typedef struct psxhip_ticket_queue psxhip_ticket_queue_t;
psxhip_ticket_queue_t *psxhip_ticket_queue_create(int64_t n_units, int64_t ticket_units);
int psxhip_ticket_queue_next(psxhip_ticket_queue_t *q, int64_t *first, int64_t *count);
void psxhip_ticket_queue_destroy(psxhip_ticket_queue_t *q);

enum {
	PSXHIP_SCHED_STATIC = 0,    /* worker d takes psxhip_shard_range(n, d, n_devices) */
	PSXHIP_SCHED_TICKETS = 1    /* workers draw ranges of ticket_frames frames from a ticket queue until it is empty: a device
	                               that drew expensive frames (content at a scale boundary costs up to 1.5x) draws fewer */
};

/* what each worker did (optional out-parameter, one entry per listed device, at most PSXHIP_MULTI_MAX_REPORT) */
#define PSXHIP_MULTI_MAX_REPORT 64
typedef struct {
	int32_t device;
	int64_t units;       /* frames / streams this worker encoded */
	int32_t tickets;     /* ranges it drew */
	double seconds;      /* wall time from the start of the call to this worker's end */
} psxhip_multi_report_t;

typedef struct psxhip_mdec_multi psxhip_mdec_multi_t;
int psxhip_mdec_multi_create(psxhip_mdec_multi_t **m, const int *devices, int n_devices, int codec, int width, int height,
                             int max_frame_size);
void psxhip_mdec_multi_destroy(psxhip_mdec_multi_t *m);
int psxhip_mdec_multi_device_count(const psxhip_mdec_multi_t *m);
/* psxhip_mdec_encode_frames_host over all listed devices; same arguments, same bytes, same results, same return value.
 * ticket_frames <= 0: a default (1536 frames, halved until every device gets about 8 tickets). */
int psxhip_mdec_multi_encode_frames_host(psxhip_mdec_multi_t *m, const uint8_t *frames, int n_frames,
                                         const int32_t *frame_max_sizes, int uniform_max_size, uint8_t *out,
                                         size_t out_stride, psxhip_mdec_result_t *results, int schedule, int ticket_frames,
                                         psxhip_multi_report_t *report);

/* psxhip_xa_encode_streams_host with the streams sharded over the listed devices (contiguous stream ranges, e.g. the 8
 * XA channels of config `xacd` on 8 GPUs); same bytes and states. */
int psxhip_xa_encode_streams_host_multi(const int *devices, int n_devices, int format, int stereo, int frequency, int bits,
                                        int file_number, int channel_number, const int16_t *samples, int n_streams,
                                        int64_t stream_stride, int samples_per_stream, const int32_t *lbas,
                                        psxhip_adpcm_state_t *states, uint8_t *out, int64_t out_stride, int finalize,
                                        psxhip_multi_report_t *report);

/* ---------------------------------------------------------------- STR / STRCD / STRV muxer -- */

/* The reference's encode_file_str (psxavenc/filefmt.c:391-520) for inputs that are all there up front: every frame goes
 * through ONE batched MDEC call (the per-frame budgets are a closed-form function of the frame index, mdec.c:768-775),
 * sharded over the handle's devices; the audio is one XA stream encoded concurrently by the ADPCM kernels, and the host
 * interleaves 2016-byte slices of the finished frames with the finished audio sectors on the reference's sector schedule
 * ((sector % interleave) > 0 = video, filefmt.c:454-461).  Fields mirror args_t (psxavenc/args.h). */
enum {
	/* How the stream ends.  REFERENCE (default, 0) = the CLI's sector loop fed by its decoder (decoding.c:510-560) when the
	 * whole input is there: end_of_input is raised as soon as no more than `frames_needed` (>= 2, filefmt.c:443-446) frames or
	 * no more than one sector's worth of audio are left; the loop then runs until the frame in progress is written out
	 * (filefmt.c:450) -- the last frames_needed frames of the input are NOT encoded (the FIXME at filefmt.c:442), a stream
	 * whose audio is shorter than its video ends with the audio -- every audio sector from that point on carries EOF
	 * (:492-493), and an audio slot with no samples left is an all-zero sector that also widens the video share of the
	 * trailing-audio schedule (:483-484).
	 * COMPLETE = every frame is encoded, the stream ends with the last frame's last sector, short audio is padded with
	 * silence and only the last audio sector carries EOF (what a caller who wants all of its frames in the file asks for). */
	PSXHIP_STR_TAIL_REFERENCE = 0,
	PSXHIP_STR_TAIL_COMPLETE = 1
};

typedef struct {
	int32_t format;             /* format_t: 6 = STR (2336-byte sectors), 7 = STRCD (2352), 9 = STRV (2048), 8 = STRSPU (2048, below) */
	int32_t video_codec;        /* bs_codec_t */
	int32_t video_width, video_height;
	int32_t str_fps_num, str_fps_den;
	int32_t str_cd_speed;       /* 1 or 2 */
	int32_t str_video_id;       /* 0x8001 */
	int32_t trailing_audio;     /* FLAG_STR_TRAILING_AUDIO: audio sector last in each block instead of first */
	int32_t audio_channels;     /* 0 = no audio stream (all sectors are video), 1, 2 */
	int32_t audio_frequency;    /* 18900 / 37800; STRSPU: any rate the CD speed can carry */
	int32_t audio_bit_depth;    /* 4 / 8 (STRSPU: ignored) */
	int32_t audio_xa_file, audio_xa_channel;   /* (STRSPU: ignored) */
	int32_t tail_mode;          /* PSXHIP_STR_TAIL_* */
	int32_t strspu_options;     /* STRSPU: audio chunk id | PSXHIP_STRSPU_*; any other bit set is PSXHIP_EINVAL.  Formats 6 / 7 / 9 ignore it */
} psxhip_str_settings_t;

/* Format 8, STRSPU ("psxhip STRSPU v1"): .str video chunks interleaved with chunks of SPU-ADPCM audio in plain
 * 2048-byte sectors -- the format the reference lists and leaves unimplemented (filefmt.c:522-631).  A video sector is STRV's.  An
 * audio sector is a 32-byte chunk header (60 01, the audio chunk id, index 0 of 1, the chunk's number from 1, 2016, channels, lane
 * bytes L, frequency, first sample, flags) and 126 SPU blocks: B = 126 / channels per channel, channel c's lane at 0x20 + c * L,
 * L = 16 B; the lanes are an SPUI file of interleave L (leading dummy block, loop flag or trap block at the end of a chunk,
 * filefmt.c:323-371).  Audio sectors are the share audio_frequency / (28 B * 75 * str_cd_speed) of the stream, which must be below 1:
 * among the first n sectors ceil(n p / q) are audio (floor with trailing_audio).  Only PSXHIP_STR_TAIL_COMPLETE is defined.  With
 * audio_channels 0 the stream is byte for byte the STRV stream. */
#define PSXHIP_STRSPU_ID_MASK 0xFFFF             /* bits 0-15: the audio chunk id (args_t.str_audio_id, default 0x0001), taken literally */
#define PSXHIP_STRSPU_LOOP 0x10000               /* FLAG_SPU_ENABLE_LOOP (-L): every chunk's last block carries the repeat flag, no trap block */
#define PSXHIP_STRSPU_NO_LEADING_DUMMY 0x20000   /* -D: the lanes do not start with a silent block */

typedef struct {
	int32_t n_sectors;
	int32_t n_video_sectors, n_audio_sectors;   /* audio slots, incl. those with no samples left */
	int32_t sector_size;        /* 2336, 2352 or 2048 */
	int32_t interleave;         /* sectors per block: 1 audio + (interleave - 1) video (STRSPU: q / p when that is whole, else 0) */
	int32_t audio_samples_per_sector;   /* per channel */
	int32_t max_frame_size;     /* largest per-frame budget */
	int32_t n_frames_encoded;   /* frames that are part of the stream (REFERENCE tail: n_frames - frames_needed, or fewer when
	                               the audio ends first) */
	int64_t quant_scale_sum;    /* filled by psxhip_str_encode_host (mdec_encoder_state_t.quant_scale_sum) */
} psxhip_str_plan_t;

/* sector counts and sizes for n_frames frames and pcm_samples_per_channel samples of audio (what a caller needs to size the
 * output; the amount of audio matters because the reference's stream ends with whichever input ends first) */
int psxhip_str_plan(const psxhip_str_settings_t *settings, int n_frames, int64_t pcm_samples_per_channel,
                    psxhip_str_plan_t *plan);
/* what each sector of the stream holds, in stream order: returns the sector count (= plan.n_sectors) and fills
 * min(cap, count) entries */
enum { PSXHIP_STR_SECTOR_VIDEO = 0, PSXHIP_STR_SECTOR_AUDIO = 1, PSXHIP_STR_SECTOR_EMPTY = 2 /* audio slot, no samples left */ };
typedef struct {
	int32_t kind;
	int32_t frame;      /* video: 0-based frame; else -1 */
	int32_t index;      /* video: chunk index inside the frame (mdec.c:794); audio: index of the XA sector; empty: -1 */
	int32_t eof;        /* audio: the sector carries the EOF submode bit */
} psxhip_str_sector_t;
int psxhip_str_plan_sectors(const psxhip_str_settings_t *settings, int n_frames, int64_t pcm_samples_per_channel,
                            psxhip_str_sector_t *sectors, int cap);
/* frame_max_size of frames first_frame .. first_frame + n_frames - 1 (so that any rank can budget its own frame range) */
int psxhip_str_frame_budgets(const psxhip_str_settings_t *settings, int first_frame, int n_frames, int32_t *budgets);

/* A muxer handle owns what is kept between calls: the encoder contexts (device buffers, pinned staging) of the listed
 * devices and the page-locked buffer the bitstreams land in.  Handles are independent (no process-global state); calls
 * on ONE handle are serialised. */
typedef struct psxhip_str_ctx psxhip_str_ctx_t;
int psxhip_str_create(psxhip_str_ctx_t **ctx, const int *devices, int n_devices);
void psxhip_str_destroy(psxhip_str_ctx_t *ctx);
/* frames: n_frames NV21 frames back to back (w*h*3/2 bytes each); pcm: int16, interleaved L,R when stereo,
 * pcm_samples_per_channel of them.  out: plan.n_sectors * sector_size bytes.  Sector bytes the reference leaves unwritten
 * (it muxes into an uninitialised stack buffer) are zero. */
int psxhip_str_encode_host(psxhip_str_ctx_t *ctx, const psxhip_str_settings_t *settings, const uint8_t *frames, int n_frames,
                           const int16_t *pcm, int64_t pcm_samples_per_channel, uint8_t *out, size_t out_size,
                           psxhip_str_plan_t *plan);

/* The same, device-resident: frames and PCM in HBM, muxed sectors in HBM -- no PCIe, no host interleave -- for n_streams independent
 * streams of the same settings and lengths (stream i: frames at d_frames + i * frames_stream_stride bytes, PCM at d_pcm + i *
 * pcm_stream_stride int16 elements, sectors at d_out + i * out_stream_stride bytes; strides and pointers 4-byte aligned).  The frames
 * of all streams are one batched MDEC launch, the XA tracks chains of one speculate-and-verify session (S x 2 chains share the
 * verify passes' latency, which is what bounds ONE stream), the video sectors are built by a kernel (sector header, subheaders,
 * chunk header mdec.c:782-820, 2016-byte slice :832, form-1 EDC cdrom.c:92-100) and the audio sectors assembled into their slots
 * (filefmt.c:454-461).  Runs on devices[0] of the handle; `stream` orders the inputs; the call returns when the sectors are complete
 * (the host drives the verify passes).  Bytes = psxhip_str_encode_host per stream; plan->quant_scale_sum is summed over all streams.
 * Tables and buffers are kept in the handle for the next call of the same shape. */
int psxhip_str_encode_device(psxhip_str_ctx_t *ctx, const psxhip_str_settings_t *settings, int n_streams, const uint8_t *d_frames,
                             size_t frames_stream_stride, int n_frames, const int16_t *d_pcm, int64_t pcm_stream_stride,
                             int64_t pcm_samples_per_channel, uint8_t *d_out, size_t out_stream_stride, psxhip_str_plan_t *plan,
                             void *stream);

/* The audio sector builder of format 8 on its own (as psxhip_xa_assemble_device is for XA): n_sectors audio sectors of 2048 bytes per
 * stream from SPU unit records.  d_units: per stream n_sectors * 126 records of 16 bytes (PSXHIP_ADPCM_RECORD_BYTES_4BIT), unit u of
 * channel c at record u * channels + c (the order of one chain per channel with unit_stride = channels), 16-byte aligned, the streams
 * units_stream_stride bytes (a multiple of 16) apart.  A channel has U = n_sectors * 126 / channels - 1 units (one more with
 * PSXHIP_STRSPU_NO_LEADING_DUMMY: no block is spent on the dummy); records behind them are not read.  n_sectors is the stream's whole
 * audio: the last sector carries the trap block and the last-chunk flag.  Sector k of stream i goes to d_out + i * out_stream_stride
 * + d_dst_sector[k] * 2048 (d_dst_sector NULL: dense, slot k); d_out and out_stream_stride 4-byte aligned.  channels 1 or 2;
 * options as strspu_options.  Asynchronous on `stream`; nothing is read back. */
int psxhip_strspu_audio_sectors_device(int device, const uint8_t *d_units, int n_sectors, int channels, int frequency,
                                       uint32_t options, int n_streams, size_t units_stream_stride, uint8_t *d_out,
                                       const int32_t *d_dst_sector, size_t out_stream_stride, void *stream);
/* revision of the STRSPU audio sector kernel */
const char *psxhip_strspu_kernel_rev(void);

/* ---------------------------------------------------------------- STR / STRCD / STRV reader -- */

/* The way back for a whole stream: muxed sectors in HBM -> every frame's bitstream as one row (what psxhip_mdec_decode_frames_device
 * reads), the XA sectors compacted in stream order (what psxhip_xa_disassemble_device reads), one record per frame saying whether it
 * is whole, and optionally what every sector was.  The inverse of the sector schedule and of the video sector kernel; the rules are
 * "psxhip STR demux v1" (restated in tests/str_demux_ref.py) and are defined for arbitrary bytes: every index
 * taken from the stream is bounded before it is used, and bad input gives status bits, never a fault.
 *
 * Per format (6 / 7 / 9): sector size 2336 / 2352 / 2048, subheader `sub` at 0 / 0x10 / none, chunk header (mdec.c:782-820) at
 * P = 8 / 0x18 / 0 (mdec.c:822-829).  A sector is
 *   audio  when the format has subheaders, settings->audio_channels != 0, sub[2] & 0x04, sub[0] == audio_xa_file (or that is -1) and
 *          (sub[1] & 0x1F) == (audio_xa_channel & 0x1F) (or that is -1);
 *   video  when it is not audio, the format is STRV or (sub[2] & 0x04) == 0, bytes P, P+1 are 60 01 and le16(P+2) == str_video_id (or
 *          that is -1);
 *   other  else (the all-zero sector of an audio slot with no samples left is one).
 * A video sector belongs to row = frame_index - first_frame (64-bit; frame_index = le32(P+8), unsigned); outside [0, max_frames) it
 * is dropped: counted, and it touches nothing.  It is placeable when chunk_index < chunk_count (le16(P+4), le16(P+6), its own) and
 * (chunk_index + 1) * 2016 <= bs_stride; of the placeable sectors of one (row, chunk_index) the one at the lowest stream position is
 * placed: its 2016 payload bytes (P+0x20) go to d_bs + row * bs_stride + chunk_index * 2016.  Row bytes no placed chunk covers are
 * left as they were.  The lead of a row is its sector with chunk_index 0 at the lowest position, or without one its sector at the
 * lowest position; the frame's fields are the lead's. */
enum {
	PSXHIP_STR_FRAME_MISSING = 1,     /* no sector in the row, or chunk_count 0, or an index in [0, chunk_count) without a placed sector */
	PSXHIP_STR_FRAME_DUPLICATE = 2,   /* two placeable sectors share a chunk_index */
	PSXHIP_STR_FRAME_MISMATCH = 4,    /* a sector's chunk_count / bytes_used / width / height / BS-header copy differs from the lead's, or
	                                     the lead has chunk_index 0 and its BS-header copy differs from the first 8 bytes of its payload */
	PSXHIP_STR_FRAME_RANGE = 8,       /* a sector of the row is not placeable */
	PSXHIP_STR_FRAME_EDC = 16,        /* a sector of the row fails the EDC rule below */
	PSXHIP_STR_FRAME_GEOMETRY = 32    /* settings->video_width / video_height is non-zero and differs from the lead's */
};
/* EDC rule for video sectors, c(a..b) = the CD-ROM EDC of those sector bytes (cdrom.c:28-41).  STRV: no check.  STRCD: bad iff
 * le32(0x818) is neither 0 nor c(0x10..0x817).  STR: good iff le32(0x818) == c(0x10..0x817) (where the reference's muxer puts it: it
 * hands the 2336-byte buffer to psx_cdrom_calculate_checksums as if it had 2352, filefmt.c:474), or le32(0x808) == c(0..0x807) (where
 * it lies on a disc), or both stored words are 0.  Audio sectors are not checked here (psxhip_xa_disassemble_device does that). */

typedef struct {
	uint32_t frame_index;        /* the lead's fields: le32(P+8) */
	int32_t chunk_count;         /* le16(P+6) */
	int32_t chunks_placed;       /* chunk indices of the row that got a placed sector */
	uint32_t bytes_used;         /* le32(P+0xC) */
	int32_t width, height;       /* le16(P+0x10), le16(P+0x12) */
	int32_t first_sector;        /* the lead's position in the stream */
	int32_t status;              /* PSXHIP_STR_FRAME_* bits; a row without a sector: PSXHIP_STR_FRAME_MISSING and all else 0 */
} psxhip_str_frame_info_t;

typedef struct {
	int32_t n_video, n_audio, n_other;   /* sectors by kind (dropped ones included) */
	uint32_t first_frame;        /* the first_frame in effect; 0 when the stream has no video sector */
	int32_t n_rows;              /* 1 + the highest row a sector fell into, or 0 */
	int32_t n_complete;          /* rows without PSXHIP_STR_FRAME_MISSING */
	int32_t n_dropped_video;     /* video sectors with a row outside [0, max_frames) */
	int32_t n_dropped_audio;     /* audio sectors with an ordinal >= xa_capacity */
} psxhip_str_summary_t;

/* A reader handle owns the workspace (grown on demand) and, for psxhip_str_read_host, the device buffers and the decoder context.
 * Calls on one handle must be stream-ordered. */
typedef struct psxhip_str_reader psxhip_str_reader_t;
int psxhip_str_reader_create(psxhip_str_reader_t **reader, int device);
void psxhip_str_reader_destroy(psxhip_str_reader_t *reader);

/* Take n_streams streams of n_sectors sectors apart (stream i: sectors at d_sectors + i * in_stream_stride, rows at d_bs + i *
 * bs_stream_stride, XA sectors at d_xa + i * xa_stream_stride; d_bs_sizes, d_frame_info are [n_streams][max_frames], d_sector_table
 * [n_streams][n_sectors], d_summary [n_streams]).  Of the settings only format, str_video_id, audio_channels, audio_xa_file,
 * audio_xa_channel, video_width and video_height are read.
 *   first_frame    >= 0: the frame_index of row 0; -1: the smallest frame_index of the stream's video sectors (found on the device)
 *   d_bs_sizes     [row] = chunk_count * 2016, or 0 when the row is MISSING -- so psxhip_mdec_decode_frames_device reports a frame
 *                  that is not whole as PSXHIP_DEC_EHEADER and the two calls compose without a host decision
 *   d_frame_info   every row in [0, max_frames) is written
 *   d_xa           the audio sector with ordinal k (the number of audio sectors before it in its stream) is copied whole to d_xa + k *
 *                  sector size when k < xa_capacity, else counted as dropped; may be NULL when xa_capacity is 0
 *   d_sector_table (optional) psxhip_str_sector_t per sector: video {0, row or -1 when dropped, chunk_index, the RANGE / EDC bits this
 *                  sector contributed}; audio {1, -1, k, bit 0 = the EOF submode bit 0x80}; other {2, -1, -1, 0}.  For a stream this
 *                  library muxed, read with first_frame 1, it equals psxhip_str_plan_sectors' table.
 * Pointers and strides are 4-byte aligned, bs_stride is at least 2016, n_streams at most 65535; n_sectors == 0 is valid (every row
 * MISSING, a zero summary).  Asynchronous on `stream`; nothing is read back. */
int psxhip_str_demux_device(psxhip_str_reader_t *reader, const psxhip_str_settings_t *settings, int n_streams, const uint8_t *d_sectors,
                            size_t in_stream_stride, int n_sectors, int64_t first_frame, int max_frames, uint8_t *d_bs, size_t bs_stride,
                            size_t bs_stream_stride, int32_t *d_bs_sizes, psxhip_str_frame_info_t *d_frame_info, uint8_t *d_xa,
                            int xa_capacity, size_t xa_stream_stride, psxhip_str_sector_t *d_sector_table,
                            psxhip_str_summary_t *d_summary, void *stream);

/* The whole reader for one stream in host memory: H2D, demux, one read-back of the summary (the only synchronisation before the end),
 * psxhip_mdec_decode_frames_device over the max_frames rows with the demuxed sizes (dc_wrap from video_codec, the picture size from
 * the settings), psxhip_xa_disassemble_device and the chunked ADPCM decode over the compacted XA sectors (stereo / frequency / bits
 * from the settings), D2H.  Rows are as wide as the largest frame the settings' frame rate and CD speed allow (mdec.c:768-775).
 *   frames            (optional) [max_frames] NV21 pictures back to back; a frame that does not decode leaves its picture as it was
 *   frame_info, decoded   [max_frames]
 *   pcm               (optional) room for pcm_capacity int16 (interleaved L,R when stereo); whole sectors are decoded as far as they fit,
 *                     the others count as dropped in the summary (all of them when pcm is NULL)
 *   xa_sector_status  (optional) PSXHIP_XA_STATUS_* per decoded XA sector
 * Returns the samples per channel written to pcm, or a value below 0. */
int psxhip_str_read_host(psxhip_str_reader_t *reader, const psxhip_str_settings_t *settings, const uint8_t *sectors, int n_sectors,
                         int64_t first_frame, int max_frames, uint8_t *frames, psxhip_str_frame_info_t *frame_info,
                         psxhip_mdec_decoded_t *decoded, int16_t *pcm, int64_t pcm_capacity, int32_t *xa_sector_status,
                         psxhip_str_summary_t *summary);
/* revision of the reader's kernels (profiles are keyed by it) */
const char *psxhip_str_demux_kernel_rev(void);

/* ---------------------------------------------------------------- STRSPU reader -- */

/* The way back for format 8: muxed STRSPU sectors in HBM -> the video rows as above, and the audio chunks de-interleaved into SPU unit
 * records in the order psxhip_adpcm_decode_chains_* reads.  The rules are "psxhip STRSPU demux v1" (restated in
 * tests/strspu_demux_ref.py), defined for arbitrary bytes: bad input gives status bits, never a fault.  Symbols are section 15's:
 * ch = settings->audio_channels (0, 1, 2), B = 126 / ch, L = 16 B, id = strspu_options & 0xFFFF, d = 0 with
 * PSXHIP_STRSPU_NO_LEADING_DUMMY else 1, loop = the PSXHIP_STRSPU_LOOP bit.
 *   video   exactly the reader's rules for format 9 (STRV) with settings->str_video_id.
 *   audio   with ch != 0 a sector is audio iff bytes 0, 1 are 60 01 and le16(2) == id; it is neither video nor other.  ch != 0 with
 *           str_video_id == -1 or == id, and any undefined strspu_options bit, are PSXHIP_EINVAL.  With ch == 0 no sector is audio.
 *   number  k = le32(8) - 1 in 64 bits; outside [0, audio_capacity) the sector is dropped: counted in n_dropped_audio, it touches
 *           nothing.  Of the sectors of one k the one at the lowest stream position is the owner.
 *   units   by the settings' ch, never the header's: the owner's block b of lane c (16 bytes at 0x20 + c L + 16 b) becomes record
 *           (k B + b) ch + c of d_units (16-byte records): the lane streams G_c of section 15, one chain per channel with
 *           unit_stride = ch.  Records of a chunk without an owner are left as they were. */
enum {
	PSXHIP_STRSPU_CHUNK_MISSING = 1,     /* no sector carries this number */
	PSXHIP_STRSPU_CHUNK_DUPLICATE = 2,   /* more than one sector carries this number */
	PSXHIP_STRSPU_CHUNK_MISMATCH = 4     /* the owner's header is not section 15's for these settings: le16(4) != 0, le16(6) != 1,
	                                        le32(0xC) != 2016, channels != ch, lane bytes != L, frequency != settings->audio_frequency
	                                        (when that is non-zero), first sample != (k == 0 ? 0 : 28 (k B - d)), flag bit 1 !=
	                                        (k == 0 && d), flag bit 2 != loop, or a flag bit above 2 */
};

typedef struct {
	int32_t first_sector;        /* the owner's position in the stream, or -1 */
	int32_t status;              /* PSXHIP_STRSPU_CHUNK_* bits; a chunk without an owner: {-1, MISSING, 0 ...} */
	int32_t channels;            /* the owner's fields: le16(0x10) */
	int32_t lane_bytes;          /* le16(0x12) */
	int32_t frequency;           /* le32(0x14) */
	int32_t first_sample;        /* le32(0x18) */
	int32_t flags;               /* le16(0x1C) */
	int32_t reserved;            /* 0 */
} psxhip_strspu_chunk_info_t;

typedef struct {
	int32_t n_chunks;            /* 1 + the highest owned k, or 0 */
	int32_t n_complete;          /* the k < n_chunks without MISSING */
	int32_t last_chunk;          /* the lowest owned k whose flag bit 0 (last audio chunk) is set, or -1 */
	int32_t reserved;
} psxhip_strspu_audio_summary_t;

/* psxhip_str_demux_device for format 8, on the same handle: the video arguments, their alignment and stride rules are that call's.
 *   d_units         per stream audio_capacity * 126 records of 16 bytes, 16-byte aligned, streams units_stream_stride bytes (a multiple
 *                   of 16) apart; may be NULL when audio_capacity is 0.  audio_capacity <= (2^31 - 1) / 126
 *   d_chunk_info    [n_streams][audio_capacity]; every k in [0, audio_capacity) is written
 *   d_summary       as psxhip_str_demux_device's: n_audio counts the audio sectors (dropped ones included), n_other does not
 *   d_audio_summary [n_streams]
 *   d_sector_table  (optional) audio sectors are {1, -1, k or -1 when dropped, flags & 1}; for a stream this library muxed, read with
 *                   first_frame 1, the table equals psxhip_str_plan_sectors' and every status is 0
 * Of the settings str_video_id, audio_channels, audio_frequency (0: not compared), strspu_options, video_width and video_height are
 * read.  Asynchronous on `stream`; nothing is read back. */
int psxhip_strspu_demux_device(psxhip_str_reader_t *reader, const psxhip_str_settings_t *settings, int n_streams,
                               const uint8_t *d_sectors, size_t in_stream_stride, int n_sectors, int64_t first_frame, int max_frames,
                               uint8_t *d_bs, size_t bs_stride, size_t bs_stream_stride, int32_t *d_bs_sizes,
                               psxhip_str_frame_info_t *d_frame_info, uint8_t *d_units, int audio_capacity, size_t units_stream_stride,
                               psxhip_strspu_chunk_info_t *d_chunk_info, psxhip_str_sector_t *d_sector_table,
                               psxhip_str_summary_t *d_summary, psxhip_strspu_audio_summary_t *d_audio_summary, void *stream);

/* The de-interleave on its own: the inverse of psxhip_strspu_audio_sectors_device, and what an SPUI / VAGI body needs.  Chunk k of
 * stream i lies at d_in + i * in_stream_stride + (d_src_chunk ? d_src_chunk[k] : k) * chunk_stride; a negative table entry skips the
 * chunk (its records are left as they were).  Block b of lane c (16 bytes at lane_offset + c * lane_bytes + 16 b of the chunk) becomes
 * record (k B + b) * channels + c of d_units + i * units_stream_stride, B = lane_bytes / 16.  lane_bytes is a positive multiple of
 * 16, channels >= 1, lane_offset + channels * lane_bytes <= chunk_stride; d_in, lane_offset and the strides are 4-byte aligned,
 * d_units and units_stream_stride 16-byte aligned; n_chunks * channels * B fits an int.  An SPUI file from
 * psxhip_spu_file_encode_host is chunk_stride = align(channels * interleave, alignment), lane_offset = 0, lane_bytes = interleave; a
 * VAGI file the same with d_in behind its header.  Asynchronous on `stream`. */
int psxhip_spu_deinterleave_device(int device, const uint8_t *d_in, int n_chunks, size_t chunk_stride, size_t lane_offset,
                                   size_t lane_bytes, int channels, const int32_t *d_src_chunk, int n_streams, size_t in_stream_stride,
                                   uint8_t *d_units, size_t units_stream_stride, void *stream);

/* The whole STRSPU reader for one stream in host memory, built like psxhip_str_read_host: H2D, demux, one read-back of the summaries,
 * the BS decoder over the rows, psxhip_adpcm_decode_chains_chunked over the units (5 filters, 4-bit codes, zero states), D2H.
 * Channel c is one chain: unit_base = d ch + c, unit_stride = ch, n_units = nK B - d with nK = min(n_chunks, the chunks pcm_capacity
 * holds, n_sectors), pitch = ch, sample_offset = c.  The units are zeroed first: a missing chunk decodes as silence; the trap block
 * decodes to 28 zeros, as it lies.
 *   frames, frame_info, decoded   as psxhip_str_read_host's
 *   pcm             (optional) room for pcm_capacity int16 (interleaved L,R when stereo): it holds the largest nK with
 *                   28 (nK B - d) ch <= pcm_capacity; NULL: no audio is taken apart, every audio sector counts as dropped
 *   chunk_info      (optional) [min(n_sectors, the chunks pcm_capacity holds)]
 *   audio_summary   (optional)
 * Returns the samples per channel written to pcm, 28 (nK B - d) or 0, or a value below 0. */
int psxhip_strspu_read_host(psxhip_str_reader_t *reader, const psxhip_str_settings_t *settings, const uint8_t *sectors, int n_sectors,
                            int64_t first_frame, int max_frames, uint8_t *frames, psxhip_str_frame_info_t *frame_info,
                            psxhip_mdec_decoded_t *decoded, int16_t *pcm, int64_t pcm_capacity,
                            psxhip_strspu_chunk_info_t *chunk_info, psxhip_str_summary_t *summary,
                            psxhip_strspu_audio_summary_t *audio_summary);
/* revision of the STRSPU reader's kernels (profiles are keyed by it) */
const char *psxhip_strspu_demux_kernel_rev(void);

/* ---------------------------------------------------------------- disc finisher -- */

/* The step between "encoded in HBM" and "bytes a drive can read": sectors as the encoders leave them (dummy ECC, file-relative
 * timecode, the .str EDC where the reference's muxer puts it, one track per buffer) -> interleaved raw 2352-byte Mode 2 sectors with
 * sync, absolute BCD header, both subheader copies, EDC and, for form 1, P and Q parity (ECMA-130 / the Yellow Book).  The rules are
 * "psxhip disc finish v1" and "psxhip disc check v1" (restated in tests/disc_ref.py).
 *
 * Sources: up to PSXHIP_DISC_MAX_SOURCES runs of n_sectors sectors of sector_size 2352, 2336 or 2048 bytes, sector i at sectors +
 * i * stride (both 4-byte aligned, stride >= sector_size).  file_number (-1 .. 255) / channel_number (-1 .. 31) override the
 * subheader's file byte and the low 5 bits of its channel byte (the top 3 bits stay); -1 keeps the source's.  A 2048-byte source has
 * no subheader of its own: data_subheader is it (and must not have the form-2 bit 0x20 in byte 2).
 *
 * Schedule: period P (1 .. 64) and slot_source[P], an entry a source index or -1 (a gap).  Source s owns count_s slots.  Output sector
 * j falls in slot q = j % P; with s = slot_source[q] and r the rank of q among s's slots it is s's sector (j / P) * count_s + r.  A gap,
 * or a number >= n_sectors, gives the null sector: form 2, subheader 00 00 20 00, data zero, EDC like any other.
 *
 * Output sector j, at lba = start_lba + j (j counts from the start of the schedule, not of the call):
 *   0x000  sync 00 FF x 10 00
 *   0x00C  BCD minute, second, frame of lba + 150 (cdrom.c:62-65), then mode 02
 *   0x010  subheader, twice: source bytes 0x10..0x13 (2352) / 0..3 (2336) / data_subheader (2048), with the overrides
 *   form = bit 0x20 of the subheader's submode byte after the overrides; nothing else in the source decides it
 *   form 2: 0x018 data 0x18..0x92B from the source; 0x92C EDC of 0x10..0x92B
 *   form 1: 0x018 data 0x18..0x817 from the source (nothing past it is read); 0x818 EDC of 0x10..0x817; 0x81C P parity (172
 *           bytes); 0x8C8 Q parity (104 bytes)
 * EDC: polynomial 0xD8018001, zero init, no final xor, little-endian (cdrom.c:28-41).
 * ECC: GF(2^8), polynomial 0x11D, alpha = 2.  d[0..2063] = sector bytes 0xC..0x81B with d[0..3] (the header) taken as zero (the
 * Mode 2 rule), d[2064..2235] = the P bytes.
 *   P, m = 0..85:  c_i = d[m + 86 i], i = 0..23, c_24 = P[m], c_25 = P[86 + m]; n = 26
 *   Q, m = 0..51:  c_i = d[((m >> 1) * 86 + (m & 1) + 88 i) mod 2236], i = 0..42, c_43 = Q[m], c_44 = Q[52 + m]; n = 45
 * The parity is the pair with sum c_i = 0 and sum alpha^(n-1-i) c_i = 0: over the data symbols A = sum c_i, B = sum alpha^(n-1-i) c_i,
 * the first parity byte is (A ^ B) / 3 and the second is that ^ A. */
#define PSXHIP_DISC_MAX_SOURCES 64
#define PSXHIP_DISC_MAX_PERIOD 64
#define PSXHIP_DISC_LBA_LIMIT 450000     /* lba + 150 stays below it: the minute is two BCD digits */

typedef struct {
	const uint8_t *sectors;      /* device memory (psxhip_disc_finish_device) or host memory (psxhip_disc_finish_host); not read by psxhip_disc_plan */
	int64_t stride;              /* bytes from one sector to the next */
	int32_t n_sectors;
	int32_t sector_size;         /* 2352, 2336 or 2048 */
	int32_t file_number;         /* -1: keep the source's byte */
	int32_t channel_number;      /* -1: keep the source's byte */
	uint8_t data_subheader[4];   /* 2048-byte sources only */
	int32_t reserved;
} psxhip_disc_source_t;

typedef struct {
	int32_t period;              /* 1 .. PSXHIP_DISC_MAX_PERIOD */
	int32_t start_lba;           /* lba of output sector 0 of the schedule (not read by psxhip_disc_plan) */
	int32_t slot_source[PSXHIP_DISC_MAX_PERIOD];   /* [period]: a source index, or -1 for a gap */
} psxhip_disc_layout_t;

/* Sectors of the whole schedule: period * max over the sources of ceil(n_sectors / count); 0 without sectors.  Host-only (no device
 * is touched).  PSXHIP_EINVAL for a layout or a source outside the rules above, or when a source with sectors owns no slot. */
int64_t psxhip_disc_plan(const psxhip_disc_layout_t *layout, const psxhip_disc_source_t *sources, int n_sources);

/* Sectors first_out .. first_out + n_out - 1 of the schedule -> d_out (n_out x 2352 bytes, 4-byte aligned, overlapping no source), so
 * a large image can be made in pieces.  Refused (PSXHIP_EINVAL, before any device call) for arguments outside the rules above,
 * start_lba < 0, or a last sector with lba + 150 >= PSXHIP_DISC_LBA_LIMIT.  Asynchronous on `stream`; nothing is read back. */
int psxhip_disc_finish_device(int device, const psxhip_disc_layout_t *layout, const psxhip_disc_source_t *sources, int n_sources,
                              uint8_t *d_out, int64_t first_out, int64_t n_out, void *stream);

/* The inverse statement, defined for arbitrary bytes: per 2352-byte sector status bits, never a fault, no correction. */
enum {
	PSXHIP_DISC_SYNC = 1,          /* bytes 0..11 are not the sync */
	PSXHIP_DISC_HEADER = 2,        /* mode is not 2, or the MSF is not the BCD of lba + 150 (lba = start_lba + the sector's index);
	                                  with start_lba == -1: mode is not 2, or a nibble of the MSF is above 9 */
	PSXHIP_DISC_SUBHEADER = 4,     /* the two subheader copies differ */
	PSXHIP_DISC_EDC = 8,           /* the stored word differs from the computed one; the form is bit 0x20 of byte 0x12 */
	PSXHIP_DISC_ECC_P = 16,        /* form 1 only: a P codeword has a non-zero syndrome, the header taken as zero */
	PSXHIP_DISC_ECC_Q = 32,        /* form 1 only: ... a Q codeword */
	PSXHIP_DISC_EDC_ABSENT = 64    /* form 2 and the stored word is 0; set instead of PSXHIP_DISC_EDC */
};
typedef struct {
	int32_t n_sectors, n_form1, n_form2;
	int32_t n_bad;               /* sectors with any bit set */
	int32_t n_sync, n_header, n_subheader, n_edc, n_ecc_p, n_ecc_q, n_edc_absent;   /* sectors per bit */
	int32_t reserved;
} psxhip_disc_summary_t;
/* d_status (optional) [n_sectors] gets the bits; *d_summary (device memory) is overwritten.  start_lba >= -1, and with start_lba >= 0
 * the last lba + 150 < PSXHIP_DISC_LBA_LIMIT.  Pointers 4-byte aligned; asynchronous on `stream`. */
int psxhip_disc_check_device(int device, const uint8_t *d_image, int64_t n_sectors, int64_t start_lba, int32_t *d_status,
                             psxhip_disc_summary_t *d_summary, void *stream);

/* psxhip_disc_finish_device for sources and an image in host memory: H2D of the sources, finish, D2H; returns when `out` is written. */
int psxhip_disc_finish_host(int device, const psxhip_disc_layout_t *layout, const psxhip_disc_source_t *sources, int n_sources,
                            uint8_t *out, int64_t first_out, int64_t n_out);
/* revision of the finisher's kernels (profiles are keyed by it) */
const char *psxhip_disc_kernel_rev(void);

/* ---------------------------------------------------------------- disc reader -- */

/* The inverse of the finisher: a raw image of 2352-byte sectors in HBM -> damaged form-1 sectors repaired from their P / Q parity,
 * every sector routed to a track by file number, channel number and submode, every track's sectors compacted in image order in the
 * sector size psxhip_str_demux_device (2352 / 2336 / 2048) and psxhip_xa_disassemble_device (2352) read.  The rules are "psxhip disc
 * read v1" (restated in tests/disc_read_ref.py); they are defined for arbitrary bytes: every index that comes
 * from the image is bounded before use, bad input gives status bits, never a fault.
 *
 * Repair (notation of the finisher's section; S0 = sum c_i, S1 = sum alpha^(n-1-i) c_i over a codeword, parity included; bytes
 * 0..15 are never altered).  A sector is a form-1 candidate unless bit 0x20 is set in BOTH byte 0x12 and byte 0x16.  On a copy of a
 * candidate, rounds of a P pass then a Q pass: a codeword with S0 != 0 and S1 != 0 has e = (log S1 - log S0) mod 255; when e < n the
 * wrong symbol is i = n - 1 - e and, unless it is a header byte, S0 is xored into it (one correction); every other codeword stays.
 * Rounds repeat until one makes no correction or four have run.  Then the copy is judged as form 1 by check v1: EDC, P and Q all
 * right -> the sector is form 1 and the copy is its content (repaired when it differs from the input, else clean).  Otherwise the
 * sector's bytes are the input's, its form is bit 0x20 of byte 0x12, and a form-1 one is unrepairable.  Form 2 sectors are never
 * altered; their status is PSXHIP_DISC_READ_EDC or _EDC_ABSENT by check v1's rule.
 *
 * Routing, on bytes 0x10..0x13 after the repair: (submode & 0x0E) == 0 -> empty, no track.  Else the first track t in list order with
 * (file_number < 0 || byte 0x10 == file_number) && (channel_number < 0 || (byte 0x11 & 0x1F) == channel_number) &&
 * (submode & submode_mask) == submode_value; none -> unclaimed.
 *
 * Writing: the track's k-th sector in image order goes to sectors + k * stride when k < capacity, else it is dropped and touches
 * nothing.  sector_size 2352: the whole sector; 2336: bytes 0x10..0x92F; 2048: bytes 0x18..0x817 (a form-2 sector too, which gets
 * PSXHIP_DISC_READ_FORM).  Bytes between sector_size and stride are never touched. */
typedef struct {
	uint8_t *sectors;            /* device memory (psxhip_disc_read_device) or host memory (psxhip_disc_read_host); may be NULL when capacity is 0 */
	int64_t stride;              /* bytes from one slot to the next: a multiple of 4, >= sector_size */
	int32_t capacity;            /* slots */
	int32_t sector_size;         /* 2352, 2336 or 2048 */
	int32_t file_number;         /* -1: any, else 0 .. 255 */
	int32_t channel_number;      /* -1: any, else 0 .. 31 */
	uint8_t submode_mask;
	uint8_t submode_value;       /* bits outside the mask never match */
	uint8_t reserved[6];
} psxhip_disc_track_t;

enum {
	PSXHIP_DISC_READ_REPAIRED = 1,       /* form 1, made right by `corrections` symbol corrections */
	PSXHIP_DISC_READ_UNREPAIRABLE = 2,   /* form 1 by byte 0x12 and EDC, P or Q still wrong: the bytes are the input's */
	PSXHIP_DISC_READ_EDC = 4,            /* form 2: the stored EDC differs from the computed one */
	PSXHIP_DISC_READ_EDC_ABSENT = 8,     /* form 2: the stored EDC is 0; set instead of PSXHIP_DISC_READ_EDC */
	PSXHIP_DISC_READ_SYNC = 16,          /* bytes 0..11 are not the sync */
	PSXHIP_DISC_READ_SUBHEADER = 32,     /* the two subheader copies differ after the repair */
	PSXHIP_DISC_READ_EMPTY = 64,         /* no video, audio or data bit in the submode: no track */
	PSXHIP_DISC_READ_UNCLAIMED = 128,    /* no track matches */
	PSXHIP_DISC_READ_DROPPED = 256,      /* ordinal >= the track's capacity: nothing written */
	PSXHIP_DISC_READ_FORM = 512          /* a form-2 sector in a 2048-byte track */
};
typedef struct {
	int32_t track;               /* index into the track list, or -1 (empty, unclaimed) */
	int32_t ordinal;             /* sectors of that track before this one in the image (dropped ones too), or -1 */
	int32_t status;              /* PSXHIP_DISC_READ_* */
	int32_t corrections;         /* symbols corrected; 0 unless PSXHIP_DISC_READ_REPAIRED */
} psxhip_disc_read_sector_t;
typedef struct {
	int32_t n_sectors, n_form1, n_form2;
	int32_t n_clean, n_repaired, n_unrepairable;     /* form 1 = their sum */
	int32_t n_edc, n_edc_absent;                     /* form 2 */
	int32_t n_sync, n_subheader, n_empty, n_unclaimed, n_dropped;
	int32_t reserved;
	int64_t n_corrections;
} psxhip_disc_read_summary_t;

typedef struct psxhip_disc_reader psxhip_disc_reader_t;
/* The handle owns the workspace (16 bytes per sector and 256 per 1024 sectors, grown on demand); calls on one handle are ordered by
 * the streams they are given: the workspace is reused, so two calls on one handle run on one stream or are ordered by the caller. */
int psxhip_disc_reader_create(psxhip_disc_reader_t **reader, int device);
void psxhip_disc_reader_destroy(psxhip_disc_reader_t *reader);

/* d_image: n_sectors x 2352 bytes.  d_sector_table (optional) [n_sectors], d_track_counts [n_tracks] (every track's sectors, dropped
 * ones included; may be NULL when n_tracks is 0) and *d_summary are overwritten; all device memory.  Refused (PSXHIP_EINVAL, before
 * any device call): a pointer or stride not 4-byte aligned, d_summary not 8-byte aligned (it holds a 64-bit counter the kernels add to
 * atomically), stride < sector_size, a sector size other than the three, file or channel
 * number out of range, capacity < 0, a track with capacity > 0 and no buffer, more than PSXHIP_DISC_MAX_SOURCES tracks, n_sectors < 0
 * or >= 2^31, a track buffer that overlaps the image or another track's.  Asynchronous on `stream`; nothing is read back;
 * n_sectors == 0 is fine. */
int psxhip_disc_read_device(psxhip_disc_reader_t *reader, const uint8_t *d_image, int64_t n_sectors, const psxhip_disc_track_t *tracks,
                            int n_tracks, psxhip_disc_read_sector_t *d_sector_table, int32_t *d_track_counts,
                            psxhip_disc_read_summary_t *d_summary, void *stream);
/* psxhip_disc_read_device for an image, track buffers and results in host memory (no alignment rule for those pointers): H2D of the
 * image, read, D2H of what was written (slots past a track's count, and bytes between sector_size and stride, stay as they were);
 * returns when the tracks are written. */
int psxhip_disc_read_host(psxhip_disc_reader_t *reader, const uint8_t *image, int64_t n_sectors, const psxhip_disc_track_t *tracks,
                          int n_tracks, psxhip_disc_read_sector_t *sector_table, int32_t *track_counts,
                          psxhip_disc_read_summary_t *summary);
/* revision of the reader's kernels (profiles are keyed by it) */
const char *psxhip_disc_read_kernel_rev(void);

/* ---------------------------------------------------------------- SPU / VAG / SPUI / VAGI files ---- */

/* The reference's encode_file_spu / encode_file_spui (psxavenc/filefmt.c:212-389, .vag header :95-162) for PCM that is
 * all there up front: all channels' blocks come from one batched GPU call, the host places them -- leading dummy
 * block, loop flags, trailing trap block, alignment padding, big-endian .vag header.  Fields mirror args_t. */
typedef struct {
	int32_t format;             /* format_t: 2 = SPU, 3 = VAG (mono), 4 = SPUI, 5 = VAGI (interleaved channels) */
	int32_t audio_frequency;    /* default 44100 */
	int32_t audio_channels;     /* SPU / VAG: 1 */
	int32_t audio_interleave;   /* SPUI / VAGI: bytes per channel per chunk, multiple of 16 (default 2048) */
	int32_t alignment;          /* default 64 (SPU / VAG), 2048 (SPUI / VAGI) */
	int32_t audio_loop_point;   /* milliseconds, < 0 = none */
	int32_t enable_loop;        /* FLAG_SPU_ENABLE_LOOP */
	int32_t no_leading_dummy;   /* FLAG_SPU_NO_LEADING_DUMMY */
	char name[16];              /* .vag name field: the output file's base name (filefmt.c:150-161) */
} psxhip_spu_file_settings_t;

/* bytes the file takes for samples_per_channel samples, or < 0 */
int64_t psxhip_spu_file_size(const psxhip_spu_file_settings_t *settings, int64_t samples_per_channel);
/* pcm: int16, channels interleaved.  Returns the bytes written (= psxhip_spu_file_size) or < 0. */
int64_t psxhip_spu_file_encode_host(int device, const psxhip_spu_file_settings_t *settings, const int16_t *pcm,
                                    int64_t samples_per_channel, uint8_t *out, size_t out_size);

/* ---------------------------------------------------------------- SPU / VAG sound banks ---- */

/* "psxhip SPU bank v1" (DESIGN.md section 23): many mono SPU / VAG files -- the samples of a sound bank, each with its own length,
 * rate, loop point and name -- encoded by one call into one device buffer, and the way back.  Every entry is one serial ADPCM chain
 * from a zero state; its blocks are written straight to their place in the bank (a 4-bit unit record is an SPU block), a second
 * kernel writes everything that is not a data block.  File i lies at offsets[i] and equals, byte for byte, what
 * psxhip_spu_file_encode_host writes for {format, the entry's audio_frequency, 1 channel, alignment, the entry's audio_loop_point
 * and enable_loop, no_leading_dummy, the entry's name}; the bytes between the files, and behind the last up to total, are zero. */
typedef struct {
	int32_t format;            /* FORMAT_SPU (2) or FORMAT_VAG (3); 4 and 5 are PSXHIP_EINVAL in this revision */
	int32_t alignment;         /* per file (filefmt.c:280-285); a positive multiple of 16 here */
	int32_t no_leading_dummy;  /* FLAG_SPU_NO_LEADING_DUMMY */
	int32_t bank_alignment;    /* every file starts at a multiple of it; a multiple of 16, 16 .. 65536 */
	int32_t beam;              /* 0 or 1: the reference's bytes; 2 .. 4: "psxhip ADPCM beam v1" */
} psxhip_spu_bank_settings_t;

typedef struct {
	int64_t pcm_offset;        /* element offset of the entry's first sample in the PCM buffer (int16, mono); >= 0 */
	int64_t samples;           /* 0 .. 0x7FFFFFFF - 28 */
	int32_t audio_frequency;   /* > 0; goes into the .vag header and into the loop-point arithmetic */
	int32_t audio_loop_point;  /* milliseconds, < 0 = none */
	int32_t enable_loop;       /* FLAG_SPU_ENABLE_LOOP */
	char name[16];             /* .vag name field */
} psxhip_spu_bank_entry_t;

/* The layout alone; runs without a device.  sizes[i] = psxhip_spu_file_size of entry i's one-file settings; offsets[i] ascend in
 * entry order, each the end of the file before rounded up to bank_alignment (offsets[0] = 0); *total = the last file's end rounded
 * up likewise.  offsets, sizes ([n]) and total may each be NULL.  PSXHIP_EINVAL, each with its own text and in this order: n outside
 * 1 .. 65535; NULL settings or entries; a format other than 2 / 3; an alignment that is no positive multiple of 16; a bank_alignment that is no multiple of 16
 * in 16 .. 65536; a beam outside 0 .. 4; then per entry: samples out of range, audio_frequency <= 0, pcm_offset < 0; at last a bank
 * of 2^31 or more 16-byte records (record indices are int32). */
int psxhip_spu_bank_plan(const psxhip_spu_bank_settings_t *settings, const psxhip_spu_bank_entry_t *entries, int n,
                         int64_t *offsets, int64_t *sizes, int64_t *total);

/* The context owns the plan and its device tables: the chains and unit bases (entry i's chain reads its PCM and writes -- or, for
 * the decoder, reads -- the records from its first data block on), the zeroed states, the per-entry rows and the tile table the
 * kernels read, the decoder's tails.  The refusals of psxhip_spu_bank_plan; PSXHIP_EDEVICE without a GPU.  The calls of one context
 * share its states and tails: one call of a context at a time (order them on one stream, or wait in between). */
typedef struct psxhip_spu_bank psxhip_spu_bank_t;
int psxhip_spu_bank_create(psxhip_spu_bank_t **bank, int device, const psxhip_spu_bank_settings_t *settings,
                           const psxhip_spu_bank_entry_t *entries, int n);
void psxhip_spu_bank_destroy(psxhip_spu_bank_t *bank);
int64_t psxhip_spu_bank_total_bytes(const psxhip_spu_bank_t *bank);
/* offsets, sizes: [n] each, either may be NULL */
int psxhip_spu_bank_layout(const psxhip_spu_bank_t *bank, int64_t *offsets, int64_t *sizes);

/* d_pcm: int16 device memory holding every entry's samples at its pcm_offset; d_out: total bytes, 16-byte aligned.  Afterwards every
 * byte of [0, total) is defined as above and nothing outside is touched.  Every call starts every entry from a zero state.  With
 * beam >= 2 the data blocks are those of psxhip_spu_encode_streams_host_beam from a zero state, under the same framing.
 * Asynchronous on `stream` ONLY when the serial chains kernel is chosen: when the longest entry has psxhip's chunked threshold of
 * units or more (512 with up to 8 entries, else 4096) the entries are encoded by psxhip_adpcm_encode_chains_chunked, in place, and
 * that call synchronises with `stream`; the framing kernel behind it is asynchronous again. */
int psxhip_spu_bank_encode_device(psxhip_spu_bank_t *bank, const int16_t *d_pcm, uint8_t *d_out, void *stream);
/* pcm and out in host memory: pcm_elements >= every entry's pcm_offset + samples, out_size >= total.  Returns total or < 0. */
int64_t psxhip_spu_bank_encode_host(psxhip_spu_bank_t *bank, const int16_t *pcm, int64_t pcm_elements, uint8_t *out, size_t out_size);

/* The inverse of the framing: d_status[i] (int32, [n], zeroed by the call on the stream) gets the bits below for entry i of the bank
 * at d_bank (16-byte aligned); a bank this library wrote gives zeros.  The data blocks' other bytes are not judged (the decoder's unit
 * flags do that).  Asynchronous on `stream`. */
#define PSXHIP_SPU_BANK_STATUS_HEADER 1    /* one of the 48 header bytes is not what the entry implies */
#define PSXHIP_SPU_BANK_STATUS_DUMMY 2     /* the leading block is not zero */
#define PSXHIP_SPU_BANK_STATUS_FLAGS 4     /* byte 1 of a data block is not what the rule puts there */
#define PSXHIP_SPU_BANK_STATUS_TRAP 8      /* the trailing block differs */
#define PSXHIP_SPU_BANK_STATUS_PADDING 16  /* a non-zero byte in the file's padding or in the gap behind it */
int psxhip_spu_bank_check_device(psxhip_spu_bank_t *bank, const uint8_t *d_bank, int32_t *d_status, void *stream);

/* Every entry's data blocks back to PCM, written in the entries' own layout (pcm_offset, samples; nothing is stored past samples):
 * psxhip_adpcm_decode_chains_device from zero states under the context's chain table over the bank in place.  With d_ref_pcm (the
 * same layout) and d_entry_sums (uint64 [n][2], 8-byte aligned) given, d_entry_sums[i] = {sum (a - b)^2, sum b^2} as
 * psxhip_adpcm_sse_device defines them with the decode call's tail: over whole blocks, the reference PCM read as zero past samples.
 * d_ref_pcm and d_entry_sums come together or not at all.  Asynchronous on `stream`. */
int psxhip_spu_bank_decode_device(psxhip_spu_bank_t *bank, const uint8_t *d_bank, int16_t *d_pcm_out, const int16_t *d_ref_pcm,
                                  uint64_t *d_entry_sums, void *stream);
/* revision of spu_bank_kernels.hip */
const char *psxhip_spu_bank_kernel_rev(void);

/* "psxhip SPU loop seam v1" (DESIGN.md section 24).  A looped sample plays intro, body, body, ...: on every repeat the SPU enters the
 * loop-start block with the decoder state the END of the body left, while the encoder planned that block from the state the intro
 * left.  An entry's seam block S is the data block that carries LOOP_START when enable_loop is set and the entry has data blocks; 0
 * when enable_loop is set, no data block carries LOOP_START and no_leading_dummy is set (key-on sets the repeat address to the start
 * address); none (-1) otherwise.  The body is the data blocks S .. D-1, the intro 0 .. S-1.
 *
 * PSXHIP_SPU_SEAM_STEADY: the intro is encoded as always, its end state is s_0 ((0, 0) when S = 0); pass k = 0 .. P-1
 * (P = PSXHIP_SPU_SEAM_PASSES) encodes the body from s_k with the bank's encoder (plain or beam) and ends in e_k; e_k == s_k keeps
 * pass k's blocks (the entry is "fixed at pass k": a repeat enters the body in the state the encoder assumed), else s_{k+1} = e_k;
 * without a fixed point below P, pass 0's blocks -- the blocks of mode OFF -- are kept and the entry reports P.  Entries without a
 * seam block and everything that is not a data block are byte for byte those of mode OFF.  All launches go to the caller's stream,
 * nothing is read back, the host never waits.  In this revision a bank in mode STEADY always takes the serial chain kernels, however
 * long its entries: the chunked route builds host tables and synchronises. */
#define PSXHIP_SPU_SEAM_OFF 0       /* the default: exactly the launches of psxhip_spu_bank_encode_device as described above */
#define PSXHIP_SPU_SEAM_STEADY 1
#define PSXHIP_SPU_SEAM_PASSES 8
/* Sets the mode of the encodes that follow (and uploads the seam tables the first time STEADY is asked for: the call waits for the
 * device).  Another mode is PSXHIP_EINVAL.  One call of a context at a time, as above. */
int psxhip_spu_bank_set_seam(psxhip_spu_bank_t *bank, int mode);
/* The last encode's outcome per entry into d_pass (int32 [n], 4-byte aligned): -1 = no seam block, k = fixed at pass k, P = no fixed
 * point (pass 0 kept).  PSXHIP_EINVAL while the mode is OFF.  Asynchronous on `stream`. */
int psxhip_spu_bank_seam_passes_device(psxhip_spu_bank_t *bank, int32_t *d_pass, void *stream);

/* The seam report, defined on a bank's bytes alone (whoever wrote them).  Pass 1 decodes the data blocks 0 .. D-1 from (0, 0), whole
 * units as the SPU decodes them: y1, end state b.  Pass 2 decodes S .. D-1 from b: y2, end state b2. */
typedef struct {
	int32_t seam_block;     /* S, or -1: no seam block, and every other field is 0 */
	int32_t first_units;    /* the smallest k with both passes in the same state in front of unit S + k (from there they are identical); D - S if never */
	int32_t first_peak;     /* max |y2 - y1| */
	int32_t settled;        /* 1: b2 == b, every later repeat equals pass 2 */
	uint64_t first_sse;     /* sum (y2 - y1)^2 */
	uint64_t pass1_err;     /* sum (y1 - x)^2 over the body's whole units, the PCM x read as zero past `samples`; 0 without d_ref_pcm */
	uint64_t pass2_err;     /* sum (y2 - x)^2 likewise */
} psxhip_spu_seam_t;
/* d_bank: the bank, 16-byte aligned; d_ref_pcm: the entries' PCM in their own layout, or NULL; d_seam: [n], 8-byte aligned.  Works
 * in either mode.  Asynchronous on `stream`. */
int psxhip_spu_bank_seam_device(psxhip_spu_bank_t *bank, const uint8_t *d_bank, const int16_t *d_ref_pcm, psxhip_spu_seam_t *d_seam,
                                void *stream);
/* revision of spu_seam_kernels.hip */
const char *psxhip_spu_seam_kernel_rev(void);

/* ---------------------------------------------------------------- colour conversion + scaling front-end ---- */

/* What the reference leaves to FFmpeg's libswscale (psxavenc/decoding.c:287-311: sws_getContext(... AV_PIX_FMT_NV21,
 * SWS_BICUBIC ...), destination colourspace ITU-R BT.601 full range; :463-475: sws_scale into the frame buffer): decoded
 * pictures of any size -> NV21 frames of the encoder's size, on the device, written where the MDEC kernel reads them.
 * libswscale is absent from the reference tree and from the build image, so this step's arithmetic is this library's own
 * ("psxhip front-end v1": bicubic B = 0 / C = 0.6 like SWS_BICUBIC, 14-bit taps, 15-bit intermediates; DESIGN.md section 9,
 * restated in oracle/frontend_oracle.c) -- PARITY WITH THE REFERENCE'S SCALER IS UNPINNED.  Everything downstream of the NV21
 * frames is unaffected. */
enum {
	PSXHIP_PIX_RGB24 = 0,      /* rows of 3 * width bytes, R G B */
	PSXHIP_PIX_YUV420P = 1     /* Y plane (w * h), U plane, V plane ((w/2) * (h/2) each); w, h even */
};
typedef struct psxhip_scaler psxhip_scaler_t;
/* src_full_range: YUV input only -- 0 = limited ("MPEG") range, expanded to the full range the encoder expects
 * (decoding.c:301-311 passes the stream's own range as the source range); RGB input is full range by definition.
 * dst_width / dst_height: multiples of 16 (mdec.c:601-602), at most 1024; shrinking by more than 16x is refused, in any of the
 * four filters (RGB chroma is filtered from full resolution to dst / 2: it shrinks twice as much as luma). */
int psxhip_scaler_create(psxhip_scaler_t **s, int device, int src_format, int src_width, int src_height, int src_full_range,
                         int dst_width, int dst_height);
void psxhip_scaler_destroy(psxhip_scaler_t *s);
size_t psxhip_scaler_source_bytes(const psxhip_scaler_t *s);      /* bytes of one source picture */
/* n_frames pictures at d_src + i * src_stride -> NV21 frames at d_frames + i * frame_stride (4-byte aligned); asynchronous
 * on `stream`.  d_frames / frame_stride are what psxhip_mdec_encode_frames_device takes. */
int psxhip_scaler_convert_device(psxhip_scaler_t *s, const uint8_t *d_src, size_t src_stride, int n_frames, uint8_t *d_frames,
                                 size_t frame_stride, void *stream);
/* host buffers (pictures and frames back to back): H2D, kernel, D2H, synchronise */
int psxhip_scaler_convert_host(psxhip_scaler_t *s, const uint8_t *src, int n_frames, uint8_t *frames);
/* the filter banks in use (which: 0 luma horizontal, 1 luma vertical, 2 chroma horizontal, 3 chroma vertical): returns
 * the number of output positions, *taps per position; fills left[n] / coef[n * taps] when both are given (cap elements) */
int psxhip_scaler_filter(const psxhip_scaler_t *s, int which, int *taps, int32_t *left, int16_t *coef, int cap);

/* ---------------------------------------------------------------- picture ingest: decoder formats -> the scaler's input ---- */

/* The step in front of the scaler: the pictures a video decoder produces -- planar, semi-planar or packed, 8 or 10 bits, padded
 * rows, any of five colour matrices in limited or full range -- to one of the scaler's two inputs, tightly packed at the source's
 * size, on the device.  The reference hands libswscale the decoder's pix_fmt and the stream's matrix and range
 * (psxavenc/decoding.c:287-311); the arithmetic here is this library's own, in integers ("psxhip ingest v1", DESIGN.md section 19;
 * >> is arithmetic), and the kernel is held to it bit for bit -- PARITY WITH LIBSWSCALE IS UNPINNED, as for the scaler.
 *
 * A source picture is up to three planes, each at a byte offset inside the picture with a pitch in bytes (>= the row's bytes); planes
 * must not overlap.  Chroma planes of a subsampled axis have ceil(n / 2) samples.  16-bit formats are little-endian words and need
 * even offsets, pitches, source address and src_stride. */
enum {
	PSXHIP_SRC_YUV420P = 0,     /* planes Y, Cb, Cr */
	PSXHIP_SRC_YUV422P = 1,
	PSXHIP_SRC_YUV444P = 2,
	PSXHIP_SRC_NV12 = 3,        /* planes Y, CbCr pairs */
	PSXHIP_SRC_NV21 = 4,        /* planes Y, CrCb pairs */
	PSXHIP_SRC_YUYV422 = 5,     /* one plane, Y Cb Y Cr; even width */
	PSXHIP_SRC_UYVY422 = 6,     /* one plane, Cb Y Cr Y; even width */
	PSXHIP_SRC_YUV420P10 = 7,   /* 16-bit words, the value in the low 10 bits (higher bits are masked off) */
	PSXHIP_SRC_YUV422P10 = 8,
	PSXHIP_SRC_YUV444P10 = 9,
	PSXHIP_SRC_P010 = 10,       /* NV12 of 16-bit words, the value = word >> 6 */
	PSXHIP_SRC_GRAY8 = 11,
	PSXHIP_SRC_RGB24 = 12,      /* one plane, R G B */
	PSXHIP_SRC_BGR24 = 13,
	PSXHIP_SRC_RGBA32 = 14,     /* R G B A, alpha dropped */
	PSXHIP_SRC_BGRA32 = 15
};
/* the source's matrix (YUV and grey sources): Kr, Kb = 0.299, 0.114 (also BT.470BG, SMPTE170M) / 0.2126, 0.0722 / 0.212, 0.087 /
 * 0.30, 0.11 / 0.2627, 0.0593 (non-constant luminance) */
enum {
	PSXHIP_MATRIX_BT601 = 0,
	PSXHIP_MATRIX_BT709 = 1,
	PSXHIP_MATRIX_SMPTE240M = 2,
	PSXHIP_MATRIX_FCC = 3,
	PSXHIP_MATRIX_BT2020_NCL = 4
};
enum {
	PSXHIP_INGEST_CHROMA_BILINEAR = 1   /* RGB24 output: centre-sited mix of subsampled chroma instead of replication */
};
typedef struct {
	size_t offset;      /* of the plane's first byte inside a picture */
	size_t pitch;       /* bytes from a row to the next */
} psxhip_ingest_plane_t;
typedef struct psxhip_ingest psxhip_ingest_t;

/* Checks the source and computes the matrix; no device is touched before a conversion (`device` is the one conversions run on), so
 * the rules and psxhip_ingest_matrix hold on a machine without one.  planes[n_planes]: as many as the format has.  matrix and
 * full_range (0 = limited) apply to YUV and grey sources.  out_format:
 *   PSXHIP_PIX_RGB24    every source; width and height may be odd.  Subsampled chroma is replicated (x >> 1, y >> 1), or with
 *                       PSXHIP_INGEST_CHROMA_BILINEAR mixed as the display back-end mixes it, at the source's depth: 4:2:0
 *                       (9 near + 3 far_x + 3 far_y + far_xy + 8) >> 4, 4:2:2 (3 near + far + 2) >> 2, the far sample on the pixel's
 *                       own side, clamped to the plane.  Then, full range out,
 *                         c = clamp((cy (Y - yoff) + cu (Cb - coff) + cv (Cr - coff) + 32768) >> 16, 0, 255)
 *                       with (cu, cv) = (0, rv) for R, (gu, gv) for G, (bu, 0) for B: 16 fractional bits, each the round-half-up of
 *                       the exact rational (psxhip_ingest_matrix).  Grey: R = G = B from the luma term.  RGB sources: a byte shuffle.
 *   PSXHIP_PIX_YUV420P  YUV and grey sources whose matrix is BT.601, even width and height: samples are copied, 10-bit ones as
 *                       min(255, (v + 2) >> 2); 4:2:2 and 4:4:4 chroma is box-averaged to 4:2:0 with one rounding, depth reduction
 *                       included; grey gets chroma 128.  The range is not touched: hand full_range to psxhip_scaler_create.
 * PSXHIP_EINVAL, with the rule in psxhip_last_error(), for anything else. */
int psxhip_ingest_create(psxhip_ingest_t **g, int device, int src_format, int width, int height, const psxhip_ingest_plane_t *planes,
                         int n_planes, int matrix, int full_range, int out_format, uint32_t options);
void psxhip_ingest_destroy(psxhip_ingest_t *g);
/* bytes of one output picture (the scaler's psxhip_scaler_source_bytes), and from a source picture's first byte to the end of its
 * last plane (the least src_stride) */
size_t psxhip_ingest_output_bytes(const psxhip_ingest_t *g);
size_t psxhip_ingest_source_bytes(const psxhip_ingest_t *g);
/* out: cy, rv, gu, gv, bu, yoff, coff (all 0 for an RGB source) */
int psxhip_ingest_matrix(const psxhip_ingest_t *g, int32_t out[7]);
/* Output picture i (at d_out + i*out_stride, psxhip_ingest_output_bytes of it written, the rest up to out_stride kept) is made from
 * source picture d_src_index[i] (at d_src + that*src_stride); d_src_index NULL: from source picture i.  A repeated index reads the
 * same source again, an index that does not occur is never read, and a negative index (or one >= n_src) leaves that output picture
 * as it was.  Only the sources' sample bytes are read.  n_out = 0 touches nothing.  d_out must not overlap d_src.  Asynchronous
 * on `stream`; the call needs no temporary memory. */
int psxhip_ingest_convert_device(psxhip_ingest_t *g, const uint8_t *d_src, size_t src_stride, int n_src, const int32_t *d_src_index,
                                 int n_out, uint8_t *d_out, size_t out_stride, void *stream);
/* Same, host buffers (src_index too): H2D, kernel, D2H, synchronise. */
int psxhip_ingest_convert_host(psxhip_ingest_t *g, const uint8_t *src, size_t src_stride, int n_src, const int32_t *src_index,
                               int n_out, uint8_t *out, size_t out_stride);
/* revision of the ingest kernels (profiles are keyed by it) */
const char *psxhip_ingest_kernel_rev(void);

/* The planners: no device.
 * recommend: PSXHIP_PIX_YUV420P when psxhip_ingest_create would accept it for this source (the cheap path), else PSXHIP_PIX_RGB24;
 * PSXHIP_EINVAL for an unknown format. */
int psxhip_ingest_recommend(int src_format, int matrix, int width, int height);
/* decoding.c:275-285: the target size (max_w x max_h, multiples of 16 in 16 .. 1024) reduced to the source's aspect ratio, in the
 * reference's double-precision expressions: src_ratio < dst_ratio ? w = ((int)round(h * src_ratio) + 15) & ~15
 * : h = ((int)round(w / src_ratio) + 15) & ~15; unchanged with ignore_aspect (FLAG_BS_IGNORE_ASPECT).  PSXHIP_EINVAL when a side
 * comes out 0 or above its maximum. */
int psxhip_ingest_fit(int src_w, int src_h, int max_w, int max_h, int ignore_aspect, int *dst_w, int *dst_h);
/* decoding.c:412-461: decoded pictures with time stamps pts[n] (in tb_num / tb_den seconds) to frames at fps_num / fps_den.  With
 * p = (double)pts * tb_num / tb_den and step = fps_den / fps_num: a picture with p < next after the first kept one is dropped; the
 * first kept one sets next = p, later ones next += step; then max(0, (int)ceil((p - next) / step)) repeats of the last kept picture
 * come out, each with next += step, and then the picture itself.  Fills out_index (cap entries at most) with the picture of each
 * output frame -- what d_src_index takes -- and returns the number of output frames, also when cap is too small. */
int psxhip_ingest_pace(const int64_t *pts, int n, int tb_num, int tb_den, int fps_num, int fps_den, int32_t *out_index, int cap);

/* ---------------------------------------------------------------- audio front-end: resample + remix ---- */

/* What the reference leaves to FFmpeg's libswresample (psxavenc/decoding.c:215-254: swr_alloc_set_opts2 to S16 at the target
 * rate, mono or stereo; :370-406: swr_convert once per decoded packet): decoded PCM of any rate and layout -> interleaved int16
 * at the target rate and channel count, on the device, written where the ADPCM and STR kernels read their input.  The
 * arithmetic is this library's own ("psxhip audio front-end v1"): int16 conversion, a Q14 channel
 * matrix at the source rate, a Kaiser-windowed sinc polyphase filter with Q15 taps and libswresample's default parameters.
 * PARITY WITH libswresample IS UNPINNED.  A handle keeps the filter history: a stream cut into any number of calls gives the
 * same bytes as one call. */
enum { PSXHIP_PCM_S16 = 0, PSXHIP_PCM_S16P = 1, PSXHIP_PCM_S32 = 2, PSXHIP_PCM_S32P = 3, PSXHIP_PCM_F32 = 4, PSXHIP_PCM_F32P = 5 };
typedef struct psxhip_resampler psxhip_resampler_t;
/* pure host, no device needed: the table the rates imply (returns P, or < 0; *taps = T; fills coef[P*T] when cap allows).
 * Equal rates are a bypass: P = 1, T = 0. */
int psxhip_resampler_design(int src_rate, int dst_rate, int *phases, int *taps, int16_t *coef, int cap);
/* pure host: outputs per channel of a call adding n_in samples to a stream that has consumed `consumed` (not flushed); < 0 on
 * bad arguments */
int64_t psxhip_resampler_output_count(int src_rate, int dst_rate, int64_t consumed, int64_t n_in, int flush);
/* rates 1 000 .. 384 000 Hz, at most 16x either way; 1 .. 8 channels.  mix: dst_channels x src_channels, Q14, no row with
 * sum |m| > 65535; NULL = the default for N -> N, 2 -> 1, 1 -> 2 and 6 -> 2 (5.1), PSXHIP_EINVAL for any other shape */
int psxhip_resampler_create(psxhip_resampler_t **r, int device, int src_format, int src_channels, int src_rate,
                            int dst_channels, int dst_rate, const int16_t *mix /* dst x src, Q14; NULL = default */);
void psxhip_resampler_destroy(psxhip_resampler_t *r);
void psxhip_resampler_reset(psxhip_resampler_t *r);
/* src: 1 pointer (interleaved) or src_channels pointers (planar), device memory; d_dst: interleaved int16, room for
 * output_count(...) * dst_channels; asynchronous on `stream`; calls on one handle are stream-ordered.  After a flush, calls
 * return PSXHIP_EINVAL until psxhip_resampler_reset. */
int psxhip_resampler_convert_device(psxhip_resampler_t *r, const void *const *src, int64_t n_in, int16_t *d_dst,
                                    int64_t *n_out, int flush, void *stream);
/* host buffers: H2D, kernel, D2H, synchronise (psxavenc's per-packet swr_convert call site); dst_cap in samples per channel */
int psxhip_resampler_convert_host(psxhip_resampler_t *r, const void *const *src, int64_t n_in, int16_t *dst,
                                  int64_t dst_cap, int64_t *n_out, int flush);
const char *psxhip_resampler_kernel_rev(void);   /* "afe-k1.2": the key for profiles of this kernel */

/* ---------------------------------------------------------------- synthetic inputs --------- */

/* Integer-only generators (same function as oracle/synth.c) so benchmarks can fill HBM directly. */
int psxhip_synth_frames_device(int device, uint8_t *d_frames, size_t frame_stride, int width, int height,
                               uint32_t seed, uint32_t first_frame, int n_frames, int noise_amp, void *stream);
int psxhip_synth_pcm_device(int device, int16_t *d_pcm, uint32_t seed, uint32_t chain, int64_t first_sample,
                            int64_t n, int kind, int pitch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSXAV_HIP_H */
