// adpcm_plan.h -- what the ADPCM encoder's and decoder's host layer (psxhip_adpcm_encode.cpp, psxhip_adpcm_decode.cpp,
// psxhip_audio_api.cpp; asked by psxhip_str.cpp and psxhip_spu_bank.cpp too) derives from a call's arguments alone: what every entry
// point refuses, with which text and in which order; whether chains run serially or cut along time, and whether a host-buffer call
// takes the per-call fast path; the chunk length; the chunk tables and the carving of the encoder session's block and of the
// decoder's workspace; the shapes of the host-buffer calls.  Arithmetic and refusals only (no HIP), like reader_plan.h and
// str_plan.h: adpcm_plan.cpp builds with a host compiler alone and links against nothing but psxhip_set_error
// (tests/test_adpcm_plan_cpu.py does so, under the host sanitizers); the launch code only executes these plans.  A plan function
// returns PSXHIP_OK, or PSXHIP_EINVAL with the error text set.  Device pointers come as numbers: nothing here reads through one (the
// chain tables and EOF flags the builders read are the caller's host arrays).  Nothing here is part of the library's surface.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/psxav_hip.h"
#include "host_layout.h"

extern "C" void psxhip_set_error(const char* fmt, ...);          // (psxhip_api.cpp; psxhip_internal.h declares it beside HIP)

#pragma GCC visibility push(hidden)

// ---------------------------------------------------------------------------------------------- constants the plan shares with the launch code
constexpr int kAdpcmCallStageMax = 8192;        // PSXHIP_ADPCM_CALL_STAGE_MAX (psxhip_audio_api.cpp asserts that they agree)
constexpr int kAdpcmVerifyBatchMax = 16;        // kVerifyBatchMax of verify_passes.h (its two users assert that they agree)
// the per-call fast path's page-locked block (CallScratch of psxhip_audio_api.cpp): [samples in | blocks or sectors out | states]
constexpr size_t kAdpcmCallIn = 32 << 10, kAdpcmCallOut = 16 << 10, kAdpcmCallStates = 256;

// ---------------------------------------------------------------------------------------------- the coding rules, entry point by entry point
enum AdpcmChainsEntry { kEncodeChains, kBeamEncodeChains };
// psxhip_adpcm_encode_chains_device, psxhip_adpcm_beam_encode_chains_device (beam and d_unit_err are the latter's)
int adpcm_encode_chains_check(AdpcmChainsEntry who, uintptr_t d_samples, uintptr_t d_chains, uintptr_t d_unit_base, uintptr_t d_states,
                              uintptr_t d_units, int n_chains, int filter_count, int bits, int beam, uintptr_t d_unit_err);
// psxhip_adpcm_session_create, behind its handle pointer
int adpcm_session_create_check(uintptr_t d_samples, bool chains, bool unit_base, uintptr_t d_units, int n_chains, int filter_count, int bits,
                               int chunk_units, int warmup_units);
// psxhip_adpcm_session_set_beam: 0 .. 4, and only while the session holds no records
int adpcm_session_beam_check(bool session, int beam, bool speculated);
// psxhip_adpcm_encode_chains_chunked (beam_entry false) and its beam twin, in front of the session they create
int adpcm_encode_chunked_check(bool beam_entry, int beam, uintptr_t d_states);
// the beam widths the *_host_beam entry points take; `who` without "psxhip_"
int adpcm_host_beam_check(const char* who, int beam);
int spu_pack_check(uintptr_t d_units, int n_blocks, uintptr_t d_out);
int xa_assemble_check(uintptr_t d_units, uintptr_t d_out, int n_sectors, int n_streams, int format, int bits, size_t units_stream_stride,
                      size_t out_stream_stride);
// psxhip_adpcm_decode_chains_device (chunked false) and psxhip_adpcm_decode_chains_chunked
int adpcm_decode_chains_check(bool chunked, uintptr_t d_units, bool chains, bool unit_base, uintptr_t d_states, uintptr_t d_samples, uintptr_t d_tail,
                              int n_chains, int filter_count, int bits);
// ... and the latter's chain table: pitch >= 1, n_units >= 0; the units of all chains together
int adpcm_decode_chunked_chains_check(const psxhip_adpcm_chain_t* chains, int n_chains, long long* total_units);
int adpcm_sse_check(uintptr_t d_a, uintptr_t d_a_tail, uintptr_t d_b, uintptr_t d_chains, int n_chains, uintptr_t d_unit_sse, uintptr_t d_unit_base,
                    uintptr_t d_chain_sums);
int xa_disassemble_check(uintptr_t d_sectors, int n_sectors, int format, int bits, uintptr_t d_units, uintptr_t d_sector_status);

// ---------------------------------------------------------------------------------------------- route
// Units per chain from which chains are cut along time (speculate-and-verify) instead of run serially: 4096, and 512 when the call
// has only a few chains -- one chain of 788 blocks (config `spu`'s second of audio) encoded serially by one wavefront takes 1.35 ms,
// cut along time 0.98 ms; 2048 blocks 3.35 ms against 0.97 (the chunked path's set-up and verify round trips are ~0.75 ms whatever
// the length, so below ~500 units serial wins; NOTEBOOK section 4).  Many short chains keep the serial kernel: it runs them all
// side by side.
constexpr int adpcm_chunked_threshold(int n_chains) { return n_chains <= 8 ? 512 : 4096; }
// the one answer to "serial or chunked": the host entry points, the decoder's, psxhip_str_encode_device and the sound bank ask it
constexpr bool adpcm_route_chunked(int units_per_chain, int n_chains) { return units_per_chain >= adpcm_chunked_threshold(n_chains); }
// The per-call fast path (the reference's pattern: psx_audio_spu_encode once per 28 samples, psx_audio_xa_encode once per sector): one
// launch out of the page-locked block.  stage_max: int16 elements the call kernel stages (kAdpcmCallStageMax); out_max: bytes of the
// block's output part (kAdpcmCallOut).  SPU: a few short streams, every stream's row padded to whole units and to a multiple of 8
bool spu_call_fast_path(int beam, int n_streams, int n_units, size_t stage_max, size_t out_max);
// XA: one stream of up to six sectors; `per` its samples (all channels), `bytes` its sectors'
bool xa_call_fast_path(int beam, int n_streams, int sectors, size_t per, size_t bytes, size_t stage_max, size_t out_max);

// ---------------------------------------------------------------------------------------------- chunking
struct AdpcmChunking {
    int chunk_units, warmup_units;
};
// Chunk length: long enough that verify needs few passes (a wrong guess travels one chunk per pass, and tonal material does not
// fall into the same state within a thousand units), short enough that there are >= ~8 k chunks -- 1600+ wavefronts -- to fill 256
// CUs (tools/gpu_adpcm_sweep.py: 13 M units, tonal: chunks of 1024 are 14 % faster than 512; noise: within 3 %); warm-up 16 .. 64
// units.  Jobs that are large enough for it get the length at which every wavefront slot of the GPU (8 per SIMD) holds exactly ONE
// wavefront of `rows` chunks: the encoder is a dependent chain per unit, so a SIMD with four wavefronts runs its VALU at 84 % and one
// with eight at ~100 %, and a launch of 3.7 wavefronts per SIMD ends when the SIMDs that drew four do (config 5, 78 M units on one
// GPU: 1899 instead of 4096 units per chunk, 21.3 -> 24.4 M sectors/s, still two verify passes; 1266: three passes, 950: four --
// NOTEBOOK section 4).  psxavenc_amd/adpcm.py: pick_chunking is held to this function by tests/test_adpcm_plan_cpu.py.
AdpcmChunking adpcm_chunking(long long total_units, int rows, int n_cu);
// The decoder's: the rule above for wavefronts of 64 chunks, and no longer than a quarter of what fills the device once (a decode
// wavefront holds 64 chunks and a CU eight such wavefronts: at least four rounds of them) but for chunks of 256
int adpcm_decode_chunking(long long total_units, int n_cu);

// ---------------------------------------------------------------------------------------------- chunk tables and layouts
// The encoder session's tables and its block (psxhip_adpcm_chunk_job_t), every part 256-byte placed and in this order
struct AdpcmSessionPlan {
    std::vector<int64_t> state_base;                    // [n_chains] index into unit_states of each chain's unit 0
    std::vector<int32_t> chunk_chain, chunk_first;      // [n_chunks]
    std::vector<int32_t> lead;                          // [n_chains] lead_units, negatives as 0; zeros without lead_units
    int64_t total_units;
    int n_chunks;
    size_t o_chains, o_base, o_sbase, o_lead, o_cstates, o_final, o_known, o_flags, o_cchain, o_cfirst, o_used, o_ustates, bytes;
};
void adpcm_session_plan(const psxhip_adpcm_chain_t* chains, const int32_t* lead_units, int n_chains, int chunk_units, AdpcmSessionPlan* p);

// The chunked decode's tables and its workspace (psxhip_adpcm_decode_job_t): chain by chain, the two chains of an interleaved stereo
// pair chunk by chunk in turns; chunk_pred the chunk in front of a chunk in its chain (-1: none), last_chunk a chain's last (-1: none)
struct AdpcmDecodePlan {
    std::vector<int32_t> chunk_chain, chunk_first, chunk_pred, last_chunk;
    size_t n_chunks;
    size_t o_chains, o_base, o_cc, o_cf, o_cp, o_last, o_used, o_end, o_flags, bytes;
};
int adpcm_decode_plan(const psxhip_adpcm_chain_t* chains, int n_chains, int chunk_units, AdpcmDecodePlan* p);

// ---------------------------------------------------------------------------------------------- psxhip_spu_encode_streams_host*, psxhip_xa_encode_streams_host*
// One device buffer per size below; `row` is the fast path's staged row per stream instead.  With `empty` the call returns `bytes` at
// once, behind the argument check alone.
struct SpuEncodeShape {
    int n_units, bytes;                     // per stream; `bytes` is what the call returns
    bool empty;
    int64_t stream_stride, out_stride;      // the caller's, or a stream's own size when there is one stream
    size_t per;                             // the device row per stream (elements): samples x pitch
    size_t readable;                        // elements of a stream that are the caller's to read: (samples - 1) pitch + 1 (adpcm.c:65,110)
    size_t row;                             // pitch 1, zero-padded to whole units and to a multiple of 8
    size_t sample_bytes, chain_bytes, base_bytes, state_bytes, unit_bytes, out_bytes;
};
int spu_encode_shape(bool buffers, int n_streams, int64_t stream_stride, int pitch, int samples_per_stream, int64_t out_stride, SpuEncodeShape* p);

struct XaEncodeShape {
    XaLayout xa;
    int groups, sectors, bytes;             // per stream; `bytes` is what the call returns
    bool empty;
    int units_per_stream, units_per_chain;
    int64_t stream_stride, out_stride;
    size_t per;                             // a stream's samples, all channels together
    size_t row;                             // the fast path's: `per` up to a multiple of 8
    size_t n_chains;
    size_t sample_bytes, chain_bytes, base_bytes, state_bytes, unit_bytes, out_bytes, eof_bytes;
};
int xa_encode_shape(bool buffers, int format, int stereo, int bits, int n_streams, int64_t stream_stride, int samples_per_stream, int64_t out_stride,
                    XaEncodeShape* p);
// Which sector gets the EOF submode bit: eof_flags[k] != 0 when given (the reference's encode_file_str finalises EVERY audio sector
// once its decoder has seen the end of the input, filefmt.c:492-493), else a stream's last sector with `finalize`.
// One stream's first 32 sectors as bits (the fast path: nothing to upload) ...
uint32_t xa_encode_eof_bits(int sectors, const uint8_t* eof_flags, int finalize);
// ... and the table of all streams
std::vector<uint8_t> xa_encode_eof_table(int n_streams, int sectors, const uint8_t* eof_flags, int finalize);

// ---------------------------------------------------------------------------------------------- psxhip_spu_decode_streams_host, psxhip_xa_decode_streams_host
// (inline: tests/cpu/reader_plan_check.cpp prints these shapes and links nothing of adpcm_plan.cpp)
struct StreamsHostShape {
    int channels, units_per_stream;
    int per_channel;                    // samples a channel of a stream decodes to: what the call returns
    size_t per, in_bytes;               // a stream's samples (all channels) and source bytes
    int64_t in_stride, out_stride;      // the caller's, or a stream's own size when there is one stream
    size_t n_chains, total_sectors;
    size_t src_bytes, unit_bytes, state_bytes, sample_bytes, status_bytes;
};

static inline int streams_host_strides(const char* who, int n_streams, int64_t in_stride, int64_t out_stride, StreamsHostShape* p) {
    if (n_streams == 1) { in_stride = (int64_t)p->in_bytes; out_stride = (int64_t)p->per; }       // one stream: the strides are not looked at
    if (n_streams > 0 && (in_stride < (int64_t)p->in_bytes || out_stride < (int64_t)p->per)) {
        psxhip_set_error("%s: in_stride %lld < %zu bytes or out_stride %lld < %zu samples per stream", who, (long long)in_stride, p->in_bytes,
                         (long long)out_stride, p->per);
        return PSXHIP_EINVAL;
    }
    p->in_stride = in_stride;
    p->out_stride = out_stride;
    const size_t S = n_streams > 0 ? (size_t)n_streams : 0;
    p->n_chains = S * (size_t)p->channels;
    p->src_bytes = p->in_bytes * S;
    p->state_bytes = sizeof(psxhip_adpcm_state_t) * p->n_chains;
    p->sample_bytes = sizeof(int16_t) * p->per * S;
    return PSXHIP_OK;
}

static inline int spu_streams_host_shape(int n_streams, int64_t in_stride, int n_blocks, bool buffers, int64_t out_stride, StreamsHostShape* p) {
    if (n_streams < 0 || n_blocks < 0 || (n_streams > 0 && n_blocks > 0 && !buffers) || (int64_t)n_blocks * 28 > 0x7FFFFFFF) {
        psxhip_set_error("spu_decode_streams_host: bad argument");
        return PSXHIP_EINVAL;
    }
    *p = StreamsHostShape();
    p->channels = 1;
    p->units_per_stream = n_blocks;
    p->per_channel = n_blocks * 28;
    p->per = (size_t)p->per_channel;
    p->in_bytes = (size_t)n_blocks * 16;
    const int rc = streams_host_strides("spu_decode_streams_host", n_streams, in_stride, out_stride, p);
    p->unit_bytes = p->src_bytes;       // the source is the unit records
    return rc;
}

static inline int xa_streams_host_shape(int format, int stereo, int bits, int n_streams, int64_t in_stride, int n_sectors, bool buffers,
                                        int64_t out_stride, StreamsHostShape* p) {
    if (n_streams < 0 || n_sectors < 0 || (bits != 4 && bits != 8) || (format != 0 && format != 1) ||
        (n_streams > 0 && n_sectors > 0 && !buffers) || (int64_t)n_sectors * 4032 > 0x7FFFFFFF ||
        (int64_t)n_streams * n_sectors > 0x7FFFFFFF / 144) {
        psxhip_set_error("xa_decode_streams_host: bad argument");
        return PSXHIP_EINVAL;
    }
    const XaLayout xa = xa_layout(format, stereo, bits);
    *p = StreamsHostShape();
    p->channels = xa.channels;
    p->units_per_stream = n_sectors * xa.units_per_sector;
    p->per_channel = p->units_per_stream / xa.channels * 28;
    p->per = (size_t)p->per_channel * xa.channels;
    p->in_bytes = (size_t)n_sectors * xa.sector_bytes;
    const int rc = streams_host_strides("xa_decode_streams_host", n_streams, in_stride, out_stride, p);
    p->total_sectors = (size_t)(n_streams > 0 ? n_streams : 0) * n_sectors;
    p->unit_bytes = (size_t)(n_streams > 0 ? n_streams : 0) * p->units_per_stream * xa.record_bytes;
    p->status_bytes = sizeof(int32_t) * p->total_sectors;
    return rc;
}

#pragma GCC visibility pop
