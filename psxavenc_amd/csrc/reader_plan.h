// reader_plan.h -- what the readers' host layer (psxhip_str_demux.cpp) derives from a call's arguments alone: what it refuses, with
// which text and in which order, how a workspace or a staging buffer is carved, how much audio a PCM buffer holds and what a call returns.  Arithmetic and refusals only (no HIP), like str_plan.h:
// reader_plan.cpp builds with a host compiler alone and links against nothing but psxhip_set_error and str_plan.cpp
// (tests/test_reader_plan_cpu.py does so, under the host sanitizers); the launch code only executes these plans.  A plan function
// returns PSXHIP_OK, or PSXHIP_EINVAL with the error text set.  Pointers come as numbers: nothing here reads through one.  Nothing here
// is part of the library's surface.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/psxav_hip.h"
#include "adpcm_plan.h"           // StreamsHostShape, the ADPCM decoder's host conveniences: it lived here, and who includes this header still finds it
#include "host_layout.h"
#include "str_plan.h"
#include "strspu_chunk.h"

#pragma GCC visibility push(hidden)

constexpr int kStrDemuxScanBlock = 256;                 // PSXHIP_STR_DEMUX_SCAN_BLOCK (psxhip_str_demux.cpp asserts that they agree)
constexpr int kStrspuMaxChunks = 0x7FFFFFFF / 126;      // audio chunks whose unit records an int still counts

// ---------------------------------------------------------------------------------------------- psxhip_str_demux_device
struct StrDemuxCall {
    const psxhip_str_settings_t* s;
    int n_streams;
    uintptr_t d_sectors;
    size_t in_stream_stride;
    int n_sectors;
    int64_t first_frame;
    int max_frames;
    uintptr_t d_bs;
    size_t bs_stride, bs_stream_stride;
    uintptr_t d_bs_sizes, d_frame_info, d_xa;
    int xa_capacity;
    size_t xa_stream_stride;
    uintptr_t d_sector_table, d_summary;
};

// The workspace of psxhip_str_demux_job_t (psxhip_str_demux_internal.h), every part 256-byte placed and in this order; owner, lead and
// min lie back to back, the launch fills them with one memset
struct StrDemuxPlan {
    int sector_size, sub_at, hdr_at;
    int chunk_cap;              // chunks a row holds: bs_stride / 2016, and no more than chunk_index's 16 bits count
    int n_blocks;               // scan blocks per stream
    size_t o_rec, o_table, o_blocks, o_owner, o_lead, o_min, o_status, ws_bytes;
};
int plan_str_demux(const StrDemuxCall& c, StrDemuxPlan* p);

// ---------------------------------------------------------------------------------------------- psxhip_strspu_demux_device: the audio half
// what the STRSPU reader's entry points refuse of the settings (the muxer's refusals, str_plan.cpp: settings_error); nullptr when fine
const char* strspu_reader_settings_error(const psxhip_str_settings_t* s);
// the video half's settings: the stream as format 9, audio off
psxhip_str_settings_t strv_settings_of(const psxhip_str_settings_t* s);

struct StrspuDemuxPlan {
    StrspuChunkRules rules;
    size_t words;               // of d_owner and of d_count behind it: n_streams x audio_capacity
    size_t ws_bytes;
};
int plan_strspu_demux(const psxhip_str_settings_t* s, int n_streams, uintptr_t d_units, int audio_capacity, size_t units_stream_stride,
                      uintptr_t d_chunk_info, uintptr_t d_audio_summary, StrspuDemuxPlan* p);

// ---------------------------------------------------------------------------------------------- psxhip_spu_deinterleave_device
struct SpuDeinterleavePlan {
    size_t blocks;              // B = lane_bytes / 16
    size_t records;             // per stream: n_chunks x channels x B
    bool vec16;                 // every source block is 16-byte aligned
};
int plan_spu_deinterleave(uintptr_t d_in, int n_chunks, size_t chunk_stride, size_t lane_offset, size_t lane_bytes, int channels,
                          uintptr_t d_src_chunk, int n_streams, size_t in_stream_stride, uintptr_t d_units, size_t units_stream_stride,
                          SpuDeinterleavePlan* p);

// ---------------------------------------------------------------------------------------------- psxhip_str_read_host, psxhip_strspu_read_host
struct ReadHostCall {
    const psxhip_str_settings_t* s;
    int n_sectors, max_frames;
    int64_t pcm_capacity;
    bool sectors, frames, frame_info, decoded, pcm, summary;        // which of the caller's buffers are there
};

// One stream's staging buffer.  An audio item is an XA sector (psxhip_str_read_host) or an STRSPU chunk (psxhip_strspu_read_host);
// audio_cap of them fit the caller's PCM buffer.  The parts, 256-byte placed, in the order of the offsets below; the two summaries are
// adjacent (the STRSPU reader reads both back in one copy), the pictures come last, and 256 bytes of margin behind them.
struct ReadHostPlan {
    bool spu;
    size_t n, mf;               // the call's n_sectors and max_frames
    int sector_size;
    int chunks;                 // the widest frame the rate allows
    size_t bs_stride, frame_bytes;
    int dec_key[3];             // the decoder context's: width, height, dc_wrap
    size_t audio_cap;
    XaLayout xa;                // (XA)
    int ch, d, B;               // (STRSPU) channels, leading dummy blocks, blocks per channel per chunk
    size_t src_item, unit_item, info_item, pcm_item;        // bytes per audio item: source sector (XA), unit records, status / chunk record, PCM
    size_t o_sec, o_bs, o_sizes, o_info, o_dec, o_sum, o_asum, o_src, o_units, o_ainfo, o_states, o_pcm, o_px, reserve;
};
int plan_read_host(bool spu, const ReadHostCall& c, ReadHostPlan* p);

// XA sectors the PCM buffer holds among n: none without pcm, without channels, or in a format without subheader
size_t xa_read_capacity(const XaLayout& xa, bool audible, int64_t pcm_capacity, size_t n);
// STRSPU chunks the PCM buffer holds among n: the largest nK with 28 (nK B - d) ch <= pcm_capacity (a chain's sample_limit is an int)
size_t strspu_read_capacity(int ch, int d, bool pcm, int64_t pcm_capacity, size_t n);
// audio items decoded, given the summary's count
static inline size_t read_items_taken(const ReadHostPlan& p, int32_t count) { return (size_t)count < p.audio_cap ? (size_t)count : p.audio_cap; }
// what psxhip_str_read_host returns: samples per channel of `na` sectors
static inline int xa_read_returns(const ReadHostPlan& p, size_t na) { return p.ch ? (int)(na * (size_t)p.xa.samples_per_sector / (size_t)p.ch) : 0; }
// units per channel of nK chunks (what psxhip_strspu_read_host returns is 28 times this), 0 when there is nothing to decode
static inline int strspu_read_units(const ReadHostPlan& p, size_t nK) {
    const int n_units = nK ? (int)nK * p.B - p.d : 0;
    return n_units > 0 ? n_units : 0;
}
// the STRSPU reader's chains: channel c decodes n_units records from record d * ch + c on, every ch-th
void strspu_read_chains(psxhip_adpcm_chain_t* chains, int32_t* unit_base, int ch, int d, int n_units);

#pragma GCC visibility pop
