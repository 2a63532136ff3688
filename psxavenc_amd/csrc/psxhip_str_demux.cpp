// psxhip_str_demux.cpp -- host side of the STR / STRCD / STRV reader (psxhip_str_reader_*, psxhip_str_demux_device,
// psxhip_str_read_host; include/psxav_hip.h) and of the STRSPU reader (psxhip_strspu_demux_device,
// psxhip_spu_deinterleave_device, psxhip_strspu_read_host; section 16): the device and handle checks, the handle's workspaces and staging buffers,
// the launches (str_demux_kernels.hip, strspu_demux_kernels.hip), and the composition with the BS decoder and the ADPCM decoder.
// What a call is refused for, how its workspace or staging buffer is carved and what it returns is reader_plan.cpp's (no HIP); this file
// executes those plans.  Nothing is taken apart or decoded on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>

#include "device_buffer.h"
#include "host_layout.h"
#include "psxhip_internal.h"
#include "psxhip_str_demux_internal.h"
#include "psxhip_strspu_demux_internal.h"
#include "reader_plan.h"

struct psxhip_str_reader {
    int device = 0;
    DeviceBuffer ws;                  // psxhip_str_demux_device: the workspace of psxhip_str_demux_job_t
    DeviceBuffer ws_audio;            // psxhip_strspu_demux_device: the workspace of psxhip_strspu_demux_job_t
    DeviceBuffer stage;               // psxhip_str_read_host: sectors, rows, records, XA sectors, unit records, PCM, pictures
    psxhip_mdec_decoder_t* dec = nullptr;
    int dec_key[3] = {-1, -1, -1};    // width, height, dc_wrap
};

static_assert(kStrDemuxScanBlock == PSXHIP_STR_DEMUX_SCAN_BLOCK, "the plan's scan blocks are the kernels'");

extern "C" const char* psxhip_str_demux_kernel_rev(void) { return PSXHIP_STR_DEMUX_KERNEL_REV; }

extern "C" int psxhip_str_reader_create(psxhip_str_reader_t** out, int device) {
    if (!out) return PSXHIP_EINVAL;
    *out = nullptr;
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    psxhip_str_reader* r = new (std::nothrow) psxhip_str_reader;
    if (!r) return PSXHIP_ENOMEM;
    r->device = device;
    *out = r;
    return PSXHIP_OK;
}

extern "C" void psxhip_str_reader_destroy(psxhip_str_reader_t* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->dec) psxhip_mdec_decoder_destroy(r->dec);
    delete r;
}

extern "C" int psxhip_str_demux_device(psxhip_str_reader_t* reader, const psxhip_str_settings_t* s, int n_streams, const uint8_t* d_sectors,
                                       size_t in_stream_stride, int n_sectors, int64_t first_frame, int max_frames, uint8_t* d_bs,
                                       size_t bs_stride, size_t bs_stream_stride, int32_t* d_bs_sizes, psxhip_str_frame_info_t* d_frame_info,
                                       uint8_t* d_xa, int xa_capacity, size_t xa_stream_stride, psxhip_str_sector_t* d_sector_table,
                                       psxhip_str_summary_t* d_summary, void* stream) {
    const StrDemuxCall c = {s, n_streams, (uintptr_t)d_sectors, in_stream_stride, n_sectors, first_frame, max_frames, (uintptr_t)d_bs,
                            bs_stride, bs_stream_stride, (uintptr_t)d_bs_sizes, (uintptr_t)d_frame_info, (uintptr_t)d_xa, xa_capacity,
                            xa_stream_stride, (uintptr_t)d_sector_table, (uintptr_t)d_summary};
    StrDemuxPlan p;
    int rc = plan_str_demux(c, &p);
    if (rc) return rc;
    if (psxhip_device_count() <= 0) return psxhip_no_device();
    if (!reader) {
        psxhip_set_error("psxhip_str_demux_device: NULL handle");
        return PSXHIP_EINVAL;
    }
    HIP_TRY(hipSetDevice(reader->device), PSXHIP_EDEVICE);
    rc = reader->ws.reserve(p.ws_bytes);
    if (rc) return rc;
    uint8_t* const ws = reader->ws.as<uint8_t>();

    psxhip_str_demux_job_t j;
    memset(&j, 0, sizeof j);
    j.format = s->format;
    j.sector_size = p.sector_size;
    j.sub_at = p.sub_at;
    j.hdr_at = p.hdr_at;
    j.audio_on = j.sub_at >= 0 && s->audio_channels != 0;
    j.xa_file = s->audio_xa_file;
    j.xa_channel = s->audio_xa_channel;
    j.video_id = s->str_video_id;
    j.width = s->video_width;
    j.height = s->video_height;
    j.n_streams = n_streams;
    j.n_sectors = n_sectors;
    j.n_blocks = p.n_blocks;
    j.max_frames = max_frames;
    j.chunk_cap = p.chunk_cap;
    j.xa_capacity = xa_capacity;
    j.first_frame = first_frame;
    j.d_sectors = d_sectors;
    j.in_stream_stride = in_stream_stride;
    j.d_bs = d_bs;
    j.bs_stride = bs_stride;
    j.bs_stream_stride = bs_stream_stride;
    j.d_bs_sizes = d_bs_sizes;
    j.d_info = d_frame_info;
    j.d_xa = d_xa;
    j.xa_stream_stride = xa_stream_stride;
    j.d_user_table = d_sector_table;
    j.d_summary = d_summary;
    j.d_rec = (uint32_t*)(ws + p.o_rec);
    j.d_table = (psxhip_str_sector_t*)(ws + p.o_table);
    j.d_blocks = (uint32_t*)(ws + p.o_blocks);
    j.d_owner = (uint32_t*)(ws + p.o_owner);
    j.d_lead = (uint32_t*)(ws + p.o_lead);
    j.d_min = (uint32_t*)(ws + p.o_min);
    j.d_status = (uint32_t*)(ws + p.o_status);
    return psxhip_str_demux_launch(reader->device, &j, stream);
}

// ---------------------------------------------------------------------------------------------- STRSPU

extern "C" const char* psxhip_strspu_demux_kernel_rev(void) { return PSXHIP_STRSPU_DEMUX_KERNEL_REV; }

extern "C" int psxhip_strspu_demux_device(psxhip_str_reader_t* reader, const psxhip_str_settings_t* s, int n_streams, const uint8_t* d_sectors,
                                          size_t in_stream_stride, int n_sectors, int64_t first_frame, int max_frames, uint8_t* d_bs,
                                          size_t bs_stride, size_t bs_stream_stride, int32_t* d_bs_sizes, psxhip_str_frame_info_t* d_frame_info,
                                          uint8_t* d_units, int audio_capacity, size_t units_stream_stride,
                                          psxhip_strspu_chunk_info_t* d_chunk_info, psxhip_str_sector_t* d_sector_table,
                                          psxhip_str_summary_t* d_summary, psxhip_strspu_audio_summary_t* d_audio_summary, void* stream) {
    StrspuDemuxPlan p;
    int rc = plan_strspu_demux(s, n_streams, (uintptr_t)d_units, audio_capacity, units_stream_stride, (uintptr_t)d_chunk_info,
                               (uintptr_t)d_audio_summary, &p);
    if (rc) return rc;
    // the video half: the STR reader over the stream as format 9 (its checks, the device and handle checks, its workspace, its launches)
    const psxhip_str_settings_t v = strv_settings_of(s);
    rc = psxhip_str_demux_device(reader, &v, n_streams, d_sectors, in_stream_stride, n_sectors, first_frame, max_frames, d_bs, bs_stride,
                                 bs_stream_stride, d_bs_sizes, d_frame_info, nullptr, 0, 0, d_sector_table, d_summary, stream);
    if (rc) return rc;
    rc = reader->ws_audio.reserve(p.ws_bytes);
    if (rc) return rc;

    psxhip_strspu_demux_job_t j;
    memset(&j, 0, sizeof j);
    j.rules = p.rules;
    j.n_streams = n_streams;
    j.n_sectors = n_sectors;
    j.audio_capacity = audio_capacity;
    j.d_sectors = d_sectors;
    j.in_stream_stride = in_stream_stride;
    j.d_units = d_units;
    j.units_stream_stride = units_stream_stride;
    j.d_chunk_info = d_chunk_info;
    j.d_user_table = d_sector_table;
    j.d_summary = d_summary;
    j.d_audio_summary = d_audio_summary;
    j.d_owner = reader->ws_audio.as<uint32_t>();
    j.d_count = j.d_owner + p.words;
    return psxhip_strspu_demux_launch(reader->device, &j, stream);
}

extern "C" int psxhip_spu_deinterleave_device(int device, const uint8_t* d_in, int n_chunks, size_t chunk_stride, size_t lane_offset,
                                              size_t lane_bytes, int channels, const int32_t* d_src_chunk, int n_streams,
                                              size_t in_stream_stride, uint8_t* d_units, size_t units_stream_stride, void* stream) {
    SpuDeinterleavePlan p;
    int rc = plan_spu_deinterleave((uintptr_t)d_in, n_chunks, chunk_stride, lane_offset, lane_bytes, channels, (uintptr_t)d_src_chunk, n_streams,
                                   in_stream_stride, (uintptr_t)d_units, units_stream_stride, &p);
    if (rc) return rc;
    if (psxhip_device_count() <= 0) return psxhip_no_device();
    rc = psxhip_ensure_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    psxhip_spu_deinterleave_job_t j;
    memset(&j, 0, sizeof j);
    j.in = d_in;
    j.in_stream_stride = in_stream_stride;
    j.chunk_stride = chunk_stride;
    j.lane_offset = lane_offset;
    j.blocks = (int)p.blocks;
    j.channels = channels;
    j.n_chunks = n_chunks;
    j.src_chunk = d_src_chunk;
    j.src_stream_stride = 0;
    j.units = d_units;
    j.units_stream_stride = units_stream_stride;
    j.vec16 = p.vec16;
    return psxhip_spu_deinterleave_launch(&j, n_streams, stream);
}

// ---------------------------------------------------------------------------------------------- the _host readers

namespace {

// the caller's buffers of a _host call
struct ReadHostBuffers {
    const uint8_t* sectors;
    uint8_t* frames;
    psxhip_str_frame_info_t* frame_info;
    psxhip_mdec_decoded_t* decoded;
    psxhip_str_summary_t* summary;
    psxhip_strspu_audio_summary_t* audio_summary;       // (STRSPU, optional)
};

struct ReadHostSummaries {          // as they lie in the staging buffer
    psxhip_str_summary_t video;
    psxhip_strspu_audio_summary_t audio;
};

// the reader's BS decoder is the one of this picture size and DC rule
int ensure_decoder(psxhip_str_reader_t* reader, const int (&key)[3]) {
    if (reader->dec && memcmp(key, reader->dec_key, sizeof key) == 0) return PSXHIP_OK;
    if (reader->dec) psxhip_mdec_decoder_destroy(reader->dec);
    reader->dec = nullptr;
    const int rc = psxhip_mdec_decoder_create(&reader->dec, reader->device, key[0], key[1], key[2]);
    if (rc) return rc;
    memcpy(reader->dec_key, key, sizeof key);
    return PSXHIP_OK;
}

// What both _host readers do around their demux call and their audio leg, on the null stream: stage the sectors, zero the rows (and an
// STRSPU call's unit records), start the pictures from the caller's, demux(d, st), read the summaries back, decode the rows, audio(d,
// st, sums) -- it decodes and queues the downloads of what the summaries count, and returns the call's value or an error --, then the
// downloads of the video half.
template <class Demux, class Audio>
int read_host(psxhip_str_reader_t* reader, const ReadHostPlan& p, const ReadHostBuffers& b, Demux demux, Audio audio) {
    if (psxhip_device_count() <= 0) return psxhip_no_device();
    if (!reader) {
        psxhip_set_error("%s: NULL handle", p.spu ? "psxhip_strspu_read_host" : "psxhip_str_read_host");
        return PSXHIP_EINVAL;
    }
    HIP_TRY(hipSetDevice(reader->device), PSXHIP_EDEVICE);
    int rc;
    if (p.mf && (rc = ensure_decoder(reader, p.dec_key))) return rc;
    if ((rc = reader->stage.reserve(p.reserve))) return rc;
    uint8_t* const d = reader->stage.as<uint8_t>();
    const size_t n = p.n, mf = p.mf, picture_bytes = mf * p.frame_bytes;
    hipStream_t st = nullptr;
    if (n) HIP_TRY(hipMemcpyAsync(d + p.o_sec, b.sectors, n * (size_t)p.sector_size, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    if (mf) HIP_TRY(hipMemsetAsync(d + p.o_bs, 0, mf * p.bs_stride, st), PSXHIP_EDEVICE);       // row bytes no chunk covers read as zero
    if (p.spu && p.audio_cap)                                                                   // a missing chunk decodes as silence
        HIP_TRY(hipMemsetAsync(d + p.o_units, 0, p.audio_cap * p.unit_item, st), PSXHIP_EDEVICE);
    // a frame that does not decode leaves its picture untouched: the pictures start from the caller's
    if (b.frames && mf) HIP_TRY(hipMemcpyAsync(d + p.o_px, b.frames, picture_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    if ((rc = demux(d, st))) return rc;
    ReadHostSummaries sums;
    HIP_TRY(hipMemcpyAsync(&sums, d + p.o_sum, p.spu ? sizeof sums : sizeof sums.video, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    *b.summary = sums.video;
    if (p.spu && b.audio_summary) *b.audio_summary = sums.audio;
    if (mf) {
        rc = psxhip_mdec_decode_frames_device(reader->dec, d + p.o_bs, p.bs_stride, (const int32_t*)(d + p.o_sizes), 0, (int)mf, nullptr,
                                              b.frames ? d + p.o_px : nullptr, p.frame_bytes, (psxhip_mdec_decoded_t*)(d + p.o_dec), st);
        if (rc) return rc;
    }
    const int value = audio(d, st, sums);
    if (value < 0) return value;
    if (mf) {
        HIP_TRY(hipMemcpyAsync(b.frame_info, d + p.o_info, mf * sizeof *b.frame_info, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
        HIP_TRY(hipMemcpyAsync(b.decoded, d + p.o_dec, mf * sizeof *b.decoded, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
        if (b.frames) HIP_TRY(hipMemcpyAsync(b.frames, d + p.o_px, picture_bytes, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    }
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return value;
}

// the audio legs' decode: `ch` chains from zero states over the unit records into the staged PCM
int decode_staged(psxhip_str_reader_t* reader, const ReadHostPlan& p, uint8_t* d, const psxhip_adpcm_chain_t* chains, const int32_t* unit_base,
                  int filter_count, int bits, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(d + p.o_states, 0, sizeof(psxhip_adpcm_state_t) * 2, st), PSXHIP_EDEVICE);
    const int rc = psxhip_adpcm_decode_chains_chunked(reader->device, d + p.o_units, chains, unit_base, p.ch, filter_count, bits,
                                                      (psxhip_adpcm_state_t*)(d + p.o_states), (int16_t*)(d + p.o_pcm), nullptr, nullptr, 0, -1, 0,
                                                      st);
    return rc < 0 ? rc : PSXHIP_OK;
}

}  // namespace

extern "C" int psxhip_str_read_host(psxhip_str_reader_t* reader, const psxhip_str_settings_t* s, const uint8_t* sectors, int n_sectors,
                                    int64_t first_frame, int max_frames, uint8_t* frames, psxhip_str_frame_info_t* frame_info,
                                    psxhip_mdec_decoded_t* decoded, int16_t* pcm, int64_t pcm_capacity, int32_t* xa_sector_status,
                                    psxhip_str_summary_t* summary) {
    const ReadHostCall c = {s, n_sectors, max_frames, pcm_capacity, sectors != nullptr, frames != nullptr, frame_info != nullptr,
                            decoded != nullptr, pcm != nullptr, summary != nullptr};
    ReadHostPlan p;
    const int refused = plan_read_host(false, c, &p);
    if (refused) return refused;
    const size_t ssz = (size_t)p.sector_size;
    return read_host(
        reader, p, {sectors, frames, frame_info, decoded, summary, nullptr},
        [&](uint8_t* d, hipStream_t st) -> int {
            return psxhip_str_demux_device(reader, s, 1, d + p.o_sec, p.n * ssz, n_sectors, first_frame, max_frames, d + p.o_bs, p.bs_stride,
                                           p.mf * p.bs_stride, (int32_t*)(d + p.o_sizes), (psxhip_str_frame_info_t*)(d + p.o_info), d + p.o_src,
                                           (int)p.audio_cap, p.audio_cap * ssz, nullptr, (psxhip_str_summary_t*)(d + p.o_sum), st);
        },
        [&](uint8_t* d, hipStream_t st, const ReadHostSummaries& sums) -> int {
            const size_t na = read_items_taken(p, sums.video.n_audio);
            if (na) {
                int rc = psxhip_xa_disassemble_device(reader->device, d + p.o_src, (int)na, s->format == 7, p.ch == 2, s->audio_frequency,
                                                      s->audio_bit_depth, d + p.o_units, (int32_t*)(d + p.o_ainfo), st);
                if (rc) return rc;
                const int units = (int)na * p.xa.units_per_sector;
                psxhip_adpcm_chain_t chains[2];
                int32_t unit_base[2];
                fill_interleaved_chains(chains, unit_base, 1, p.ch, 0, units / p.ch * 28, units);
                if ((rc = decode_staged(reader, p, d, chains, unit_base, 4, s->audio_bit_depth, st))) return rc;
                HIP_TRY(hipMemcpyAsync(pcm, d + p.o_pcm, na * p.pcm_item, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
                if (xa_sector_status) HIP_TRY(hipMemcpyAsync(xa_sector_status, d + p.o_ainfo, na * 4, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
            }
            return xa_read_returns(p, na);
        });
}

extern "C" int psxhip_strspu_read_host(psxhip_str_reader_t* reader, const psxhip_str_settings_t* s, const uint8_t* sectors, int n_sectors,
                                       int64_t first_frame, int max_frames, uint8_t* frames, psxhip_str_frame_info_t* frame_info,
                                       psxhip_mdec_decoded_t* decoded, int16_t* pcm, int64_t pcm_capacity,
                                       psxhip_strspu_chunk_info_t* chunk_info, psxhip_str_summary_t* summary,
                                       psxhip_strspu_audio_summary_t* audio_summary) {
    const ReadHostCall c = {s, n_sectors, max_frames, pcm_capacity, sectors != nullptr, frames != nullptr, frame_info != nullptr,
                            decoded != nullptr, pcm != nullptr, summary != nullptr};
    ReadHostPlan p;
    const int refused = plan_read_host(true, c, &p);
    if (refused) return refused;
    const size_t cap = p.audio_cap;
    return read_host(
        reader, p, {sectors, frames, frame_info, decoded, summary, audio_summary},
        [&](uint8_t* d, hipStream_t st) -> int {
            return psxhip_strspu_demux_device(reader, s, 1, d + p.o_sec, p.n * 2048, n_sectors, first_frame, max_frames, d + p.o_bs, p.bs_stride,
                                              p.mf * p.bs_stride, (int32_t*)(d + p.o_sizes), (psxhip_str_frame_info_t*)(d + p.o_info),
                                              d + p.o_units, (int)cap, cap * p.unit_item, (psxhip_strspu_chunk_info_t*)(d + p.o_ainfo), nullptr,
                                              (psxhip_str_summary_t*)(d + p.o_sum), (psxhip_strspu_audio_summary_t*)(d + p.o_asum), st);
        },
        [&](uint8_t* d, hipStream_t st, const ReadHostSummaries& sums) -> int {
            const int n_units = strspu_read_units(p, read_items_taken(p, sums.audio.n_chunks));
            if (n_units) {
                psxhip_adpcm_chain_t chains[2];
                int32_t unit_base[2];
                strspu_read_chains(chains, unit_base, p.ch, p.d, n_units);
                const int rc = decode_staged(reader, p, d, chains, unit_base, 5, 4, st);
                if (rc) return rc;
                HIP_TRY(hipMemcpyAsync(pcm, d + p.o_pcm, (size_t)n_units * 28 * p.ch * 2, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
            }
            if (chunk_info && cap)
                HIP_TRY(hipMemcpyAsync(chunk_info, d + p.o_ainfo, cap * sizeof *chunk_info, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
            return 28 * n_units;
        });
}
