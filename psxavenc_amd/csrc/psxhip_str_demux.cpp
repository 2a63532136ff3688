// psxhip_str_demux.cpp -- host side of the STR / STRCD / STRV reader (psxhip_str_reader_*, psxhip_str_demux_device,
// psxhip_str_read_host; include/psxav_hip.h) and of the STRSPU reader (psxhip_strspu_demux_device,
// psxhip_spu_deinterleave_device, psxhip_strspu_read_host; section 16): argument checks, the handle's workspaces and staging buffers,
// the launches (str_demux_kernels.hip, strspu_demux_kernels.hip), and the composition with the BS decoder and the ADPCM decoder.
// Nothing is taken apart or decoded on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>

#include "device_buffer.h"
#include "host_layout.h"
#include "psxhip_internal.h"
#include "psxhip_str_demux_internal.h"
#include "psxhip_strspu_demux_internal.h"
#include "str_plan.h"

struct psxhip_str_reader {
    int device = 0;
    DeviceBuffer ws;                  // psxhip_str_demux_device: the workspace of psxhip_str_demux_job_t
    DeviceBuffer ws_audio;            // psxhip_strspu_demux_device: the workspace of psxhip_strspu_demux_job_t
    DeviceBuffer stage;               // psxhip_str_read_host: sectors, rows, records, XA sectors, unit records, PCM, pictures
    psxhip_mdec_decoder_t* dec = nullptr;
    int dec_key[3] = {-1, -1, -1};    // width, height, dc_wrap
};

namespace {

bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

}  // namespace

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
    psxhip_str_demux_job_t j;
    memset(&j, 0, sizeof j);
    if (!s || !str_sector_geometry(s->format, &j.sector_size, &j.sub_at, &j.hdr_at)) {
        psxhip_set_error("psxhip_str_demux_device: NULL settings, or a format that is none of 6 (STR), 7 (STRCD), 9 (STRV); format 8 (STRSPU) is "
                         "psxhip_strspu_demux_device's");
        return PSXHIP_EINVAL;
    }
    if (n_streams < 1 || n_streams > 65535 || n_sectors < 0 || max_frames < 0 || xa_capacity < 0 || first_frame < -1 ||
        first_frame > 0xFFFFFFFFll || !d_summary || (n_sectors > 0 && !d_sectors) || (max_frames > 0 && (!d_bs || !d_bs_sizes || !d_frame_info)) ||
        (xa_capacity > 0 && !d_xa)) {
        psxhip_set_error("psxhip_str_demux_device: NULL argument, or a count or first_frame out of range");
        return PSXHIP_EINVAL;
    }
    if (misaligned(d_sectors) || misaligned(d_bs) || misaligned(d_bs_sizes) || misaligned(d_frame_info) || misaligned(d_xa) ||
        misaligned(d_sector_table) || misaligned(d_summary) || (in_stream_stride & 3) || (bs_stride & 3) || (bs_stream_stride & 3) ||
        (xa_stream_stride & 3) || bs_stride < 2016) {
        psxhip_set_error("psxhip_str_demux_device: pointers and strides must be 4-byte aligned, bs_stride at least 2016");
        return PSXHIP_EINVAL;
    }
    const size_t ssz = (size_t)j.sector_size;
    if (n_streams > 1 && (in_stream_stride < ssz * (size_t)n_sectors || bs_stream_stride < bs_stride * (size_t)max_frames ||
                          xa_stream_stride < ssz * (size_t)xa_capacity)) {
        psxhip_set_error("psxhip_str_demux_device: a stream stride smaller than a stream");
        return PSXHIP_EINVAL;
    }
    if (psxhip_device_count() <= 0) return psxhip_no_device();
    if (!reader) {
        psxhip_set_error("psxhip_str_demux_device: NULL handle");
        return PSXHIP_EINVAL;
    }
    HIP_TRY(hipSetDevice(reader->device), PSXHIP_EDEVICE);

    const size_t cap = bs_stride / 2016 < 65536 ? bs_stride / 2016 : 65536;      // chunk_index is 16 bits wide
    const size_t S = (size_t)n_streams, n = (size_t)n_sectors, rows = S * (size_t)max_frames;
    const size_t n_blocks = (n + PSXHIP_STR_DEMUX_SCAN_BLOCK - 1) / PSXHIP_STR_DEMUX_SCAN_BLOCK;
    // the workspace: d_owner, d_lead and d_min back to back (one fill with ones)
    BumpOffsets o;
    const size_t o_rec = o.take(S * n * 16), o_table = o.take(S * n * sizeof(psxhip_str_sector_t)), o_blocks = o.take(S * n_blocks * 4);
    const size_t o_owner = o.take(rows * cap * 4 + rows * 4 + S * 4), o_lead = o_owner + rows * cap * 4, o_min = o_lead + rows * 4;
    const size_t o_status = o.take(rows * 4);
    const int rc = reader->ws.reserve(o.end);
    if (rc) return rc;
    uint8_t* const ws = reader->ws.as<uint8_t>();

    j.format = s->format;
    j.audio_on = j.sub_at >= 0 && s->audio_channels != 0;
    j.xa_file = s->audio_xa_file;
    j.xa_channel = s->audio_xa_channel;
    j.video_id = s->str_video_id;
    j.width = s->video_width;
    j.height = s->video_height;
    j.n_streams = n_streams;
    j.n_sectors = n_sectors;
    j.n_blocks = (int)n_blocks;
    j.max_frames = max_frames;
    j.chunk_cap = (int)cap;
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
    j.d_rec = (uint32_t*)(ws + o_rec);
    j.d_table = (psxhip_str_sector_t*)(ws + o_table);
    j.d_blocks = (uint32_t*)(ws + o_blocks);
    j.d_owner = (uint32_t*)(ws + o_owner);
    j.d_lead = (uint32_t*)(ws + o_lead);
    j.d_min = (uint32_t*)(ws + o_min);
    j.d_status = (uint32_t*)(ws + o_status);
    return psxhip_str_demux_launch(reader->device, &j, stream);
}

extern "C" int psxhip_str_read_host(psxhip_str_reader_t* reader, const psxhip_str_settings_t* s, const uint8_t* sectors, int n_sectors,
                                    int64_t first_frame, int max_frames, uint8_t* frames, psxhip_str_frame_info_t* frame_info,
                                    psxhip_mdec_decoded_t* decoded, int16_t* pcm, int64_t pcm_capacity, int32_t* xa_sector_status,
                                    psxhip_str_summary_t* summary) {
    int ssz_i = 0, sub_at = 0, hdr_at = 0;
    if (!s || !str_sector_geometry(s->format, &ssz_i, &sub_at, &hdr_at)) {
        psxhip_set_error("psxhip_str_read_host: NULL settings, or a format that is none of 6 (STR), 7 (STRCD), 9 (STRV); format 8 (STRSPU) is "
                         "psxhip_strspu_read_host's");
        return PSXHIP_EINVAL;
    }
    const int ch = s->audio_channels;
    if (n_sectors < 0 || max_frames < 0 || pcm_capacity < 0 || !summary || (n_sectors > 0 && !sectors) ||
        (max_frames > 0 && (!frame_info || !decoded)) || s->video_codec < 0 || s->video_codec > 2 || s->str_fps_num <= 0 ||
        s->str_fps_den <= 0 || (s->str_cd_speed != 1 && s->str_cd_speed != 2) || ch < 0 || ch > 2 ||
        (ch && ((s->audio_frequency != 18900 && s->audio_frequency != 37800) || (s->audio_bit_depth != 4 && s->audio_bit_depth != 8)))) {
        psxhip_set_error("psxhip_str_read_host: NULL argument, a negative count, or settings no stream can have");
        return PSXHIP_EINVAL;
    }
    // the widest frame the rate allows: the budgets of mdec.c:768-775 never pass ceil(base / den) chunks (filefmt.c:399-403,431-432)
    const StrRates rates = str_rates(s);
    const long long chunks = (long long)((rates.base + rates.den - 1) / rates.den);
    if (chunks < 1 || chunks > 65536) {
        psxhip_set_error("psxhip_str_read_host: the frame rate and CD speed give a frame %lld chunks", chunks);
        return PSXHIP_EINVAL;
    }
    if (psxhip_device_count() <= 0) return psxhip_no_device();
    if (!reader) {
        psxhip_set_error("psxhip_str_read_host: NULL handle");
        return PSXHIP_EINVAL;
    }
    HIP_TRY(hipSetDevice(reader->device), PSXHIP_EDEVICE);
    if (max_frames > 0) {
        const int key[3] = {s->video_width, s->video_height, s->video_codec == 2};
        if (!reader->dec || memcmp(key, reader->dec_key, sizeof key) != 0) {
            if (reader->dec) psxhip_mdec_decoder_destroy(reader->dec);
            reader->dec = nullptr;
            const int rc = psxhip_mdec_decoder_create(&reader->dec, reader->device, key[0], key[1], key[2]);
            if (rc) return rc;
            memcpy(reader->dec_key, key, sizeof key);
        }
    }
    const size_t ssz = (size_t)ssz_i, n = (size_t)n_sectors, mf = (size_t)max_frames, bs_stride = (size_t)chunks * 2016;
    const size_t frame_bytes = (size_t)s->video_width * s->video_height * 3 / 2;
    const int bits = s->audio_bit_depth;
    const XaLayout xa = xa_layout(s->format == 7 ? 1 : 0, ch == 2, bits);
    const size_t sector_elems = (size_t)xa.samples_per_sector;
    size_t xa_cap = 0;
    if (pcm && ch && sub_at >= 0) xa_cap = (size_t)pcm_capacity / sector_elems < n ? (size_t)pcm_capacity / sector_elems : n;
    BumpOffsets o;
    const size_t o_sec = o.take(n * ssz), o_bs = o.take(mf * bs_stride), o_sizes = o.take(mf * 4);
    const size_t o_info = o.take(mf * sizeof(psxhip_str_frame_info_t)), o_dec = o.take(mf * sizeof(psxhip_mdec_decoded_t));
    const size_t o_sum = o.take(sizeof(psxhip_str_summary_t)), o_xa = o.take(xa_cap * ssz);
    const size_t o_units = o.take(xa_cap * xa.units_per_sector * xa.record_bytes), o_xst = o.take(xa_cap * 4);
    const size_t o_states = o.take(sizeof(psxhip_adpcm_state_t) * 2), o_pcm = o.take(xa_cap * sector_elems * 2), o_px = o.end;
    int rc = reader->stage.reserve(o_px + (frames ? mf * frame_bytes : 0) + 256);
    if (rc) return rc;
    uint8_t* const d = reader->stage.as<uint8_t>();
    hipStream_t st = nullptr;
    if (n) HIP_TRY(hipMemcpyAsync(d + o_sec, sectors, n * ssz, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    if (mf) HIP_TRY(hipMemsetAsync(d + o_bs, 0, mf * bs_stride, st), PSXHIP_EDEVICE);       // row bytes no chunk covers read as zero
    // a frame that does not decode leaves its picture untouched: the pictures start from the caller's
    if (frames && mf) HIP_TRY(hipMemcpyAsync(d + o_px, frames, mf * frame_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    rc = psxhip_str_demux_device(reader, s, 1, d + o_sec, n * ssz, n_sectors, first_frame, max_frames, d + o_bs, bs_stride, mf * bs_stride,
                                 (int32_t*)(d + o_sizes), (psxhip_str_frame_info_t*)(d + o_info), d + o_xa, (int)xa_cap, xa_cap * ssz, nullptr,
                                 (psxhip_str_summary_t*)(d + o_sum), st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(summary, d + o_sum, sizeof *summary, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    if (mf) {
        rc = psxhip_mdec_decode_frames_device(reader->dec, d + o_bs, bs_stride, (const int32_t*)(d + o_sizes), 0, max_frames, nullptr,
                                              frames ? d + o_px : nullptr, frame_bytes, (psxhip_mdec_decoded_t*)(d + o_dec), st);
        if (rc) return rc;
    }
    const size_t na = (size_t)summary->n_audio < xa_cap ? (size_t)summary->n_audio : xa_cap;
    if (na) {
        rc = psxhip_xa_disassemble_device(reader->device, d + o_xa, (int)na, s->format == 7, ch == 2, s->audio_frequency, bits, d + o_units,
                                          (int32_t*)(d + o_xst), st);
        if (rc) return rc;
        const int units = (int)na * xa.units_per_sector;
        psxhip_adpcm_chain_t chains[2];
        int32_t unit_base[2];
        fill_interleaved_chains(chains, unit_base, 1, ch, 0, units / ch * 28, units);
        HIP_TRY(hipMemsetAsync(d + o_states, 0, sizeof(psxhip_adpcm_state_t) * 2, st), PSXHIP_EDEVICE);
        rc = psxhip_adpcm_decode_chains_chunked(reader->device, d + o_units, chains, unit_base, ch, 4, bits, (psxhip_adpcm_state_t*)(d + o_states),
                                                (int16_t*)(d + o_pcm), nullptr, nullptr, 0, -1, 0, st);
        if (rc < 0) return rc;
        HIP_TRY(hipMemcpyAsync(pcm, d + o_pcm, na * sector_elems * 2, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
        if (xa_sector_status) HIP_TRY(hipMemcpyAsync(xa_sector_status, d + o_xst, na * 4, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    }
    if (mf) {
        HIP_TRY(hipMemcpyAsync(frame_info, d + o_info, mf * sizeof *frame_info, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
        HIP_TRY(hipMemcpyAsync(decoded, d + o_dec, mf * sizeof *decoded, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
        if (frames) HIP_TRY(hipMemcpyAsync(frames, d + o_px, mf * frame_bytes, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    }
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return ch ? (int)(na * sector_elems / (size_t)ch) : 0;
}

// ---------------------------------------------------------------------------------------------- STRSPU

namespace {

constexpr int kStrspuMaxChunks = 0x7FFFFFFF / 126;

// what the STRSPU reader's entry points refuse of the settings (the muxer's refusals, str_plan.cpp: settings_error); nullptr when fine
const char* strspu_reader_settings_error(const psxhip_str_settings_t* s) {
    if (!s || s->format != FORMAT_STRSPU) return "NULL settings, or a format that is not 8 (STRSPU)";
    if (s->audio_channels < 0 || s->audio_channels > 2) return "audio_channels is none of 0, 1, 2";
    if ((uint32_t)s->strspu_options & ~kStrspuOptionBits) return "unknown bit set in strspu_options";
    if (s->audio_channels) {
        if (s->str_video_id == -1) return "str_video_id -1 (any) cannot tell video chunks from audio chunks";
        if (((uint32_t)s->strspu_options & PSXHIP_STRSPU_ID_MASK) == ((uint32_t)s->str_video_id & 0xFFFFu))
            return "the audio chunk id of strspu_options equals str_video_id";
    }
    return nullptr;
}

// the video half's settings: the stream as format 9, audio off
psxhip_str_settings_t strv_settings_of(const psxhip_str_settings_t* s) {
    psxhip_str_settings_t v = *s;
    v.format = FORMAT_STRV;
    v.audio_channels = 0;
    return v;
}

}  // namespace

extern "C" const char* psxhip_strspu_demux_kernel_rev(void) { return PSXHIP_STRSPU_DEMUX_KERNEL_REV; }

extern "C" int psxhip_strspu_demux_device(psxhip_str_reader_t* reader, const psxhip_str_settings_t* s, int n_streams, const uint8_t* d_sectors,
                                          size_t in_stream_stride, int n_sectors, int64_t first_frame, int max_frames, uint8_t* d_bs,
                                          size_t bs_stride, size_t bs_stream_stride, int32_t* d_bs_sizes, psxhip_str_frame_info_t* d_frame_info,
                                          uint8_t* d_units, int audio_capacity, size_t units_stream_stride,
                                          psxhip_strspu_chunk_info_t* d_chunk_info, psxhip_str_sector_t* d_sector_table,
                                          psxhip_str_summary_t* d_summary, psxhip_strspu_audio_summary_t* d_audio_summary, void* stream) {
    if (const char* why = strspu_reader_settings_error(s)) {
        psxhip_set_error("psxhip_strspu_demux_device: %s", why);
        return PSXHIP_EINVAL;
    }
    if (n_streams < 1 || n_streams > 65535 || audio_capacity < 0 || audio_capacity > kStrspuMaxChunks || !d_audio_summary ||
        (audio_capacity > 0 && (!d_units || !d_chunk_info))) {
        psxhip_set_error("psxhip_strspu_demux_device: NULL argument, or audio_capacity outside 0 .. (2^31 - 1) / 126");
        return PSXHIP_EINVAL;
    }
    if (((uintptr_t)d_units & 15) || (units_stream_stride & 15) || misaligned(d_chunk_info) || misaligned(d_audio_summary)) {
        psxhip_set_error("psxhip_strspu_demux_device: d_units and units_stream_stride must be 16-byte aligned, the records 4-byte aligned");
        return PSXHIP_EINVAL;
    }
    if (n_streams > 1 && units_stream_stride < (size_t)audio_capacity * 126 * 16) {
        psxhip_set_error("psxhip_strspu_demux_device: a stream stride smaller than a stream");
        return PSXHIP_EINVAL;
    }
    // the video half: the STR reader over the stream as format 9 (its checks, its workspace, its launches)
    const psxhip_str_settings_t v = strv_settings_of(s);
    int rc = psxhip_str_demux_device(reader, &v, n_streams, d_sectors, in_stream_stride, n_sectors, first_frame, max_frames, d_bs, bs_stride,
                                     bs_stream_stride, d_bs_sizes, d_frame_info, nullptr, 0, 0, d_sector_table, d_summary, stream);
    if (rc) return rc;

    const size_t words = (size_t)n_streams * (size_t)audio_capacity;
    rc = reader->ws_audio.reserve(2 * words * sizeof(uint32_t));
    if (rc) return rc;
    psxhip_strspu_demux_job_t j;
    memset(&j, 0, sizeof j);
    j.rules.ch = s->audio_channels;
    j.rules.id = (uint32_t)s->strspu_options & PSXHIP_STRSPU_ID_MASK;
    j.rules.d = strspu_dummy_of((uint32_t)s->strspu_options);
    j.rules.loop = ((uint32_t)s->strspu_options & PSXHIP_STRSPU_LOOP) != 0;
    j.rules.frequency = (uint32_t)s->audio_frequency;
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
    j.d_count = j.d_owner + words;
    return psxhip_strspu_demux_launch(reader->device, &j, stream);
}

extern "C" int psxhip_spu_deinterleave_device(int device, const uint8_t* d_in, int n_chunks, size_t chunk_stride, size_t lane_offset,
                                              size_t lane_bytes, int channels, const int32_t* d_src_chunk, int n_streams,
                                              size_t in_stream_stride, uint8_t* d_units, size_t units_stream_stride, void* stream) {
    if (n_chunks < 0 || n_streams < 1 || n_streams > 65535 || channels < 1 || lane_bytes == 0 || (lane_bytes & 15) ||
        (n_chunks > 0 && (!d_in || !d_units))) {
        psxhip_set_error("psxhip_spu_deinterleave_device: NULL argument, a count out of range, or lane_bytes no positive multiple of 16");
        return PSXHIP_EINVAL;
    }
    if (misaligned(d_in) || misaligned(d_src_chunk) || (chunk_stride & 3) || (lane_offset & 3) || (in_stream_stride & 3) ||
        ((uintptr_t)d_units & 15) || (units_stream_stride & 15)) {
        psxhip_set_error("psxhip_spu_deinterleave_device: d_in, lane_offset and the strides must be 4-byte aligned, d_units and its stride 16-byte aligned");
        return PSXHIP_EINVAL;
    }
    // lane_offset + channels * lane_bytes <= chunk_stride, and n_chunks * channels * B records within an int, without overflow
    const size_t blocks = lane_bytes / 16;
    if (lane_offset > chunk_stride || (size_t)channels > (chunk_stride - lane_offset) / lane_bytes ||
        (n_chunks > 0 && (size_t)channels * blocks > (size_t)0x7FFFFFFF / (size_t)n_chunks)) {
        psxhip_set_error("psxhip_spu_deinterleave_device: the lanes overrun chunk_stride, or more than 2^31 - 1 records");
        return PSXHIP_EINVAL;
    }
    const size_t records = (size_t)n_chunks * (size_t)channels * blocks;
    if (n_streams > 1 && (units_stream_stride < records * 16 || (!d_src_chunk && in_stream_stride < (size_t)n_chunks * chunk_stride))) {
        psxhip_set_error("psxhip_spu_deinterleave_device: a stream stride smaller than a stream");
        return PSXHIP_EINVAL;
    }
    if (psxhip_device_count() <= 0) return psxhip_no_device();
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    psxhip_spu_deinterleave_job_t j;
    memset(&j, 0, sizeof j);
    j.in = d_in;
    j.in_stream_stride = in_stream_stride;
    j.chunk_stride = chunk_stride;
    j.lane_offset = lane_offset;
    j.blocks = (int)blocks;
    j.channels = channels;
    j.n_chunks = n_chunks;
    j.src_chunk = d_src_chunk;
    j.src_stream_stride = 0;
    j.units = d_units;
    j.units_stream_stride = units_stream_stride;
    j.vec16 = (((uintptr_t)d_in + lane_offset) & 15) == 0 && (chunk_stride & 15) == 0 && (n_streams == 1 || (in_stream_stride & 15) == 0);
    return psxhip_spu_deinterleave_launch(&j, n_streams, stream);
}

extern "C" int psxhip_strspu_read_host(psxhip_str_reader_t* reader, const psxhip_str_settings_t* s, const uint8_t* sectors, int n_sectors,
                                       int64_t first_frame, int max_frames, uint8_t* frames, psxhip_str_frame_info_t* frame_info,
                                       psxhip_mdec_decoded_t* decoded, int16_t* pcm, int64_t pcm_capacity,
                                       psxhip_strspu_chunk_info_t* chunk_info, psxhip_str_summary_t* summary,
                                       psxhip_strspu_audio_summary_t* audio_summary) {
    if (const char* why = strspu_reader_settings_error(s)) {
        psxhip_set_error("psxhip_strspu_read_host: %s", why);
        return PSXHIP_EINVAL;
    }
    const int ch = s->audio_channels;
    if (n_sectors < 0 || max_frames < 0 || pcm_capacity < 0 || !summary || (n_sectors > 0 && !sectors) ||
        (max_frames > 0 && (!frame_info || !decoded)) || s->video_codec < 0 || s->video_codec > 2 || s->str_fps_num <= 0 ||
        s->str_fps_den <= 0 || (s->str_cd_speed != 1 && s->str_cd_speed != 2) || s->audio_frequency < 0) {
        psxhip_set_error("psxhip_strspu_read_host: NULL argument, a negative count, or settings no stream can have");
        return PSXHIP_EINVAL;
    }
    // the widest frame the rate allows: the stream's budgets (section 15) never pass those of the stream without audio
    const psxhip_str_settings_t v = strv_settings_of(s);
    const StrRates rates = str_rates(&v);
    const long long chunks = (long long)((rates.base + rates.den - 1) / rates.den);
    if (chunks < 1 || chunks > 65536) {
        psxhip_set_error("psxhip_strspu_read_host: the frame rate and CD speed give a frame %lld chunks", chunks);
        return PSXHIP_EINVAL;
    }
    if (psxhip_device_count() <= 0) return psxhip_no_device();
    if (!reader) {
        psxhip_set_error("psxhip_strspu_read_host: NULL handle");
        return PSXHIP_EINVAL;
    }
    HIP_TRY(hipSetDevice(reader->device), PSXHIP_EDEVICE);
    if (max_frames > 0) {
        const int key[3] = {s->video_width, s->video_height, s->video_codec == 2};
        if (!reader->dec || memcmp(key, reader->dec_key, sizeof key) != 0) {
            if (reader->dec) psxhip_mdec_decoder_destroy(reader->dec);
            reader->dec = nullptr;
            const int rc = psxhip_mdec_decoder_create(&reader->dec, reader->device, key[0], key[1], key[2]);
            if (rc) return rc;
            memcpy(reader->dec_key, key, sizeof key);
        }
    }
    const size_t ssz = 2048, n = (size_t)n_sectors, mf = (size_t)max_frames, bs_stride = (size_t)chunks * 2016;
    const size_t frame_bytes = (size_t)s->video_width * s->video_height * 3 / 2;
    const int d = strspu_dummy_of((uint32_t)s->strspu_options), B = ch ? 126 / ch : 0;
    // the chunks the PCM buffer holds: the largest nK with 28 (nK B - d) ch <= pcm_capacity, and no more than there are sectors
    size_t cap = 0;
    if (pcm && ch) {
        const int64_t held = (pcm_capacity / (28 * ch) + d) / B;
        cap = (size_t)held < n ? (size_t)held : n;
        if (cap > (size_t)kStrspuMaxChunks / 28) cap = (size_t)kStrspuMaxChunks / 28;         // (a chain's sample_limit is an int)
    }
    BumpOffsets o;
    const size_t o_sec = o.take(n * ssz), o_bs = o.take(mf * bs_stride), o_sizes = o.take(mf * 4);
    const size_t o_info = o.take(mf * sizeof(psxhip_str_frame_info_t)), o_dec = o.take(mf * sizeof(psxhip_mdec_decoded_t));
    const size_t o_sum = o.take(sizeof(psxhip_str_summary_t) + sizeof(psxhip_strspu_audio_summary_t));
    const size_t o_asum = o_sum + sizeof(psxhip_str_summary_t);
    const size_t o_units = o.take(cap * 126 * 16), o_cinfo = o.take(cap * sizeof(psxhip_strspu_chunk_info_t));
    const size_t o_states = o.take(sizeof(psxhip_adpcm_state_t) * 2), o_pcm = o.take(cap * 126 * 28 * 2), o_px = o.end;
    int rc = reader->stage.reserve(o_px + (frames ? mf * frame_bytes : 0) + 256);
    if (rc) return rc;
    uint8_t* const dv = reader->stage.as<uint8_t>();
    hipStream_t st = nullptr;
    if (n) HIP_TRY(hipMemcpyAsync(dv + o_sec, sectors, n * ssz, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    if (mf) HIP_TRY(hipMemsetAsync(dv + o_bs, 0, mf * bs_stride, st), PSXHIP_EDEVICE);      // row bytes no chunk covers read as zero
    if (cap) HIP_TRY(hipMemsetAsync(dv + o_units, 0, cap * 126 * 16, st), PSXHIP_EDEVICE);  // a missing chunk decodes as silence
    if (frames && mf) HIP_TRY(hipMemcpyAsync(dv + o_px, frames, mf * frame_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    rc = psxhip_strspu_demux_device(reader, s, 1, dv + o_sec, n * ssz, n_sectors, first_frame, max_frames, dv + o_bs, bs_stride, mf * bs_stride,
                                    (int32_t*)(dv + o_sizes), (psxhip_str_frame_info_t*)(dv + o_info), dv + o_units, (int)cap, cap * 126 * 16,
                                    (psxhip_strspu_chunk_info_t*)(dv + o_cinfo), nullptr, (psxhip_str_summary_t*)(dv + o_sum),
                                    (psxhip_strspu_audio_summary_t*)(dv + o_asum), st);
    if (rc) return rc;
    struct { psxhip_str_summary_t video; psxhip_strspu_audio_summary_t audio; } sums;
    HIP_TRY(hipMemcpyAsync(&sums, dv + o_sum, sizeof sums, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    *summary = sums.video;
    if (audio_summary) *audio_summary = sums.audio;
    if (mf) {
        rc = psxhip_mdec_decode_frames_device(reader->dec, dv + o_bs, bs_stride, (const int32_t*)(dv + o_sizes), 0, max_frames, nullptr,
                                              frames ? dv + o_px : nullptr, frame_bytes, (psxhip_mdec_decoded_t*)(dv + o_dec), st);
        if (rc) return rc;
    }
    const size_t nK = (size_t)sums.audio.n_chunks < cap ? (size_t)sums.audio.n_chunks : cap;
    const int n_units = nK ? (int)nK * B - d : 0;
    if (n_units > 0) {
        psxhip_adpcm_chain_t chains[2];
        int32_t unit_base[2];
        for (int c = 0; c < ch; c++) {
            chains[c].sample_offset = c;
            chains[c].pitch = ch;
            chains[c].sample_limit = 28 * n_units;
            chains[c].n_units = n_units;
            chains[c].unit_stride = ch;
            unit_base[c] = d * ch + c;
        }
        HIP_TRY(hipMemsetAsync(dv + o_states, 0, sizeof(psxhip_adpcm_state_t) * 2, st), PSXHIP_EDEVICE);
        rc = psxhip_adpcm_decode_chains_chunked(reader->device, dv + o_units, chains, unit_base, ch, 5, 4, (psxhip_adpcm_state_t*)(dv + o_states),
                                                (int16_t*)(dv + o_pcm), nullptr, nullptr, 0, -1, 0, st);
        if (rc < 0) return rc;
        HIP_TRY(hipMemcpyAsync(pcm, dv + o_pcm, (size_t)n_units * 28 * ch * 2, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    }
    if (chunk_info && cap)
        HIP_TRY(hipMemcpyAsync(chunk_info, dv + o_cinfo, cap * sizeof *chunk_info, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    if (mf) {
        HIP_TRY(hipMemcpyAsync(frame_info, dv + o_info, mf * sizeof *frame_info, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
        HIP_TRY(hipMemcpyAsync(decoded, dv + o_dec, mf * sizeof *decoded, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
        if (frames) HIP_TRY(hipMemcpyAsync(frames, dv + o_px, mf * frame_bytes, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    }
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return n_units > 0 ? 28 * n_units : 0;
}
