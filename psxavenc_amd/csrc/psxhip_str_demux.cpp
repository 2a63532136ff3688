// psxhip_str_demux.cpp -- host side of the STR / STRCD / STRV reader (psxhip_str_reader_*, psxhip_str_demux_device,
// psxhip_str_read_host; include/psxav_hip.h): argument checks, the handle's workspace and staging buffers, the
// launches (str_demux_kernels.hip), and the composition with the BS decoder and the ADPCM decoder.  Nothing is taken apart or decoded
// on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>

#include "device_buffer.h"
#include "host_layout.h"
#include "psxhip_internal.h"
#include "psxhip_str_demux_internal.h"
#include "str_plan.h"

struct psxhip_str_reader {
    int device = 0;
    DeviceBuffer ws;                  // psxhip_str_demux_device: the workspace of psxhip_str_demux_job_t
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
        psxhip_set_error("psxhip_str_demux_device: NULL settings, or a format that is none of 6 (STR), 7 (STRCD), 9 (STRV)");
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
        psxhip_set_error("psxhip_str_read_host: NULL settings, or a format that is none of 6 (STR), 7 (STRCD), 9 (STRV)");
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
