// reader_plan.cpp -- the readers' plans (reader_plan.h): every refusal of psxhip_str_demux_device, psxhip_strspu_demux_device,
// psxhip_spu_deinterleave_device and the two _host readers with its text and its place in the order, the workspace of a demux call and
// the staging buffer of a _host call.  No HIP and no device: psxhip_str_demux.cpp reserves and launches what a plan names.
#include "reader_plan.h"

int plan_str_demux(const StrDemuxCall& c, StrDemuxPlan* p) {
    const psxhip_str_settings_t* s = c.s;
    if (!s || !str_sector_geometry(s->format, &p->sector_size, &p->sub_at, &p->hdr_at)) {
        psxhip_set_error("psxhip_str_demux_device: NULL settings, or a format that is none of 6 (STR), 7 (STRCD), 9 (STRV); format 8 (STRSPU) is "
                         "psxhip_strspu_demux_device's");
        return PSXHIP_EINVAL;
    }
    if (c.n_streams < 1 || c.n_streams > 65535 || c.n_sectors < 0 || c.max_frames < 0 || c.xa_capacity < 0 || c.first_frame < -1 ||
        c.first_frame > 0xFFFFFFFFll || !c.d_summary || (c.n_sectors > 0 && !c.d_sectors) ||
        (c.max_frames > 0 && (!c.d_bs || !c.d_bs_sizes || !c.d_frame_info)) || (c.xa_capacity > 0 && !c.d_xa)) {
        psxhip_set_error("psxhip_str_demux_device: NULL argument, or a count or first_frame out of range");
        return PSXHIP_EINVAL;
    }
    if (misaligned(c.d_sectors) || misaligned(c.d_bs) || misaligned(c.d_bs_sizes) || misaligned(c.d_frame_info) || misaligned(c.d_xa) ||
        misaligned(c.d_sector_table) || misaligned(c.d_summary) || (c.in_stream_stride & 3) || (c.bs_stride & 3) || (c.bs_stream_stride & 3) ||
        (c.xa_stream_stride & 3) || c.bs_stride < 2016) {
        psxhip_set_error("psxhip_str_demux_device: pointers and strides must be 4-byte aligned, bs_stride at least 2016");
        return PSXHIP_EINVAL;
    }
    const size_t ssz = (size_t)p->sector_size;
    if (c.n_streams > 1 && (c.in_stream_stride < ssz * (size_t)c.n_sectors || c.bs_stream_stride < c.bs_stride * (size_t)c.max_frames ||
                            c.xa_stream_stride < ssz * (size_t)c.xa_capacity)) {
        psxhip_set_error("psxhip_str_demux_device: a stream stride smaller than a stream");
        return PSXHIP_EINVAL;
    }
    const size_t cap = c.bs_stride / 2016 < 65536 ? c.bs_stride / 2016 : 65536;      // chunk_index is 16 bits wide
    const size_t S = (size_t)c.n_streams, n = (size_t)c.n_sectors, rows = S * (size_t)c.max_frames;
    const size_t n_blocks = (n + kStrDemuxScanBlock - 1) / kStrDemuxScanBlock;
    p->chunk_cap = (int)cap;
    p->n_blocks = (int)n_blocks;
    BumpOffsets o;
    p->o_rec = o.take(S * n * 16);
    p->o_table = o.take(S * n * sizeof(psxhip_str_sector_t));
    p->o_blocks = o.take(S * n_blocks * 4);
    p->o_owner = o.take(rows * cap * 4 + rows * 4 + S * 4);       // d_owner, d_lead and d_min back to back (one fill with ones)
    p->o_lead = p->o_owner + rows * cap * 4;
    p->o_min = p->o_lead + rows * 4;
    p->o_status = o.take(rows * 4);
    p->ws_bytes = o.end;
    return PSXHIP_OK;
}

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

psxhip_str_settings_t strv_settings_of(const psxhip_str_settings_t* s) {
    psxhip_str_settings_t v = *s;
    v.format = FORMAT_STRV;
    v.audio_channels = 0;
    return v;
}

int plan_strspu_demux(const psxhip_str_settings_t* s, int n_streams, uintptr_t d_units, int audio_capacity, size_t units_stream_stride,
                      uintptr_t d_chunk_info, uintptr_t d_audio_summary, StrspuDemuxPlan* p) {
    if (const char* why = strspu_reader_settings_error(s)) {
        psxhip_set_error("psxhip_strspu_demux_device: %s", why);
        return PSXHIP_EINVAL;
    }
    if (n_streams < 1 || n_streams > 65535 || audio_capacity < 0 || audio_capacity > kStrspuMaxChunks || !d_audio_summary ||
        (audio_capacity > 0 && (!d_units || !d_chunk_info))) {
        psxhip_set_error("psxhip_strspu_demux_device: NULL argument, or audio_capacity outside 0 .. (2^31 - 1) / 126");
        return PSXHIP_EINVAL;
    }
    if ((d_units & 15) || (units_stream_stride & 15) || misaligned(d_chunk_info) || misaligned(d_audio_summary)) {
        psxhip_set_error("psxhip_strspu_demux_device: d_units and units_stream_stride must be 16-byte aligned, the records 4-byte aligned");
        return PSXHIP_EINVAL;
    }
    if (n_streams > 1 && units_stream_stride < (size_t)audio_capacity * 126 * 16) {
        psxhip_set_error("psxhip_strspu_demux_device: a stream stride smaller than a stream");
        return PSXHIP_EINVAL;
    }
    p->rules.ch = s->audio_channels;
    p->rules.id = (uint32_t)s->strspu_options & PSXHIP_STRSPU_ID_MASK;
    p->rules.d = strspu_dummy_of((uint32_t)s->strspu_options);
    p->rules.loop = ((uint32_t)s->strspu_options & PSXHIP_STRSPU_LOOP) != 0;
    p->rules.frequency = (uint32_t)s->audio_frequency;
    p->words = (size_t)n_streams * (size_t)audio_capacity;
    p->ws_bytes = 2 * p->words * sizeof(uint32_t);
    return PSXHIP_OK;
}

int plan_spu_deinterleave(uintptr_t d_in, int n_chunks, size_t chunk_stride, size_t lane_offset, size_t lane_bytes, int channels,
                          uintptr_t d_src_chunk, int n_streams, size_t in_stream_stride, uintptr_t d_units, size_t units_stream_stride,
                          SpuDeinterleavePlan* p) {
    if (n_chunks < 0 || n_streams < 1 || n_streams > 65535 || channels < 1 || lane_bytes == 0 || (lane_bytes & 15) ||
        (n_chunks > 0 && (!d_in || !d_units))) {
        psxhip_set_error("psxhip_spu_deinterleave_device: NULL argument, a count out of range, or lane_bytes no positive multiple of 16");
        return PSXHIP_EINVAL;
    }
    if (misaligned(d_in) || misaligned(d_src_chunk) || (chunk_stride & 3) || (lane_offset & 3) || (in_stream_stride & 3) || (d_units & 15) ||
        (units_stream_stride & 15)) {
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
    p->blocks = blocks;
    p->records = records;
    p->vec16 = ((d_in + lane_offset) & 15) == 0 && (chunk_stride & 15) == 0 && (n_streams == 1 || (in_stream_stride & 15) == 0);
    return PSXHIP_OK;
}

size_t xa_read_capacity(const XaLayout& xa, bool audible, int64_t pcm_capacity, size_t n) {
    if (!audible) return 0;
    const size_t held = (size_t)pcm_capacity / (size_t)xa.samples_per_sector;
    return held < n ? held : n;
}

size_t strspu_read_capacity(int ch, int d, bool pcm, int64_t pcm_capacity, size_t n) {
    if (!pcm || !ch) return 0;
    const int64_t held = (pcm_capacity / (28 * ch) + d) / (126 / ch);
    size_t cap = (size_t)held < n ? (size_t)held : n;
    if (cap > (size_t)kStrspuMaxChunks / 28) cap = (size_t)kStrspuMaxChunks / 28;
    return cap;
}

void strspu_read_chains(psxhip_adpcm_chain_t* chains, int32_t* unit_base, int ch, int d, int n_units) {
    for (int c = 0; c < ch; c++) {
        chains[c].sample_offset = c;
        chains[c].pitch = ch;
        chains[c].sample_limit = 28 * n_units;
        chains[c].n_units = n_units;
        chains[c].unit_stride = ch;
        unit_base[c] = d * ch + c;
    }
}

int plan_read_host(bool spu, const ReadHostCall& c, ReadHostPlan* p) {
    const char* const who = spu ? "psxhip_strspu_read_host" : "psxhip_str_read_host";
    const psxhip_str_settings_t* s = c.s;
    *p = ReadHostPlan();
    p->spu = spu;
    int sub_at = -1, hdr_at = 0;
    if (spu) {
        if (const char* why = strspu_reader_settings_error(s)) {
            psxhip_set_error("%s: %s", who, why);
            return PSXHIP_EINVAL;
        }
        p->sector_size = 2048;
    } else if (!s || !str_sector_geometry(s->format, &p->sector_size, &sub_at, &hdr_at)) {
        psxhip_set_error("psxhip_str_read_host: NULL settings, or a format that is none of 6 (STR), 7 (STRCD), 9 (STRV); format 8 (STRSPU) is "
                         "psxhip_strspu_read_host's");
        return PSXHIP_EINVAL;
    }
    const int ch = s->audio_channels, bits = s->audio_bit_depth;
    // the audio settings a stream of the call's kind can have (STRSPU: the channels are strspu_reader_settings_error's)
    const bool bad_audio = spu ? s->audio_frequency < 0
                               : ch < 0 || ch > 2 || (ch && ((s->audio_frequency != 18900 && s->audio_frequency != 37800) || (bits != 4 && bits != 8)));
    if (c.n_sectors < 0 || c.max_frames < 0 || c.pcm_capacity < 0 || !c.summary || (c.n_sectors > 0 && !c.sectors) ||
        (c.max_frames > 0 && (!c.frame_info || !c.decoded)) || s->video_codec < 0 || s->video_codec > 2 || s->str_fps_num <= 0 ||
        s->str_fps_den <= 0 || (s->str_cd_speed != 1 && s->str_cd_speed != 2) || bad_audio) {
        psxhip_set_error("%s: NULL argument, a negative count, or settings no stream can have", who);
        return PSXHIP_EINVAL;
    }
    // the widest frame the rate allows: the budgets of mdec.c:768-775 never pass ceil(base / den) chunks (filefmt.c:399-403,431-432); an
    // STRSPU stream's budgets (section 15) never pass those of the stream without audio
    const psxhip_str_settings_t v = spu ? strv_settings_of(s) : *s;
    const StrRates rates = str_rates(&v);
    const long long chunks = (long long)((rates.base + rates.den - 1) / rates.den);
    if (chunks < 1 || chunks > 65536) {
        psxhip_set_error("%s: the frame rate and CD speed give a frame %lld chunks", who, chunks);
        return PSXHIP_EINVAL;
    }
    p->chunks = (int)chunks;
    p->bs_stride = (size_t)chunks * 2016;
    p->frame_bytes = (size_t)s->video_width * s->video_height * 3 / 2;
    p->dec_key[0] = s->video_width;
    p->dec_key[1] = s->video_height;
    p->dec_key[2] = s->video_codec == 2;
    p->ch = ch;
    const size_t ssz = (size_t)p->sector_size, n = p->n = (size_t)c.n_sectors, mf = p->mf = (size_t)c.max_frames;
    if (spu) {
        p->d = strspu_dummy_of((uint32_t)s->strspu_options);
        p->B = ch ? 126 / ch : 0;
        p->audio_cap = strspu_read_capacity(ch, p->d, c.pcm, c.pcm_capacity, n);
        p->unit_item = 126 * 16;
        p->info_item = sizeof(psxhip_strspu_chunk_info_t);
        p->pcm_item = 126 * 28 * 2;
    } else {
        p->xa = xa_layout(s->format == 7 ? 1 : 0, ch == 2, bits);
        p->audio_cap = xa_read_capacity(p->xa, c.pcm && ch && sub_at >= 0, c.pcm_capacity, n);
        p->src_item = ssz;
        p->unit_item = (size_t)p->xa.units_per_sector * p->xa.record_bytes;
        p->info_item = 4;
        p->pcm_item = (size_t)p->xa.samples_per_sector * 2;
    }
    const size_t cap = p->audio_cap;
    BumpOffsets o;
    p->o_sec = o.take(n * ssz);
    p->o_bs = o.take(mf * p->bs_stride);
    p->o_sizes = o.take(mf * 4);
    p->o_info = o.take(mf * sizeof(psxhip_str_frame_info_t));
    p->o_dec = o.take(mf * sizeof(psxhip_mdec_decoded_t));
    p->o_sum = o.take(sizeof(psxhip_str_summary_t) + sizeof(psxhip_strspu_audio_summary_t));
    p->o_asum = p->o_sum + sizeof(psxhip_str_summary_t);
    p->o_src = o.take(cap * p->src_item);
    p->o_units = o.take(cap * p->unit_item);
    p->o_ainfo = o.take(cap * p->info_item);
    p->o_states = o.take(sizeof(psxhip_adpcm_state_t) * 2);
    p->o_pcm = o.take(cap * p->pcm_item);
    p->o_px = o.end;
    p->reserve = p->o_px + (c.frames ? mf * p->frame_bytes : 0) + 256;
    return PSXHIP_OK;
}
