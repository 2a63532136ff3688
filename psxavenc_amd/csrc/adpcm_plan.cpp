// adpcm_plan.cpp -- the ADPCM host layer's plans (adpcm_plan.h): every refusal of the encoder's and the decoder's entry points, the
// route, the chunk length, the chunk tables with their layouts and the shapes of the host-buffer encoders.  No HIP; the one symbol it
// links against is psxhip_set_error.
#include "adpcm_plan.h"

namespace {

bool bad_encode_coding(int filter_count, int bits) { return (filter_count != 4 && filter_count != 5) || (bits != 4 && bits != 8); }
// the decoder's: five filters are the SPU's, whose records hold 4-bit codes
bool bad_decode_coding(int filter_count, int bits) { return bad_encode_coding(filter_count, bits) || (bits == 8 && filter_count == 5); }
bool bad_beam(int beam) { return beam < 1 || beam > PSXHIP_ADPCM_BEAM_MAX_WIDTH; }
// a 4-bit record is stored and read back as one uint4 (store_spu_block, spu_pack_kernel, the sector kernels): 16 bytes, like the
// decoder's entry points ask for; an 8-bit record goes out in words
bool units_misaligned(uintptr_t d_units, int bits) { return (d_units & (bits == 4 ? 15 : 3)) != 0; }

size_t up8(size_t n) { return (n + 7) & ~(size_t)7; }

}  // namespace

// ---------------------------------------------------------------------------------------------- the coding rules
int adpcm_encode_chains_check(AdpcmChainsEntry who, uintptr_t d_samples, uintptr_t d_chains, uintptr_t d_unit_base, uintptr_t d_states,
                              uintptr_t d_units, int n_chains, int filter_count, int bits, int beam, uintptr_t d_unit_err) {
    const bool bad = !d_samples || !d_chains || !d_unit_base || !d_states || !d_units || n_chains < 0 || bad_encode_coding(filter_count, bits);
    if (who == kEncodeChains) {
        if (bad || units_misaligned(d_units, bits)) {
            psxhip_set_error("adpcm_encode_chains: bad argument (d_units 16-byte aligned for 4-bit records, 4-byte for 8-bit)");
            return PSXHIP_EINVAL;
        }
    } else if (bad || bad_beam(beam) || units_misaligned(d_units, bits) || (d_unit_err & 3)) {
        psxhip_set_error("adpcm_beam_encode_chains: bad argument (beam 1 .. 4; d_units 16-byte aligned for 4-bit records, 4-byte for 8-bit)");
        return PSXHIP_EINVAL;
    }
    return PSXHIP_OK;
}

int adpcm_session_create_check(uintptr_t d_samples, bool chains, bool unit_base, uintptr_t d_units, int n_chains, int filter_count, int bits,
                               int chunk_units, int warmup_units) {
    if (!d_samples || !chains || !unit_base || !d_units || n_chains < 0 || bad_encode_coding(filter_count, bits) || chunk_units < 1 ||
        warmup_units < 0 || units_misaligned(d_units, bits)) {
        psxhip_set_error("adpcm_session_create: bad argument (d_units 16-byte aligned for 4-bit records, 4-byte for 8-bit)");
        return PSXHIP_EINVAL;
    }
    return PSXHIP_OK;
}

int adpcm_session_beam_check(bool session, int beam, bool speculated) {
    if (!session || beam < 0 || beam > PSXHIP_ADPCM_BEAM_MAX_WIDTH || speculated) {
        psxhip_set_error("adpcm_session_set_beam: bad argument (beam 0 .. 4, before the first run or after a reset)");
        return PSXHIP_EINVAL;
    }
    return PSXHIP_OK;
}

int adpcm_encode_chunked_check(bool beam_entry, int beam, uintptr_t d_states) {
    if (beam_entry && bad_beam(beam)) {
        psxhip_set_error("adpcm_beam_encode_chains_chunked: bad argument (beam 1 .. 4)");
        return PSXHIP_EINVAL;
    }
    if (!d_states) {
        psxhip_set_error("adpcm_encode_chains_chunked: bad argument");
        return PSXHIP_EINVAL;
    }
    return PSXHIP_OK;
}

int adpcm_host_beam_check(const char* who, int beam) {
    if (!bad_beam(beam)) return PSXHIP_OK;
    psxhip_set_error("%s: bad argument (beam 1 .. 4)", who);
    return PSXHIP_EINVAL;
}

int spu_pack_check(uintptr_t d_units, int n_blocks, uintptr_t d_out) {
    if (!d_units || !d_out || n_blocks < 0 || (d_out & 15) || units_misaligned(d_units, 4)) {
        psxhip_set_error("spu_pack: bad argument (d_units and d_out must be 16-byte aligned)");
        return PSXHIP_EINVAL;
    }
    return PSXHIP_OK;
}

int xa_assemble_check(uintptr_t d_units, uintptr_t d_out, int n_sectors, int n_streams, int format, int bits, size_t units_stream_stride,
                      size_t out_stream_stride) {
    if (!d_units || !d_out || n_sectors < 0 || n_streams < 1 || n_streams > 65535 || (format != 0 && format != 1) || (bits != 4 && bits != 8) ||
        (d_out & 3) || (out_stream_stride & 3) || (units_stream_stride & 3)) {
        psxhip_set_error("xa_assemble: bad argument");
        return PSXHIP_EINVAL;
    }
    return PSXHIP_OK;
}

int adpcm_decode_chains_check(bool chunked, uintptr_t d_units, bool chains, bool unit_base, uintptr_t d_states, uintptr_t d_samples, uintptr_t d_tail,
                              int n_chains, int filter_count, int bits) {
    if (n_chains < 0 || bad_decode_coding(filter_count, bits) || (n_chains > 0 && (!d_units || !chains || !unit_base || !d_states || !d_samples)) ||
        (d_units & 15) || (d_samples & 1) || (d_tail & 3)) {
        psxhip_set_error("%s: bad argument (bits 4 or 8, filter_count 4 or 5 and 4 with 8 bits, d_units 16-byte aligned, d_tail 4-byte)",
                         chunked ? "adpcm_decode_chains_chunked" : "adpcm_decode_chains");
        return PSXHIP_EINVAL;
    }
    return PSXHIP_OK;
}

int adpcm_decode_chunked_chains_check(const psxhip_adpcm_chain_t* chains, int n_chains, long long* total_units) {
    *total_units = 0;
    for (int c = 0; c < n_chains; c++) {
        if (chains[c].pitch < 1 || chains[c].n_units < 0) {
            psxhip_set_error("adpcm_decode_chains_chunked: chain %d has pitch %d, n_units %d", c, chains[c].pitch, chains[c].n_units);
            return PSXHIP_EINVAL;
        }
        *total_units += chains[c].n_units;
    }
    return PSXHIP_OK;
}

int adpcm_sse_check(uintptr_t d_a, uintptr_t d_a_tail, uintptr_t d_b, uintptr_t d_chains, int n_chains, uintptr_t d_unit_sse, uintptr_t d_unit_base,
                    uintptr_t d_chain_sums) {
    if (n_chains < 0 || (n_chains > 0 && (!d_a || !d_b || !d_chains || (d_unit_sse && !d_unit_base))) || (d_a & 1) || (d_b & 1) || (d_a_tail & 1) ||
        (d_unit_sse & 7) || (d_chain_sums & 7)) {
        psxhip_set_error("adpcm_sse: NULL or misaligned argument, negative chain count, or d_unit_sse without d_unit_base");
        return PSXHIP_EINVAL;
    }
    return PSXHIP_OK;
}

int xa_disassemble_check(uintptr_t d_sectors, int n_sectors, int format, int bits, uintptr_t d_units, uintptr_t d_sector_status) {
    if (n_sectors < 0 || (format != 0 && format != 1) || (bits != 4 && bits != 8) || (n_sectors > 0 && (!d_sectors || !d_units)) ||
        (d_sectors & 3) || (d_units & 3) || (d_sector_status & 3)) {
        psxhip_set_error("xa_disassemble: bad argument (format 0 or 1, bits 4 or 8, pointers 4-byte aligned)");
        return PSXHIP_EINVAL;
    }
    return PSXHIP_OK;
}

// ---------------------------------------------------------------------------------------------- route
bool spu_call_fast_path(int beam, int n_streams, int n_units, size_t stage_max, size_t out_max) {
    return beam == 0 && n_streams <= 4 && !adpcm_route_chunked(n_units, n_streams) && (size_t)n_streams * ((size_t)n_units * 28 + 8) <= stage_max &&
           (size_t)n_streams * (size_t)n_units * 16 <= out_max;
}

bool xa_call_fast_path(int beam, int n_streams, int sectors, size_t per, size_t bytes, size_t stage_max, size_t out_max) {
    return beam == 0 && n_streams == 1 && sectors <= 6 && up8(per) <= stage_max && bytes <= out_max;
}

// ---------------------------------------------------------------------------------------------- chunking
AdpcmChunking adpcm_chunking(long long total_units, int rows, int n_cu) {
    const long long per_round = 32ll * n_cu * rows;                        // chunks in flight when every slot holds a wavefront
    const long long fill = (total_units + per_round - 1) / per_round;
    if (fill >= 1024) {
        const long long rounds = (fill + 4095) / 4096;
        return {(int)((total_units + per_round * rounds - 1) / (per_round * rounds)), 64};
    }
    const long long c = total_units / 8192;
    int p = 64;
    while (p * 2 <= c && p < 1024) p *= 2;
    return {p, p >= 1024 ? 32 : 16};     // noisy material converges within a few units, tonal material not within 1024 either
}

int adpcm_decode_chunking(long long total_units, int n_cu) {
    const int chunk_units = adpcm_chunking(total_units, 64, n_cu).chunk_units;
    const long long fill = total_units / (4ll * 8 * 64 * n_cu);
    const long long want = fill < 256 ? 256 : fill;
    return want < chunk_units ? (int)want : chunk_units;
}

// ---------------------------------------------------------------------------------------------- chunk tables and layouts
void adpcm_session_plan(const psxhip_adpcm_chain_t* chains, const int32_t* lead_units, int n_chains, int chunk_units, AdpcmSessionPlan* p) {
    const size_t nc = (size_t)n_chains;
    p->state_base.assign(nc, 0);
    p->lead.assign(nc, 0);
    p->chunk_chain.clear();
    p->chunk_first.clear();
    p->total_units = 0;
    for (int c = 0; c < n_chains; c++) {
        p->state_base[(size_t)c] = p->total_units;
        for (int f = 0; f < chains[c].n_units; f += chunk_units) {
            p->chunk_chain.push_back(c);
            p->chunk_first.push_back(f);
        }
        p->total_units += chains[c].n_units;
        if (lead_units) p->lead[(size_t)c] = lead_units[c] < 0 ? 0 : lead_units[c];
    }
    p->n_chunks = (int)p->chunk_chain.size();
    const size_t nk = (size_t)p->n_chunks, state = sizeof(psxhip_adpcm_state_t);
    BumpOffsets o;
    p->o_chains = o.take(sizeof(psxhip_adpcm_chain_t) * nc);
    p->o_base = o.take(sizeof(int32_t) * nc);
    p->o_sbase = o.take(sizeof(int64_t) * nc);
    p->o_lead = o.take(sizeof(int32_t) * nc);
    p->o_cstates = o.take(state * nc);
    p->o_final = o.take(state * nc);
    p->o_known = o.take(nc);
    p->o_flags = o.take(kAdpcmVerifyBatchMax * sizeof(int));
    p->o_cchain = o.take(sizeof(int32_t) * nk);
    p->o_cfirst = o.take(sizeof(int32_t) * nk);
    p->o_used = o.take(state * nk);
    p->o_ustates = o.take(state * (size_t)p->total_units);
    p->bytes = o.end;
}

int adpcm_decode_plan(const psxhip_adpcm_chain_t* chains, int n_chains, int chunk_units, AdpcmDecodePlan* p) {
    p->chunk_chain.clear();
    p->chunk_first.clear();
    p->chunk_pred.clear();
    p->last_chunk.assign((size_t)n_chains, -1);
    for (int c = 0; c < n_chains;) {
        const bool pair = c + 1 < n_chains && chains[c].pitch == 2 && chains[c + 1].pitch == 2 && chains[c].n_units > 0 &&
                          chains[c + 1].sample_offset == chains[c].sample_offset + 1 && chains[c + 1].n_units == chains[c].n_units;
        const int span = pair ? 2 : 1;
        for (int f = 0; f < chains[c].n_units; f += chunk_units)
            for (int k = 0; k < span; k++) {
                const int32_t idx = (int32_t)p->chunk_chain.size();
                p->last_chunk[(size_t)(c + k)] = idx;
                p->chunk_chain.push_back(c + k);
                p->chunk_first.push_back(f);
                p->chunk_pred.push_back(f ? idx - span : -1);
            }
        c += span;
    }
    p->n_chunks = p->chunk_chain.size();
    if (p->n_chunks > 0x7FFFFFFFu) {
        psxhip_set_error("adpcm_decode_chains_chunked: %zu chunks", p->n_chunks);
        return PSXHIP_EINVAL;
    }
    const size_t nc = (size_t)n_chains, nk = p->n_chunks;
    BumpOffsets o;
    p->o_chains = o.take(sizeof(psxhip_adpcm_chain_t) * nc);
    p->o_base = o.take(4 * nc);
    p->o_cc = o.take(4 * nk);
    p->o_cf = o.take(4 * nk);
    p->o_cp = o.take(4 * nk);
    p->o_last = o.take(4 * nc);
    p->o_used = o.take(8 * nk);
    p->o_end = o.take(8 * nk);
    p->o_flags = o.take(sizeof(int) * kAdpcmVerifyBatchMax);
    p->bytes = o.end;
    return PSXHIP_OK;
}

// ---------------------------------------------------------------------------------------------- the host-buffer encoders
namespace {
// one stream needs neither stride; more need room for a stream's bytes in the output
int encode_out_stride(const char* who, int n_streams, int bytes, int64_t* out_stride) {
    if (n_streams == 1) *out_stride = bytes;
    if (*out_stride >= bytes) return PSXHIP_OK;
    psxhip_set_error("%s: out_stride %lld < %d bytes per stream", who, (long long)*out_stride, bytes);
    return PSXHIP_EINVAL;
}
}  // namespace

int spu_encode_shape(bool buffers, int n_streams, int64_t stream_stride, int pitch, int samples_per_stream, int64_t out_stride, SpuEncodeShape* p) {
    if (!buffers || n_streams < 0 || samples_per_stream < 0 || pitch < 1) {
        psxhip_set_error("spu_encode_streams_host: bad argument");
        return PSXHIP_EINVAL;
    }
    *p = SpuEncodeShape();
    p->n_units = (samples_per_stream + 27) / 28;
    p->bytes = p->n_units * 16;
    p->empty = n_streams == 0 || p->n_units == 0;
    if (p->empty) return PSXHIP_OK;
    const int rc = encode_out_stride("spu_encode_streams_host", n_streams, p->bytes, &out_stride);
    if (rc) return rc;
    const size_t S = (size_t)n_streams;
    p->per = (size_t)samples_per_stream * pitch;
    p->readable = (size_t)(samples_per_stream - 1) * pitch + 1;
    p->row = up8((size_t)p->n_units * 28);
    p->stream_stride = n_streams == 1 ? (int64_t)p->readable : stream_stride;
    p->out_stride = out_stride;
    p->sample_bytes = p->per * S * sizeof(int16_t);
    p->chain_bytes = S * sizeof(psxhip_adpcm_chain_t);
    p->base_bytes = S * sizeof(int32_t);
    p->state_bytes = S * sizeof(psxhip_adpcm_state_t);
    p->unit_bytes = S * p->n_units * PSXHIP_ADPCM_RECORD_BYTES;
    p->out_bytes = S * p->bytes;
    return PSXHIP_OK;
}

int xa_encode_shape(bool buffers, int format, int stereo, int bits, int n_streams, int64_t stream_stride, int samples_per_stream, int64_t out_stride,
                    XaEncodeShape* p) {
    if (!buffers || n_streams < 0 || samples_per_stream < 0 || (bits != 4 && bits != 8) || (format != 0 && format != 1)) {
        psxhip_set_error("xa_encode_streams_host: bad argument");
        return PSXHIP_EINVAL;
    }
    *p = XaEncodeShape();
    const XaLayout& xa = p->xa = xa_layout(format, stereo, bits);
    const int group_samples = xa.units_per_group * 28;                      // interleaved samples consumed per group (adpcm.c:301)
    const int64_t total = (int64_t)samples_per_stream * xa.channels;        // adpcm.c:307-308
    p->groups = (int)((total + group_samples - 1) / group_samples);
    p->sectors = (p->groups + 17) / 18;                                     // the loop runs until the sector is complete (adpcm.c:310)
    p->bytes = p->sectors * xa.sector_bytes;
    p->empty = n_streams == 0 || p->sectors == 0;
    if (p->empty) return PSXHIP_OK;
    const int rc = encode_out_stride("xa_encode_streams_host", n_streams, p->bytes, &out_stride);
    if (rc) return rc;
    const size_t S = (size_t)n_streams;
    p->units_per_stream = p->sectors * xa.units_per_sector;
    p->units_per_chain = p->units_per_stream / xa.channels;
    p->per = (size_t)total;
    p->row = up8(p->per);
    p->stream_stride = n_streams == 1 ? (int64_t)p->per : stream_stride;
    p->out_stride = out_stride;
    p->n_chains = S * xa.channels;
    p->sample_bytes = p->per * S * sizeof(int16_t);
    p->chain_bytes = p->n_chains * sizeof(psxhip_adpcm_chain_t);
    p->base_bytes = p->n_chains * sizeof(int32_t);
    p->state_bytes = p->n_chains * sizeof(psxhip_adpcm_state_t);
    p->unit_bytes = S * p->units_per_stream * PSXHIP_ADPCM_RECORD_BYTES;
    p->out_bytes = S * p->bytes;
    p->eof_bytes = S * p->sectors;
    return PSXHIP_OK;
}

uint32_t xa_encode_eof_bits(int sectors, const uint8_t* eof_flags, int finalize) {
    uint32_t eof_bits = 0;
    for (int k = 0; k < sectors && k < 32; k++)
        if (eof_flags ? eof_flags[k] != 0 : (finalize && k == sectors - 1)) eof_bits |= 1u << k;
    return eof_bits;
}

std::vector<uint8_t> xa_encode_eof_table(int n_streams, int sectors, const uint8_t* eof_flags, int finalize) {
    std::vector<uint8_t> eof((size_t)n_streams * sectors, 0);
    if (eof_flags)
        eof.assign(eof_flags, eof_flags + eof.size());
    else if (finalize)
        for (int i = 0; i < n_streams; i++) eof[(size_t)i * sectors + sectors - 1] = 1;
    return eof;
}
