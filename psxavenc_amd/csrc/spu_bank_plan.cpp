// spu_bank_plan.cpp -- the sound bank's plan (spu_bank_plan.h): refusals, file offsets and sizes, the kernels' rows, the chain table,
// the check kernel's tiles, the serial / chunked decision.  No HIP; the one symbol it links against is psxhip_set_error.
#include "spu_bank_plan.h"

#include <string.h>

#include "spu_file_layout.h"

extern "C" void psxhip_set_error(const char* fmt, ...);          // (psxhip_api.cpp; psxhip_internal.h declares it beside HIP)

psxhip_spu_file_settings_t spu_bank_file_settings(const psxhip_spu_bank_settings_t* s, const psxhip_spu_bank_entry_t* e) {
    psxhip_spu_file_settings_t f;
    memset(&f, 0, sizeof f);
    f.format = s->format;
    f.audio_frequency = e->audio_frequency;
    f.audio_channels = 1;
    f.audio_interleave = 0;
    f.alignment = s->alignment;
    f.audio_loop_point = e->audio_loop_point;
    f.enable_loop = e->enable_loop;
    f.no_leading_dummy = s->no_leading_dummy;
    memcpy(f.name, e->name, sizeof f.name);
    return f;
}

int64_t spu_bank_seam_block(const psxhip_spu_file_settings_t* f, int64_t data_blocks) {
    if (!f->enable_loop || data_blocks <= 0) return -1;
    const int64_t start = spu_loop_start_data_block(f, data_blocks);
    if (start >= 0) return start;
    return f->no_leading_dummy ? 0 : -1;        // key-on sets the repeat address to the start address: block 0, or the dummy block
}

// units [first, first + count) of entry chain c as a chain of their own
static psxhip_adpcm_chain_t chain_part(const psxhip_adpcm_chain_t& c, int64_t first, int64_t count) {
    psxhip_adpcm_chain_t part = c;
    part.sample_offset = c.sample_offset + first * kSpuBlockSamples;
    const int64_t limit = (int64_t)c.sample_limit - first * kSpuBlockSamples;
    part.sample_limit = (int32_t)(limit > 0 ? limit : 0);
    part.n_units = (int32_t)count;
    return part;
}

static int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

int spu_bank_plan_build(const psxhip_spu_bank_settings_t* s, const psxhip_spu_bank_entry_t* entries, int n, int chunked_threshold,
                        SpuBankPlan* p) {
    if (n < 1 || n > 65535) {
        psxhip_set_error("psxhip_spu_bank: %d entries (1 .. 65535)", n);
        return PSXHIP_EINVAL;
    }
    if (!s || !entries || !p) {
        psxhip_set_error("psxhip_spu_bank: NULL settings or entries");
        return PSXHIP_EINVAL;
    }
    if (s->format != FORMAT_SPU && s->format != FORMAT_VAG) {
        psxhip_set_error("psxhip_spu_bank: format %d (2 = SPU, 3 = VAG; interleaved files are not banked in this revision)", s->format);
        return PSXHIP_EINVAL;
    }
    if (s->alignment < 16 || s->alignment % 16) {
        psxhip_set_error("psxhip_spu_bank: alignment %d is no positive multiple of 16", s->alignment);
        return PSXHIP_EINVAL;
    }
    if (s->bank_alignment < 16 || s->bank_alignment > 65536 || s->bank_alignment % 16) {
        psxhip_set_error("psxhip_spu_bank: bank_alignment %d (a multiple of 16, 16 .. 65536)", s->bank_alignment);
        return PSXHIP_EINVAL;
    }
    if (s->beam < 0 || s->beam > PSXHIP_ADPCM_BEAM_MAX_WIDTH) {
        psxhip_set_error("psxhip_spu_bank: beam %d (0 .. 4)", s->beam);
        return PSXHIP_EINVAL;
    }
    for (int i = 0; i < n; i++) {
        const psxhip_spu_bank_entry_t& e = entries[i];
        if (e.samples < 0 || e.samples > 0x7FFFFFFF - kSpuBlockSamples) {
            psxhip_set_error("psxhip_spu_bank: entry %d has %lld samples (0 .. %d)", i, (long long)e.samples, 0x7FFFFFFF - kSpuBlockSamples);
            return PSXHIP_EINVAL;
        }
        if (e.audio_frequency <= 0) {
            psxhip_set_error("psxhip_spu_bank: entry %d has audio_frequency %d", i, e.audio_frequency);
            return PSXHIP_EINVAL;
        }
        if (e.pcm_offset < 0 || e.pcm_offset > INT64_MAX - e.samples) {
            psxhip_set_error("psxhip_spu_bank: entry %d has pcm_offset %lld", i, (long long)e.pcm_offset);
            return PSXHIP_EINVAL;
        }
    }

    *p = SpuBankPlan();
    p->settings = *s;
    p->n = n;
    p->offsets.resize((size_t)n);
    p->sizes.resize((size_t)n);
    std::vector<int64_t> data_blocks((size_t)n);
    int64_t at = 0;
    for (int i = 0; i < n; i++) {
        const psxhip_spu_file_settings_t f = spu_bank_file_settings(s, &entries[i]);
        int64_t count;
        p->offsets[(size_t)i] = at;
        p->sizes[(size_t)i] = spu_layout(&f, entries[i].samples, &data_blocks[(size_t)i], &count);
        // (n <= 65535 files of less than 2^33 bytes each: far inside 64 bits)
        at = round_up(at + p->sizes[(size_t)i], s->bank_alignment);
    }
    p->total = at;
    if (p->total / kSpuBlockBytes >= (int64_t)1 << 31) {
        psxhip_set_error("psxhip_spu_bank: the bank takes %lld bytes, %lld records of 16: record indices are int32", (long long)p->total,
                         (long long)(p->total / kSpuBlockBytes));
        return PSXHIP_EINVAL;
    }

    p->rows.resize((size_t)n);
    p->chains.resize((size_t)n);
    p->unit_base.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        const psxhip_spu_bank_entry_t& e = entries[i];
        const psxhip_spu_file_settings_t f = spu_bank_file_settings(s, &e);
        const int64_t blocks = data_blocks[(size_t)i];
        psxhip_spu_bank_row_t& r = p->rows[(size_t)i];
        memset(&r, 0, sizeof r);
        r.first_word = (int32_t)(p->offsets[(size_t)i] / kSpuBlockBytes);
        r.header_words = s->format == FORMAT_VAG ? kVagHeaderBytes / kSpuBlockBytes : 0;
        r.dummy = s->no_leading_dummy ? 0 : 1;
        r.data_blocks = (int32_t)blocks;
        r.trap = e.enable_loop ? 0 : 1;
        r.end_word = (int32_t)((i + 1 < n ? p->offsets[(size_t)i + 1] : p->total) / kSpuBlockBytes);
        r.loop_start_block = (int32_t)spu_loop_start_data_block(&f, blocks);
        r.loop_repeat = e.enable_loop && blocks ? 1 : 0;
        if (s->format == FORMAT_VAG) {
            uint8_t h[kVagHeaderBytes];
            vag_header(&f, (int)((r.dummy + blocks + r.trap) * kSpuBlockBytes), h);
            memcpy(r.header, h, sizeof h);
        }

        psxhip_adpcm_chain_t& c = p->chains[(size_t)i];
        c.sample_offset = e.pcm_offset;
        c.pitch = 1;
        c.sample_limit = (int32_t)e.samples;
        c.n_units = (int32_t)blocks;
        c.unit_stride = 1;
        p->unit_base[(size_t)i] = r.first_word + r.header_words + r.dummy;

        if (e.pcm_offset + e.samples > p->pcm_elements) p->pcm_elements = e.pcm_offset + e.samples;
        p->total_units += blocks;
        if (blocks > p->max_units) p->max_units = (int)blocks;

        const int64_t frame_words = spu_bank_frame_words(r);
        for (int64_t w = 0; w < frame_words; w += kSpuBankTile)
            p->tiles.push_back(psxhip_spu_bank_tile_t{i, 0, (int32_t)w, (int32_t)(frame_words - w < kSpuBankTile ? frame_words - w : kSpuBankTile)});
        for (int64_t b = 0; b < blocks; b += kSpuBankTile)
            p->tiles.push_back(psxhip_spu_bank_tile_t{i, 1, (int32_t)b, (int32_t)(blocks - b < kSpuBankTile ? blocks - b : kSpuBankTile)});
    }
    p->chunked = p->max_units >= chunked_threshold;

    // the seam tables
    p->seam_block.resize((size_t)n);
    p->seam_rows.resize((size_t)n);
    std::vector<int32_t> intro_slot((size_t)n, -1);
    for (int i = 0; i < n; i++) {
        const psxhip_spu_file_settings_t f = spu_bank_file_settings(s, &entries[i]);
        const int64_t S = spu_bank_seam_block(&f, data_blocks[(size_t)i]);
        p->seam_block[(size_t)i] = (int32_t)S;
        p->seam_rows[(size_t)i] = psxhip_spu_seam_row_t{entries[i].pcm_offset, (int32_t)entries[i].samples, p->unit_base[(size_t)i],
                                                        (int32_t)data_blocks[(size_t)i], (int32_t)S};
        if (S == 0) continue;
        intro_slot[(size_t)i] = (int32_t)p->seam_chains.size();
        p->seam_chains.push_back(S < 0 ? p->chains[(size_t)i] : chain_part(p->chains[(size_t)i], 0, S));
        p->seam_unit_base.push_back(p->unit_base[(size_t)i]);
    }
    p->seam_first = (int)p->seam_chains.size();
    for (int i = 0; i < n; i++) {
        const int64_t S = p->seam_block[(size_t)i];
        if (S < 0) continue;
        p->seam_chains.push_back(chain_part(p->chains[(size_t)i], S, data_blocks[(size_t)i] - S));
        p->seam_unit_base.push_back((int32_t)(p->unit_base[(size_t)i] + S));
        p->seam_body_entry.push_back(i);
        p->seam_body_intro.push_back(S > 0 ? intro_slot[(size_t)i] : -1);
    }
    p->seam_body = (int)p->seam_chains.size() - p->seam_first;
    return PSXHIP_OK;
}

extern "C" __attribute__((visibility("default"))) int psxhip_spu_bank_plan(const psxhip_spu_bank_settings_t* settings,
                                                                          const psxhip_spu_bank_entry_t* entries, int n, int64_t* offsets,
                                                                          int64_t* sizes, int64_t* total) {
    SpuBankPlan p;
    const int rc = spu_bank_plan_build(settings, entries, n, 0x7FFFFFFF, &p);      // (the layout does not depend on the threshold)
    if (rc) return rc;
    if (offsets) memcpy(offsets, p.offsets.data(), sizeof(int64_t) * (size_t)n);
    if (sizes) memcpy(sizes, p.sizes.data(), sizeof(int64_t) * (size_t)n);
    if (total) *total = p.total;
    return PSXHIP_OK;
}
