// psxhip_spu_bank.cpp -- the sound bank's entry points (include/psxav_hip.h, psxhip_spu_bank_*; "psxhip SPU bank v1", DESIGN.md
// section 23).  What a bank refuses, where its files lie, its rows, chain table and tiles are spu_bank_plan.cpp's, without HIP; here
// are the context, which owns the plan and its device tables, and the HIP calls in their order: the ADPCM encoder (or decoder) of
// the library under the plan's chain table over the bank in place, then the framing kernels (spu_bank_kernels.hip).  No encoding
// and no framing happens on the host.  "psxhip SPU loop seam v1"  is here too: mode STEADY's launches in their
// order, and the seam report (spu_seam_kernels.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "device_buffer.h"
#include "adpcm_plan.h"
#include "psxhip_internal.h"
#include "psxhip_spu_bank_internal.h"
#include "psxhip_spu_seam_internal.h"
#include "spu_bank_plan.h"

struct __attribute__((visibility("hidden"))) psxhip_spu_bank {      // (the handle is opaque: none of this is part of the library's surface)
    int device = 0;
    SpuBankPlan plan;
    DeviceBuffer tables;            // one block: chains, unit bases, states, rows, tiles, tails
    psxhip_adpcm_chain_t* d_chains = nullptr;
    int32_t* d_base = nullptr;
    psxhip_adpcm_state_t* d_states = nullptr;
    psxhip_spu_bank_row_t* d_rows = nullptr;
    psxhip_spu_bank_tile_t* d_tiles = nullptr;
    int16_t* d_tails = nullptr;     // [n][28] the decoder's, for the unit `samples` cuts
    psxhip_spu_seam_row_t* d_seam_rows = nullptr;       // [n] the seam report's
    // mode STEADY (psxhip_spu_bank_set_seam): the plan's seam chain table and what the step kernel keeps, in a block of their own
    int seam_mode = PSXHIP_SPU_SEAM_OFF;
    DeviceBuffer seam_tables;
    psxhip_adpcm_chain_t* d_seam_chains = nullptr;      // [seam_first + seam_body]; the body chains' n_units are the step kernel's
    int32_t* d_seam_base = nullptr;
    psxhip_adpcm_state_t* d_seam_states = nullptr;      // a slot per chain
    psxhip_adpcm_state_t* d_seam_start = nullptr;       // [seam_body] s_k
    int32_t *d_seam_intro = nullptr, *d_seam_entry = nullptr, *d_seam_units = nullptr;      // [seam_body]
    int32_t* d_seam_outcome = nullptr;                  // [n]
    // psxhip_spu_bank_encode_host's staging
    DeviceBuffer h_pcm, h_out;
    Stream h_stream;
};

extern "C" const char* psxhip_spu_bank_kernel_rev(void) { return PSXHIP_SPU_BANK_KERNEL_REV; }

extern "C" int psxhip_spu_bank_create(psxhip_spu_bank_t** out, int device, const psxhip_spu_bank_settings_t* settings,
                                      const psxhip_spu_bank_entry_t* entries, int n) {
    if (!out) {
        psxhip_set_error("psxhip_spu_bank_create: NULL handle pointer");
        return PSXHIP_EINVAL;
    }
    *out = nullptr;
    struct Guard {                       // frees the half-built context on every early return
        psxhip_spu_bank* p;
        ~Guard() { delete p; }
    } guard{new psxhip_spu_bank()};
    psxhip_spu_bank* b = guard.p;
    int rc = spu_bank_plan_build(settings, entries, n, adpcm_chunked_threshold(n), &b->plan);
    if (rc) return rc;
    rc = psxhip_ensure_device(device);
    if (rc) return rc;
    b->device = device;

    const SpuBankPlan& p = b->plan;
    const size_t N = (size_t)n, T = p.tiles.size();
    BumpOffsets o;
    const size_t o_chains = o.take(sizeof(psxhip_adpcm_chain_t) * N), o_base = o.take(sizeof(int32_t) * N);
    const size_t o_states = o.take(sizeof(psxhip_adpcm_state_t) * N), o_rows = o.take(sizeof(psxhip_spu_bank_row_t) * N);
    const size_t o_tiles = o.take(sizeof(psxhip_spu_bank_tile_t) * T), o_tails = o.take(sizeof(int16_t) * 28 * N);
    const size_t o_seam_rows = o.take(sizeof(psxhip_spu_seam_row_t) * N);
    rc = b->tables.reserve(o.end);
    if (rc) return rc;
    uint8_t* d = b->tables.as<uint8_t>();
    b->d_chains = (psxhip_adpcm_chain_t*)(d + o_chains);
    b->d_base = (int32_t*)(d + o_base);
    b->d_states = (psxhip_adpcm_state_t*)(d + o_states);
    b->d_rows = (psxhip_spu_bank_row_t*)(d + o_rows);
    b->d_tiles = (psxhip_spu_bank_tile_t*)(d + o_tiles);
    b->d_tails = (int16_t*)(d + o_tails);
    b->d_seam_rows = (psxhip_spu_seam_row_t*)(d + o_seam_rows);
    HIP_TRY(hipMemset(d, 0, o.end), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpy(b->d_chains, p.chains.data(), sizeof(psxhip_adpcm_chain_t) * N, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpy(b->d_base, p.unit_base.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpy(b->d_rows, p.rows.data(), sizeof(psxhip_spu_bank_row_t) * N, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpy(b->d_seam_rows, p.seam_rows.data(), sizeof(psxhip_spu_seam_row_t) * N, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    if (T) HIP_TRY(hipMemcpy(b->d_tiles, p.tiles.data(), sizeof(psxhip_spu_bank_tile_t) * T, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    HIP_TRY(hipDeviceSynchronize(), PSXHIP_EDEVICE);          // the tables are there for whatever stream the calls name
    guard.p = nullptr;
    *out = b;
    return PSXHIP_OK;
}

extern "C" void psxhip_spu_bank_destroy(psxhip_spu_bank_t* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();       // launches that read the tables may still run
    delete b;
}

extern "C" int64_t psxhip_spu_bank_total_bytes(const psxhip_spu_bank_t* b) {
    if (!b) {
        psxhip_set_error("psxhip_spu_bank_total_bytes: NULL bank");
        return PSXHIP_EINVAL;
    }
    return b->plan.total;
}

extern "C" int psxhip_spu_bank_layout(const psxhip_spu_bank_t* b, int64_t* offsets, int64_t* sizes) {
    if (!b) {
        psxhip_set_error("psxhip_spu_bank_layout: NULL bank");
        return PSXHIP_EINVAL;
    }
    if (offsets) memcpy(offsets, b->plan.offsets.data(), sizeof(int64_t) * (size_t)b->plan.n);
    if (sizes) memcpy(sizes, b->plan.sizes.data(), sizeof(int64_t) * (size_t)b->plan.n);
    return PSXHIP_OK;
}

// One launch of the bank's unit encoder over `count` chains of the seam table from chain `first` on: serial, on the stream
static int seam_encode(psxhip_spu_bank* b, const int16_t* d_pcm, uint8_t* d_out, int first, int count, hipStream_t st) {
    if (count == 0) return PSXHIP_OK;
    return psxhip_adpcm_encode_routed(b->device, d_pcm, nullptr, nullptr, b->d_seam_chains + first, b->d_seam_base + first, count, false, 0, 4, 5, 4,
                                      b->plan.settings.beam, b->d_seam_states + first, d_out, st);
}

// Mode STEADY: the intros and the entries without a seam block once from zero states, the step kernel arms the bodies with s_0, then
// P times (the bodies, the step), then the bodies once more: the step behind the last pass has re-armed those without a fixed point
// with s_0, which puts pass 0's blocks back.  A body the step retired has no units in the device table and is passed over.
static int encode_steady(psxhip_spu_bank* b, const int16_t* d_pcm, uint8_t* d_out, hipStream_t st) {
    const SpuBankPlan& p = b->plan;
    const int first = p.seam_first, body = p.seam_body;
    HIP_TRY(hipMemsetAsync(b->d_seam_states, 0, sizeof(psxhip_adpcm_state_t) * (size_t)(first + body), st), PSXHIP_EDEVICE);
    int rc = seam_encode(b, d_pcm, d_out, 0, first, st);
    if (rc || body == 0) return rc;
    psxhip_spu_seam_step_job_t job;
    job.chains = b->d_seam_chains + first;
    job.states = b->d_seam_states + first;
    job.first_states = b->d_seam_states;
    job.start = b->d_seam_start;
    job.body_intro = b->d_seam_intro;
    job.body_entry = b->d_seam_entry;
    job.body_units = b->d_seam_units;
    job.outcome = b->d_seam_outcome;
    job.n_body = body;
    job.passes = PSXHIP_SPU_SEAM_PASSES;
    for (int k = -1; k < PSXHIP_SPU_SEAM_PASSES; k++) {
        if (k >= 0 && (rc = seam_encode(b, d_pcm, d_out, first, body, st))) return rc;
        job.k = k;
        HIP_TRY(psxhip_spu_seam_step_launch(&job, st), PSXHIP_EDEVICE);
    }
    return seam_encode(b, d_pcm, d_out, first, body, st);
}

extern "C" int psxhip_spu_bank_encode_device(psxhip_spu_bank_t* b, const int16_t* d_pcm, uint8_t* d_out, void* stream) {
    if (!b || (b->plan.total > 0 && !d_out) || ((uintptr_t)d_out & 15) || (b->plan.total_units > 0 && !d_pcm) || ((uintptr_t)d_pcm & 1)) {
        psxhip_set_error("psxhip_spu_bank_encode_device: NULL bank, PCM or output, or a misaligned pointer (d_out 16 bytes, d_pcm 2)");
        return PSXHIP_EINVAL;
    }
    const SpuBankPlan& p = b->plan;
    if (p.total == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(b->device), PSXHIP_EDEVICE);
    hipStream_t st = (hipStream_t)stream;
    if (p.total_units > 0 && b->seam_mode == PSXHIP_SPU_SEAM_STEADY) {
        const int rc = encode_steady(b, d_pcm, d_out, st);
        if (rc) return rc;
    } else if (p.total_units > 0) {
        // every call starts every entry from a zero state; the records go straight into place (a 4-bit record is an SPU block with
        // byte 1 = 0, and unit_base[i] is entry i's first data block)
        HIP_TRY(hipMemsetAsync(b->d_states, 0, sizeof(psxhip_adpcm_state_t) * (size_t)p.n, st), PSXHIP_EDEVICE);
        const int rc = psxhip_adpcm_encode_routed(b->device, d_pcm, p.chains.data(), p.unit_base.data(), b->d_chains, b->d_base, p.n, p.chunked,
                                                  p.total_units, 4, 5, 4, p.settings.beam, b->d_states, d_out, st);
        if (rc) return rc;
    }
    psxhip_spu_bank_frame_job_t job;
    job.rows = b->d_rows;
    job.n_entries = p.n;
    job.out = d_out;
    HIP_TRY(psxhip_spu_bank_frame_launch(&job, st), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int64_t psxhip_spu_bank_encode_host(psxhip_spu_bank_t* b, const int16_t* pcm, int64_t pcm_elements, uint8_t* out, size_t out_size) {
    if (!b) {
        psxhip_set_error("psxhip_spu_bank_encode_host: NULL bank");
        return PSXHIP_EINVAL;
    }
    const SpuBankPlan& p = b->plan;
    if (pcm_elements < p.pcm_elements || (p.pcm_elements > 0 && !pcm)) {
        psxhip_set_error("psxhip_spu_bank_encode_host: the entries read %lld PCM elements, %lld given", (long long)p.pcm_elements, (long long)pcm_elements);
        return PSXHIP_EINVAL;
    }
    if ((p.total > 0 && !out) || (uint64_t)p.total > out_size) {
        psxhip_set_error("psxhip_spu_bank_encode_host: output needs %lld bytes, %zu given", (long long)p.total, out_size);
        return PSXHIP_EINVAL;
    }
    if (p.total == 0) return 0;
    HIP_TRY(hipSetDevice(b->device), PSXHIP_EDEVICE);
    int rc = b->h_stream.ensure();
    if (rc) return rc;
    const size_t pcm_bytes = sizeof(int16_t) * (size_t)p.pcm_elements;
    if ((rc = b->h_pcm.reserve(pcm_bytes + 16)) || (rc = b->h_out.reserve((size_t)p.total))) return rc;
    hipStream_t st = b->h_stream;
    if (pcm_bytes) HIP_TRY(hipMemcpyAsync(b->h_pcm.p, pcm, pcm_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    rc = psxhip_spu_bank_encode_device(b, b->h_pcm.as<int16_t>(), b->h_out.as<uint8_t>(), st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, b->h_out.p, (size_t)p.total, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return p.total;
}

extern "C" int psxhip_spu_bank_check_device(psxhip_spu_bank_t* b, const uint8_t* d_bank, int32_t* d_status, void* stream) {
    if (!b || !d_status || ((uintptr_t)d_status & 3) || (b->plan.total > 0 && !d_bank) || ((uintptr_t)d_bank & 15)) {
        psxhip_set_error("psxhip_spu_bank_check_device: NULL bank, buffer or status, or a misaligned pointer (d_bank 16 bytes, d_status 4)");
        return PSXHIP_EINVAL;
    }
    const SpuBankPlan& p = b->plan;
    HIP_TRY(hipSetDevice(b->device), PSXHIP_EDEVICE);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(int32_t) * (size_t)p.n, st), PSXHIP_EDEVICE);
    if (p.tiles.empty()) return PSXHIP_OK;
    psxhip_spu_bank_check_job_t job;
    job.rows = b->d_rows;
    job.tiles = b->d_tiles;
    job.n_tiles = (int)p.tiles.size();
    job.bank = d_bank;
    job.status = d_status;
    HIP_TRY(psxhip_spu_bank_check_launch(&job, st), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_spu_bank_decode_device(psxhip_spu_bank_t* b, const uint8_t* d_bank, int16_t* d_pcm_out, const int16_t* d_ref_pcm,
                                             uint64_t* d_entry_sums, void* stream) {
    if (!b || (b->plan.total_units > 0 && (!d_bank || !d_pcm_out)) || ((uintptr_t)d_bank & 15) || ((uintptr_t)d_pcm_out & 1) ||
        ((uintptr_t)d_ref_pcm & 1) || ((uintptr_t)d_entry_sums & 7) || (d_ref_pcm != nullptr) != (d_entry_sums != nullptr)) {
        psxhip_set_error("psxhip_spu_bank_decode_device: NULL bank, buffer or PCM, a misaligned pointer (d_bank 16 bytes, d_entry_sums 8, PCM 2), "
                         "or one of d_ref_pcm and d_entry_sums without the other");
        return PSXHIP_EINVAL;
    }
    const SpuBankPlan& p = b->plan;
    HIP_TRY(hipSetDevice(b->device), PSXHIP_EDEVICE);
    hipStream_t st = (hipStream_t)stream;
    if (p.total_units == 0) {           // nothing to decode: the sums of nothing
        if (d_entry_sums) HIP_TRY(hipMemsetAsync(d_entry_sums, 0, sizeof(uint64_t) * 2 * (size_t)p.n, st), PSXHIP_EDEVICE);
        return PSXHIP_OK;
    }
    HIP_TRY(hipMemsetAsync(b->d_states, 0, sizeof(psxhip_adpcm_state_t) * (size_t)p.n, st), PSXHIP_EDEVICE);
    int rc = psxhip_adpcm_decode_chains_device(b->device, d_bank, b->d_chains, b->d_base, p.n, 5, 4, b->d_states, d_pcm_out, nullptr, b->d_tails, st);
    if (rc) return rc;
    if (d_entry_sums)
        rc = psxhip_adpcm_sse_device(b->device, d_pcm_out, b->d_tails, d_ref_pcm, b->d_chains, p.n, nullptr, nullptr, d_entry_sums, st);
    return rc;
}

extern "C" const char* psxhip_spu_seam_kernel_rev(void) { return PSXHIP_SPU_SEAM_KERNEL_REV; }

extern "C" int psxhip_spu_bank_set_seam(psxhip_spu_bank_t* b, int mode) {
    if (!b) {
        psxhip_set_error("psxhip_spu_bank_set_seam: NULL bank");
        return PSXHIP_EINVAL;
    }
    if (mode != PSXHIP_SPU_SEAM_OFF && mode != PSXHIP_SPU_SEAM_STEADY) {
        psxhip_set_error("psxhip_spu_bank_set_seam: mode %d (0 = off, 1 = steady)", mode);
        return PSXHIP_EINVAL;
    }
    if (mode == PSXHIP_SPU_SEAM_STEADY && !b->seam_tables.p) {
        const SpuBankPlan& p = b->plan;
        const size_t M = p.seam_chains.size(), B = (size_t)p.seam_body, N = (size_t)p.n;
        HIP_TRY(hipSetDevice(b->device), PSXHIP_EDEVICE);
        BumpOffsets o;
        const size_t o_chains = o.take(sizeof(psxhip_adpcm_chain_t) * M), o_base = o.take(sizeof(int32_t) * M);
        const size_t o_states = o.take(sizeof(psxhip_adpcm_state_t) * M), o_start = o.take(sizeof(psxhip_adpcm_state_t) * B);
        const size_t o_intro = o.take(sizeof(int32_t) * B), o_entry = o.take(sizeof(int32_t) * B), o_units = o.take(sizeof(int32_t) * B);
        const size_t o_outcome = o.take(sizeof(int32_t) * N);
        DeviceBuffer block;
        int rc = block.reserve(o.end);
        if (rc) return rc;
        uint8_t* d = block.as<uint8_t>();
        std::vector<int32_t> units(B), outcome(N);
        for (size_t j = 0; j < B; j++) units[j] = p.seam_chains[(size_t)p.seam_first + j].n_units;
        for (size_t i = 0; i < N; i++) outcome[i] = p.seam_block[i] < 0 ? -1 : PSXHIP_SPU_SEAM_PASSES;
        HIP_TRY(hipMemset(d, 0, o.end), PSXHIP_EDEVICE);
        if (M) {
            HIP_TRY(hipMemcpy(d + o_chains, p.seam_chains.data(), sizeof(psxhip_adpcm_chain_t) * M, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
            HIP_TRY(hipMemcpy(d + o_base, p.seam_unit_base.data(), sizeof(int32_t) * M, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
        }
        if (B) {
            HIP_TRY(hipMemcpy(d + o_intro, p.seam_body_intro.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
            HIP_TRY(hipMemcpy(d + o_entry, p.seam_body_entry.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
            HIP_TRY(hipMemcpy(d + o_units, units.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
        }
        HIP_TRY(hipMemcpy(d + o_outcome, outcome.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
        HIP_TRY(hipDeviceSynchronize(), PSXHIP_EDEVICE);          // the tables are there for whatever stream the calls name
        b->seam_tables = std::move(block);
        b->d_seam_chains = (psxhip_adpcm_chain_t*)(d + o_chains);
        b->d_seam_base = (int32_t*)(d + o_base);
        b->d_seam_states = (psxhip_adpcm_state_t*)(d + o_states);
        b->d_seam_start = (psxhip_adpcm_state_t*)(d + o_start);
        b->d_seam_intro = (int32_t*)(d + o_intro);
        b->d_seam_entry = (int32_t*)(d + o_entry);
        b->d_seam_units = (int32_t*)(d + o_units);
        b->d_seam_outcome = (int32_t*)(d + o_outcome);
    }
    b->seam_mode = mode;
    return PSXHIP_OK;
}

extern "C" int psxhip_spu_bank_seam_passes_device(psxhip_spu_bank_t* b, int32_t* d_pass, void* stream) {
    if (!b || !d_pass || ((uintptr_t)d_pass & 3)) {
        psxhip_set_error("psxhip_spu_bank_seam_passes_device: NULL bank or d_pass, or a misaligned pointer (d_pass 4 bytes)");
        return PSXHIP_EINVAL;
    }
    if (b->seam_mode != PSXHIP_SPU_SEAM_STEADY) {
        psxhip_set_error("psxhip_spu_bank_seam_passes_device: the seam mode is off (psxhip_spu_bank_set_seam)");
        return PSXHIP_EINVAL;
    }
    HIP_TRY(hipSetDevice(b->device), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d_pass, b->d_seam_outcome, sizeof(int32_t) * (size_t)b->plan.n, hipMemcpyDeviceToDevice, (hipStream_t)stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_spu_bank_seam_device(psxhip_spu_bank_t* b, const uint8_t* d_bank, const int16_t* d_ref_pcm, psxhip_spu_seam_t* d_seam,
                                           void* stream) {
    if (!b || !d_seam || ((uintptr_t)d_seam & 7) || (b->plan.total > 0 && !d_bank) || ((uintptr_t)d_bank & 15) || ((uintptr_t)d_ref_pcm & 1)) {
        psxhip_set_error("psxhip_spu_bank_seam_device: NULL bank, buffer or d_seam, or a misaligned pointer (d_bank 16 bytes, d_seam 8, d_ref_pcm 2)");
        return PSXHIP_EINVAL;
    }
    HIP_TRY(hipSetDevice(b->device), PSXHIP_EDEVICE);
    psxhip_spu_seam_report_job_t job;
    job.rows = b->d_seam_rows;
    job.n_entries = b->plan.n;
    job.bank = d_bank;
    job.pcm = d_ref_pcm;
    job.seam = d_seam;
    HIP_TRY(psxhip_spu_seam_report_launch(&job, (hipStream_t)stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}
