// psxhip_spu_bank.cpp -- the sound bank's entry points (include/psxav_hip.h, psxhip_spu_bank_*; "psxhip SPU bank v1", DESIGN.md
// section 23).  What a bank refuses, where its files lie, its rows, chain table and tiles are spu_bank_plan.cpp's, without HIP; here
// are the context, which owns the plan and its device tables, and the HIP calls in their order: the ADPCM encoder (or decoder) of
// the library under the plan's chain table over the bank in place, then the framing kernels (spu_bank_kernels.hip).  No encoding
// and no framing happens on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "device_buffer.h"
#include "adpcm_plan.h"
#include "psxhip_internal.h"
#include "psxhip_spu_bank_internal.h"
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
    rc = b->tables.reserve(o.end);
    if (rc) return rc;
    uint8_t* d = b->tables.as<uint8_t>();
    b->d_chains = (psxhip_adpcm_chain_t*)(d + o_chains);
    b->d_base = (int32_t*)(d + o_base);
    b->d_states = (psxhip_adpcm_state_t*)(d + o_states);
    b->d_rows = (psxhip_spu_bank_row_t*)(d + o_rows);
    b->d_tiles = (psxhip_spu_bank_tile_t*)(d + o_tiles);
    b->d_tails = (int16_t*)(d + o_tails);
    HIP_TRY(hipMemset(d, 0, o.end), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpy(b->d_chains, p.chains.data(), sizeof(psxhip_adpcm_chain_t) * N, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpy(b->d_base, p.unit_base.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpy(b->d_rows, p.rows.data(), sizeof(psxhip_spu_bank_row_t) * N, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
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

extern "C" int psxhip_spu_bank_encode_device(psxhip_spu_bank_t* b, const int16_t* d_pcm, uint8_t* d_out, void* stream) {
    if (!b || (b->plan.total > 0 && !d_out) || ((uintptr_t)d_out & 15) || (b->plan.total_units > 0 && !d_pcm) || ((uintptr_t)d_pcm & 1)) {
        psxhip_set_error("psxhip_spu_bank_encode_device: NULL bank, PCM or output, or a misaligned pointer (d_out 16 bytes, d_pcm 2)");
        return PSXHIP_EINVAL;
    }
    const SpuBankPlan& p = b->plan;
    if (p.total == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(b->device), PSXHIP_EDEVICE);
    hipStream_t st = (hipStream_t)stream;
    if (p.total_units > 0) {
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
