// psxhip_disc.cpp -- host side of the disc finisher (psxhip_disc_plan, psxhip_disc_finish_device, psxhip_disc_check_device,
// psxhip_disc_finish_host; include/psxav_hip.h): argument checks, the job structs, the launches
// (disc_kernels.hip).  No sector byte is computed on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "device_buffer.h"
#include "host_layout.h"
#include "psxhip_disc_internal.h"
#include "psxhip_internal.h"

namespace {

// the layout and the sources against the rules that need no pointer; fills the per-slot ranks and per-source slot counts and returns
// the sectors of the whole schedule, or PSXHIP_EINVAL with the text set
int64_t plan(const char* who, const psxhip_disc_layout_t* L, const psxhip_disc_source_t* src, int n_sources, int* count, uint8_t* rank) {
    if (!L || n_sources < 0 || n_sources > PSXHIP_DISC_MAX_SOURCES || (n_sources > 0 && !src)) {
        psxhip_set_error("%s: NULL layout or sources, or more than %d sources", who, PSXHIP_DISC_MAX_SOURCES);
        return PSXHIP_EINVAL;
    }
    if (L->period < 1 || L->period > PSXHIP_DISC_MAX_PERIOD) {
        psxhip_set_error("%s: period %d is not in 1 .. %d", who, L->period, PSXHIP_DISC_MAX_PERIOD);
        return PSXHIP_EINVAL;
    }
    for (int s = 0; s < PSXHIP_DISC_MAX_SOURCES; s++) count[s] = 0;
    for (int q = 0; q < L->period; q++) {
        const int s = L->slot_source[q];
        if (s < -1 || s >= n_sources) {
            psxhip_set_error("%s: slot %d names source %d of %d", who, q, s, n_sources);
            return PSXHIP_EINVAL;
        }
        rank[q] = s >= 0 ? (uint8_t)count[s]++ : 0;
    }
    int64_t rounds = 0;
    for (int s = 0; s < n_sources; s++) {
        const psxhip_disc_source_t& S = src[s];
        if ((S.sector_size != 2352 && S.sector_size != 2336 && S.sector_size != 2048) || S.n_sectors < 0 || (S.stride & 3) ||
            S.stride < S.sector_size || S.file_number < -1 || S.file_number > 255 || S.channel_number < -1 || S.channel_number > 31) {
            psxhip_set_error("%s: source %d: sector_size 2352 / 2336 / 2048, n_sectors >= 0, stride a multiple of 4 and >= sector_size, "
                             "file_number -1 .. 255, channel_number -1 .. 31", who, s);
            return PSXHIP_EINVAL;
        }
        if (S.sector_size == 2048 && (S.data_subheader[2] & 0x20)) {
            psxhip_set_error("%s: source %d: a 2048-byte source is never form 2 (data_subheader has bit 0x20)", who, s);
            return PSXHIP_EINVAL;
        }
        if (S.n_sectors > 0 && count[s] == 0) {
            psxhip_set_error("%s: source %d has sectors and owns no slot", who, s);
            return PSXHIP_EINVAL;
        }
        if (S.n_sectors > 0) {
            const int64_t r = ((int64_t)S.n_sectors + count[s] - 1) / count[s];
            if (r > rounds) rounds = r;
        }
    }
    return rounds * L->period;
}

int launch_grid(int64_t n_sectors) { return (int)((n_sectors + PSXHIP_DISC_SECTORS_PER_GROUP - 1) / PSXHIP_DISC_SECTORS_PER_GROUP); }

}  // namespace

extern "C" const char* psxhip_disc_kernel_rev(void) { return PSXHIP_DISC_KERNEL_REV; }

extern "C" int64_t psxhip_disc_plan(const psxhip_disc_layout_t* layout, const psxhip_disc_source_t* sources, int n_sources) {
    int count[PSXHIP_DISC_MAX_SOURCES];
    uint8_t rank[PSXHIP_DISC_MAX_PERIOD];
    return plan("psxhip_disc_plan", layout, sources, n_sources, count, rank);
}

extern "C" int psxhip_disc_finish_device(int device, const psxhip_disc_layout_t* layout, const psxhip_disc_source_t* sources, int n_sources,
                                         uint8_t* d_out, int64_t first_out, int64_t n_out, void* stream) {
    static const char who[] = "psxhip_disc_finish_device";
    psxhip_disc_finish_job_t j;
    memset(&j, 0, sizeof j);
    int count[PSXHIP_DISC_MAX_SOURCES];
    const int64_t total = plan(who, layout, sources, n_sources, count, j.slot_rank);
    if (total < 0) return PSXHIP_EINVAL;
    if (first_out < 0 || n_out < 0 || (n_out > 0 && !d_out) || misaligned(d_out) || layout->start_lba < 0 ||
        first_out > PSXHIP_DISC_LBA_LIMIT || n_out > PSXHIP_DISC_LBA_LIMIT ||
        (n_out > 0 && (int64_t)layout->start_lba + first_out + n_out - 1 + 150 >= PSXHIP_DISC_LBA_LIMIT)) {
        psxhip_set_error("%s: d_out NULL or not 4-byte aligned, a negative start_lba, first_out or n_out, or a last sector with "
                         "lba + 150 >= %d", who, PSXHIP_DISC_LBA_LIMIT);
        return PSXHIP_EINVAL;
    }
    const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (size_t)n_out * 2352;
    for (int s = 0; s < n_sources; s++) {
        const psxhip_disc_source_t& S = sources[s];
        if (S.n_sectors == 0) continue;
        if (!S.sectors || misaligned(S.sectors)) {
            psxhip_set_error("%s: source %d: sectors NULL or not 4-byte aligned", who, s);
            return PSXHIP_EINVAL;
        }
        const uintptr_t s0 = (uintptr_t)S.sectors, s1 = s0 + (size_t)(S.n_sectors - 1) * (size_t)S.stride + (size_t)S.sector_size;
        if (n_out > 0 && s0 < o1 && o0 < s1) {
            psxhip_set_error("%s: d_out overlaps source %d", who, s);
            return PSXHIP_EINVAL;
        }
    }
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_out == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    const int rt = psxhip_disc_tables(device);
    if (rt) return rt;
    for (int s = 0; s < n_sources; s++) {
        const psxhip_disc_source_t& S = sources[s];
        psxhip_disc_dev_source_t& D = j.src[s];
        D.base = S.sectors;
        D.stride = S.stride;
        D.n_sectors = S.n_sectors;
        D.lead = S.sector_size == 2048 ? 24 : 2352 - S.sector_size;
        D.count = count[s];
        D.file = (int16_t)S.file_number;
        D.channel = (int16_t)S.channel_number;
        D.has_subheader = S.sector_size != 2048;
        D.data_subheader = (uint32_t)S.data_subheader[0] | (uint32_t)S.data_subheader[1] << 8 | (uint32_t)S.data_subheader[2] << 16 |
                           (uint32_t)S.data_subheader[3] << 24;
    }
    for (int q = 0; q < layout->period; q++) j.slot_source[q] = (int8_t)layout->slot_source[q];
    j.period = layout->period;
    j.start_lba = layout->start_lba;
    j.first_out = first_out;
    j.n_out = n_out;
    j.out = d_out;
    HIP_TRY(psxhip_disc_finish_launch(&j, launch_grid(n_out), stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_disc_check_device(int device, const uint8_t* d_image, int64_t n_sectors, int64_t start_lba, int32_t* d_status,
                                        psxhip_disc_summary_t* d_summary, void* stream) {
    if (n_sectors < 0 || n_sectors > 0x7FFFFFFFll || (n_sectors > 0 && !d_image) || !d_summary || misaligned(d_image) ||
        misaligned(d_status) || misaligned(d_summary) || start_lba < -1 || start_lba > PSXHIP_DISC_LBA_LIMIT ||
        (start_lba >= 0 && n_sectors > 0 && start_lba + n_sectors - 1 + 150 >= PSXHIP_DISC_LBA_LIMIT)) {
        psxhip_set_error("psxhip_disc_check_device: NULL or misaligned pointer, a negative count, start_lba below -1, or a last sector "
                         "with lba + 150 >= %d", PSXHIP_DISC_LBA_LIMIT);
        return PSXHIP_EINVAL;
    }
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    HIP_TRY(hipMemsetAsync(d_summary, 0, sizeof *d_summary, (hipStream_t)stream), PSXHIP_EDEVICE);
    if (n_sectors == 0) return PSXHIP_OK;
    const int rt = psxhip_disc_tables(device);
    if (rt) return rt;
    psxhip_disc_check_job_t j;
    j.image = d_image;
    j.n_sectors = n_sectors;
    j.start_lba = start_lba;
    j.status = d_status;
    j.summary = d_summary;
    HIP_TRY(psxhip_disc_check_launch(&j, launch_grid(n_sectors), stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_disc_finish_host(int device, const psxhip_disc_layout_t* layout, const psxhip_disc_source_t* sources, int n_sources,
                                       uint8_t* out, int64_t first_out, int64_t n_out) {
    static const char who[] = "psxhip_disc_finish_host";
    int count[PSXHIP_DISC_MAX_SOURCES];
    uint8_t rank[PSXHIP_DISC_MAX_PERIOD];
    if (plan(who, layout, sources, n_sources, count, rank) < 0) return PSXHIP_EINVAL;
    if (n_out < 0 || n_out > PSXHIP_DISC_LBA_LIMIT || (n_out > 0 && !out)) {
        psxhip_set_error("%s: out NULL, or n_out negative or past %d", who, PSXHIP_DISC_LBA_LIMIT);
        return PSXHIP_EINVAL;
    }
    for (int s = 0; s < n_sources; s++)
        if (sources[s].n_sectors > 0 && !sources[s].sectors) {
            psxhip_set_error("%s: source %d: sectors NULL", who, s);
            return PSXHIP_EINVAL;
        }
    // the sources densely behind the image in one block: the device call checks the rest
    psxhip_disc_source_t dev[PSXHIP_DISC_MAX_SOURCES];
    BumpOffsets o;
    const size_t o_out = o.take((size_t)n_out * 2352 + 4);
    size_t at[PSXHIP_DISC_MAX_SOURCES];
    for (int s = 0; s < n_sources; s++) at[s] = o.take((size_t)sources[s].n_sectors * (size_t)sources[s].sector_size + 4);
    if (psxhip_device_count() <= 0) {
        // argument errors come first, also without a device: the device call's checks on dummy addresses
        for (int s = 0; s < n_sources; s++) {
            dev[s] = sources[s];
            dev[s].sectors = (const uint8_t*)(uintptr_t)(0x10000 + at[s]);
            dev[s].stride = sources[s].sector_size;
        }
        return psxhip_disc_finish_device(device, layout, dev, n_sources, (uint8_t*)(uintptr_t)(0x10000 + o_out), first_out, n_out, nullptr);
    }
    int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    DeviceBuffer buf;
    if ((rc = buf.reserve(o.end + 4))) return rc;
    uint8_t* const d = buf.as<uint8_t>();
    hipStream_t st = nullptr;
    for (int s = 0; s < n_sources; s++) {
        const psxhip_disc_source_t& S = sources[s];
        dev[s] = S;
        dev[s].sectors = d + at[s];
        dev[s].stride = S.sector_size;
        if (S.n_sectors > 0)
            HIP_TRY(hipMemcpy2DAsync(d + at[s], (size_t)S.sector_size, S.sectors, (size_t)S.stride, (size_t)S.sector_size, (size_t)S.n_sectors,
                                     hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    }
    rc = psxhip_disc_finish_device(device, layout, dev, n_sources, d + o_out, first_out, n_out, st);
    if (rc) return rc;
    if (n_out > 0) HIP_TRY(hipMemcpyAsync(out, d + o_out, (size_t)n_out * 2352, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}
