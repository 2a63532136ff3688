// psxhip_disc_read.cpp -- host side of the disc reader (psxhip_disc_reader_*, psxhip_disc_read_device, psxhip_disc_read_host;
// include/psxav_hip.h): argument checks, the handle's workspace, the job struct, the launches
// (disc_read_kernels.hip).  No sector byte is read, repaired or moved on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>

#include "device_buffer.h"
#include "host_layout.h"
#include "psxhip_disc_read_internal.h"
#include "psxhip_internal.h"

struct psxhip_disc_reader {
    int device = 0;
    DeviceBuffer ws;                  // psxhip_disc_read_device: the records (without a caller's table) and the span counts
    DeviceBuffer stage;               // psxhip_disc_read_host: image, track buffers, table, counts, summary
};

namespace {

// the rules of the track list that need no pointer
int check_tracks(const char* who, int64_t n_sectors, const psxhip_disc_track_t* tracks, int n_tracks) {
    if (n_sectors < 0 || n_sectors > 0x7FFFFFFFll || n_tracks < 0 || n_tracks > PSXHIP_DISC_MAX_SOURCES || (n_tracks > 0 && !tracks)) {
        psxhip_set_error("%s: n_sectors negative or 2^31 and more, NULL tracks, or more than %d tracks", who, PSXHIP_DISC_MAX_SOURCES);
        return PSXHIP_EINVAL;
    }
    for (int t = 0; t < n_tracks; t++) {
        const psxhip_disc_track_t& T = tracks[t];
        if ((T.sector_size != 2352 && T.sector_size != 2336 && T.sector_size != 2048) || T.capacity < 0 || (T.stride & 3) ||
            T.stride < T.sector_size || T.file_number < -1 || T.file_number > 255 || T.channel_number < -1 || T.channel_number > 31) {
            psxhip_set_error("%s: track %d: sector_size 2352 / 2336 / 2048, capacity >= 0, stride a multiple of 4 and >= sector_size, "
                             "file_number -1 .. 255, channel_number -1 .. 31", who, t);
            return PSXHIP_EINVAL;
        }
    }
    return PSXHIP_OK;
}

// every rule of psxhip_disc_read_device; no device call
int check_call(const char* who, const uint8_t* d_image, int64_t n_sectors, const psxhip_disc_track_t* tracks, int n_tracks,
               const void* d_table, const void* d_counts, const void* d_summary) {
    const int rc = check_tracks(who, n_sectors, tracks, n_tracks);
    if (rc) return rc;
    if ((n_sectors > 0 && !d_image) || !d_summary || (n_tracks > 0 && !d_counts) || misaligned(d_image) || misaligned(d_table) ||
        misaligned(d_counts) || ((uintptr_t)d_summary & 7) != 0) {      // (n_corrections takes a 64-bit atomic add)
        psxhip_set_error("%s: d_image, d_track_counts or d_summary NULL, a pointer not 4-byte aligned, or d_summary not 8-byte aligned", who);
        return PSXHIP_EINVAL;
    }
    const uintptr_t i0 = (uintptr_t)d_image, i1 = i0 + (size_t)n_sectors * 2352;
    uintptr_t lo[PSXHIP_DISC_MAX_SOURCES], hi[PSXHIP_DISC_MAX_SOURCES];
    for (int t = 0; t < n_tracks; t++) {
        const psxhip_disc_track_t& T = tracks[t];
        lo[t] = hi[t] = 0;
        if (T.capacity == 0) continue;
        if (!T.sectors || misaligned(T.sectors)) {
            psxhip_set_error("%s: track %d: sectors NULL or not 4-byte aligned", who, t);
            return PSXHIP_EINVAL;
        }
        lo[t] = (uintptr_t)T.sectors;
        hi[t] = lo[t] + (size_t)(T.capacity - 1) * (size_t)T.stride + (size_t)T.sector_size;
        if (n_sectors > 0 && lo[t] < i1 && i0 < hi[t]) {
            psxhip_set_error("%s: track %d's buffer overlaps the image", who, t);
            return PSXHIP_EINVAL;
        }
        for (int u = 0; u < t; u++)
            if (lo[u] < hi[t] && lo[t] < hi[u]) {
                psxhip_set_error("%s: the buffers of tracks %d and %d overlap", who, u, t);
                return PSXHIP_EINVAL;
            }
    }
    return PSXHIP_OK;
}

}  // namespace

extern "C" const char* psxhip_disc_read_kernel_rev(void) { return PSXHIP_DISC_READ_KERNEL_REV; }

extern "C" int psxhip_disc_reader_create(psxhip_disc_reader_t** out, int device) {
    if (!out) return PSXHIP_EINVAL;
    *out = nullptr;
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    psxhip_disc_reader* r = new (std::nothrow) psxhip_disc_reader;
    if (!r) return PSXHIP_ENOMEM;
    r->device = device;
    *out = r;
    return PSXHIP_OK;
}

extern "C" void psxhip_disc_reader_destroy(psxhip_disc_reader_t* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    delete r;
}

extern "C" int psxhip_disc_read_device(psxhip_disc_reader_t* reader, const uint8_t* d_image, int64_t n_sectors,
                                       const psxhip_disc_track_t* tracks, int n_tracks, psxhip_disc_read_sector_t* d_sector_table,
                                       int32_t* d_track_counts, psxhip_disc_read_summary_t* d_summary, void* stream) {
    static const char who[] = "psxhip_disc_read_device";
    int rc = check_call(who, d_image, n_sectors, tracks, n_tracks, d_sector_table, d_track_counts, d_summary);
    if (rc) return rc;
    if (psxhip_device_count() <= 0) return psxhip_no_device();
    if (!reader) {
        psxhip_set_error("%s: NULL handle", who);
        return PSXHIP_EINVAL;
    }
    HIP_TRY(hipSetDevice(reader->device), PSXHIP_EDEVICE);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_summary, 0, sizeof *d_summary, st), PSXHIP_EDEVICE);
    if (n_sectors == 0) {
        if (n_tracks > 0) HIP_TRY(hipMemsetAsync(d_track_counts, 0, (size_t)n_tracks * 4, st), PSXHIP_EDEVICE);
        return PSXHIP_OK;
    }
    if ((rc = psxhip_disc_read_tables(reader->device))) return rc;

    psxhip_disc_read_job_t j;
    memset(&j, 0, sizeof j);
    j.image = d_image;
    j.n_sectors = n_sectors;
    j.n_tracks = n_tracks;
    j.n_spans = (int32_t)((n_sectors + PSXHIP_DISC_READ_SPAN - 1) / PSXHIP_DISC_READ_SPAN);
    BumpOffsets o;
    const size_t o_table = o.take(d_sector_table ? 0 : (size_t)n_sectors * sizeof(psxhip_disc_read_sector_t));
    const size_t o_spans = o.take((size_t)j.n_spans * PSXHIP_DISC_MAX_SOURCES * 4);
    if ((rc = reader->ws.reserve(o.end))) return rc;
    uint8_t* const ws = reader->ws.as<uint8_t>();
    j.table = d_sector_table ? d_sector_table : (psxhip_disc_read_sector_t*)(ws + o_table);
    j.span_counts = (int32_t*)(ws + o_spans);
    j.track_counts = d_track_counts;
    j.summary = d_summary;
    for (int t = 0; t < n_tracks; t++) {
        const psxhip_disc_track_t& T = tracks[t];
        j.key[t] = (uint32_t)(T.file_number + 1) | (uint32_t)(T.channel_number + 1) << 9 | (uint32_t)T.submode_mask << 16 |
                   (uint32_t)T.submode_value << 24;
        psxhip_disc_read_dev_track_t& D = j.track[t];
        D.base = T.sectors;
        D.stride = T.stride;
        D.capacity = T.capacity;
        D.lead4 = T.sector_size == 2352 ? 0 : T.sector_size == 2336 ? 4 : 6;
        D.size4 = T.sector_size / 4;
    }
    HIP_TRY(psxhip_disc_read_launch(&j, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_disc_read_host(psxhip_disc_reader_t* reader, const uint8_t* image, int64_t n_sectors, const psxhip_disc_track_t* tracks,
                                     int n_tracks, psxhip_disc_read_sector_t* sector_table, int32_t* track_counts,
                                     psxhip_disc_read_summary_t* summary) {
    static const char who[] = "psxhip_disc_read_host";
    int rc = check_tracks(who, n_sectors, tracks, n_tracks);
    if (rc) return rc;
    if ((n_sectors > 0 && !image) || !summary || (n_tracks > 0 && !track_counts)) {
        psxhip_set_error("%s: image, track_counts or summary NULL", who);
        return PSXHIP_EINVAL;
    }
    for (int t = 0; t < n_tracks; t++)
        if (tracks[t].capacity > 0 && !tracks[t].sectors) {
            psxhip_set_error("%s: track %d: sectors NULL", who, t);
            return PSXHIP_EINVAL;
        }
    if (psxhip_device_count() <= 0) return psxhip_no_device();
    if (!reader) {
        psxhip_set_error("%s: NULL handle", who);
        return PSXHIP_EINVAL;
    }
    HIP_TRY(hipSetDevice(reader->device), PSXHIP_EDEVICE);
    // the image, the tracks densely, then the results in one block: the device call checks the rest
    psxhip_disc_track_t dev[PSXHIP_DISC_MAX_SOURCES];
    BumpOffsets o;
    const size_t o_image = o.take((size_t)n_sectors * 2352);
    size_t at[PSXHIP_DISC_MAX_SOURCES];
    for (int t = 0; t < n_tracks; t++) at[t] = o.take((size_t)tracks[t].capacity * (size_t)tracks[t].sector_size);
    const size_t o_table = o.take(sector_table ? (size_t)n_sectors * sizeof *sector_table : 0);
    const size_t o_counts = o.take(PSXHIP_DISC_MAX_SOURCES * 4), o_summary = o.take(sizeof *summary);
    if ((rc = reader->stage.reserve(o.end))) return rc;
    uint8_t* const d = reader->stage.as<uint8_t>();
    hipStream_t st = nullptr;
    if (n_sectors > 0) HIP_TRY(hipMemcpyAsync(d + o_image, image, (size_t)n_sectors * 2352, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    for (int t = 0; t < n_tracks; t++) {
        dev[t] = tracks[t];
        dev[t].sectors = tracks[t].capacity > 0 ? d + at[t] : nullptr;
        dev[t].stride = tracks[t].sector_size;
    }
    rc = psxhip_disc_read_device(reader, d + o_image, n_sectors, dev, n_tracks, sector_table ? (psxhip_disc_read_sector_t*)(d + o_table) : nullptr,
                                 (int32_t*)(d + o_counts), (psxhip_disc_read_summary_t*)(d + o_summary), st);
    if (rc) return rc;
    if (n_tracks > 0) HIP_TRY(hipMemcpyAsync(track_counts, d + o_counts, (size_t)n_tracks * 4, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(summary, d + o_summary, sizeof *summary, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    if (sector_table && n_sectors > 0)
        HIP_TRY(hipMemcpyAsync(sector_table, d + o_table, (size_t)n_sectors * sizeof *sector_table, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    // only the slots that were written travel back
    for (int t = 0; t < n_tracks; t++) {
        const psxhip_disc_track_t& T = tracks[t];
        int32_t count;                     // (track_counts is the caller's host memory: no alignment rule)
        memcpy(&count, (const uint8_t*)track_counts + (size_t)t * 4, sizeof count);
        const size_t rows = (size_t)(count < T.capacity ? count : T.capacity);
        if (rows > 0)
            HIP_TRY(hipMemcpy2DAsync(T.sectors, (size_t)T.stride, d + at[t], (size_t)T.sector_size, (size_t)T.sector_size, rows,
                                     hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    }
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}
