// psxhip_adpcm_decode.cpp -- host-buffer conveniences of the ADPCM decoder (psxhip_spu_decode_streams_host,
// psxhip_xa_decode_streams_host; include/psxav_hip.h): build the chain descriptors, move buffers, launch the
// disassemble / decode kernels (adpcm_decode_kernels.hip).  No decoding happens on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "device_buffer.h"
#include "host_layout.h"
#include "psxhip_internal.h"

namespace {

// a call's temporaries (never an empty allocation)
int alloc(DeviceBuffer& b, size_t n) { return b.reserve(n ? n : 4); }

// decode `chains` (host arrays) from d_units into d_samples: serial per chain, or cut along time when the chains are long
int decode_chains(int device, const uint8_t* d_units, const std::vector<psxhip_adpcm_chain_t>& chains, const std::vector<int32_t>& base,
                  int filter_count, int bits, psxhip_adpcm_state_t* d_states, int16_t* d_samples, hipStream_t st) {
    const int n = (int)chains.size();
    if (n > 0 && chains[0].n_units >= psxhip_adpcm_chunked_threshold(n)) {
        HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
        const int rc = psxhip_adpcm_decode_chains_chunked(device, d_units, chains.data(), base.data(), n, filter_count, bits, d_states,
                                                          d_samples, nullptr, nullptr, 0, -1, 0, st);
        return rc < 0 ? rc : PSXHIP_OK;
    }
    DeviceBuffer d_c, d_b;
    int rc;
    if ((rc = alloc(d_c, chains.size() * sizeof(chains[0]))) || (rc = alloc(d_b, base.size() * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(d_c.p, chains.data(), chains.size() * sizeof(chains[0]), hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d_b.p, base.data(), base.size() * sizeof(int32_t), hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    rc = psxhip_adpcm_decode_chains_device(device, d_units, d_c.as<psxhip_adpcm_chain_t>(), d_b.as<int32_t>(), n, filter_count, bits, d_states,
                                           d_samples, nullptr, nullptr, st);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);      // the tables are freed on return
    return PSXHIP_OK;
}

}  // namespace

extern "C" int psxhip_spu_decode_streams_host(int device, const uint8_t* blocks, int n_streams, int64_t in_stride, int n_blocks,
                                              psxhip_adpcm_state_t* states, int16_t* samples, int64_t out_stride) {
    if (n_streams < 0 || n_blocks < 0 || (n_streams > 0 && n_blocks > 0 && (!blocks || !states || !samples)) ||
        (int64_t)n_blocks * 28 > 0x7FFFFFFF) {
        psxhip_set_error("spu_decode_streams_host: bad argument");
        return PSXHIP_EINVAL;
    }
    const int per = n_blocks * 28;
    const size_t in_bytes = (size_t)n_blocks * 16;
    if (n_streams == 1) { in_stride = (int64_t)in_bytes; out_stride = per; }
    if (n_streams > 0 && (in_stride < (int64_t)in_bytes || out_stride < per)) {
        psxhip_set_error("spu_decode_streams_host: in_stride %lld < %zu bytes or out_stride %lld < %d samples per stream",
                         (long long)in_stride, in_bytes, (long long)out_stride, per);
        return PSXHIP_EINVAL;
    }
    const int rc0 = psxhip_ensure_device(device);
    if (rc0) return rc0;
    if (n_streams == 0 || n_blocks == 0) return per;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    std::vector<psxhip_adpcm_chain_t> chains((size_t)n_streams);
    std::vector<int32_t> base((size_t)n_streams);
    fill_planar_chains(chains.data(), base.data(), n_streams, per, 1, per, n_blocks);
    DeviceBuffer d_u, d_st, d_s;
    int rc;
    if ((rc = alloc(d_u, in_bytes * n_streams)) || (rc = alloc(d_st, sizeof(psxhip_adpcm_state_t) * n_streams)) ||
        (rc = alloc(d_s, sizeof(int16_t) * (size_t)per * n_streams)))
        return rc;
    hipStream_t st = nullptr;
    HIP_TRY(hipMemcpy2DAsync(d_u.p, in_bytes, blocks, (size_t)in_stride, in_bytes, (size_t)n_streams, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d_st.p, states, sizeof(psxhip_adpcm_state_t) * n_streams, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    rc = decode_chains(device, d_u.as<uint8_t>(), chains, base, 5, 4, d_st.as<psxhip_adpcm_state_t>(), d_s.as<int16_t>(), st);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(samples, (size_t)out_stride * sizeof(int16_t), d_s.p, (size_t)per * sizeof(int16_t), (size_t)per * sizeof(int16_t),
                             (size_t)n_streams, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(states, d_st.p, sizeof(psxhip_adpcm_state_t) * n_streams, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return per;
}

extern "C" int psxhip_xa_decode_streams_host(int device, int format, int stereo, int frequency, int bits, const uint8_t* sectors,
                                             int n_streams, int64_t in_stride, int n_sectors, psxhip_adpcm_state_t* states,
                                             int16_t* samples, int64_t out_stride, int32_t* sector_status) {
    if (n_streams < 0 || n_sectors < 0 || (bits != 4 && bits != 8) || (format != 0 && format != 1) ||
        (n_streams > 0 && n_sectors > 0 && (!sectors || !states || !samples)) || (int64_t)n_sectors * 4032 > 0x7FFFFFFF ||
        (int64_t)n_streams * n_sectors > 0x7FFFFFFF / 144) {
        psxhip_set_error("xa_decode_streams_host: bad argument");
        return PSXHIP_EINVAL;
    }
    const XaLayout xa = xa_layout(format, stereo, bits);
    const int ch = xa.channels, units_per_stream = n_sectors * xa.units_per_sector;
    const int per_channel = units_per_stream / ch * 28;
    const size_t per = (size_t)per_channel * ch, in_bytes = (size_t)n_sectors * xa.sector_bytes;
    if (n_streams == 1) { in_stride = (int64_t)in_bytes; out_stride = (int64_t)per; }
    if (n_streams > 0 && (in_stride < (int64_t)in_bytes || out_stride < (int64_t)per)) {
        psxhip_set_error("xa_decode_streams_host: in_stride %lld < %zu bytes or out_stride %lld < %zu samples per stream",
                         (long long)in_stride, in_bytes, (long long)out_stride, per);
        return PSXHIP_EINVAL;
    }
    const int rc0 = psxhip_ensure_device(device);
    if (rc0) return rc0;
    if (n_streams == 0 || n_sectors == 0) return per_channel;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    std::vector<psxhip_adpcm_chain_t> chains((size_t)n_streams * ch);
    std::vector<int32_t> base((size_t)n_streams * ch);
    fill_interleaved_chains(chains.data(), base.data(), n_streams, ch, (int64_t)per, per_channel, units_per_stream);
    const size_t total_sectors = (size_t)n_streams * n_sectors;
    DeviceBuffer d_in, d_u, d_st, d_s, d_status;
    int rc;
    if ((rc = alloc(d_in, in_bytes * n_streams)) || (rc = alloc(d_u, (size_t)n_streams * units_per_stream * xa.record_bytes)) ||
        (rc = alloc(d_st, sizeof(psxhip_adpcm_state_t) * chains.size())) || (rc = alloc(d_s, sizeof(int16_t) * per * n_streams)) ||
        (rc = alloc(d_status, sizeof(int32_t) * total_sectors)))
        return rc;
    hipStream_t st = nullptr;
    HIP_TRY(hipMemcpy2DAsync(d_in.p, in_bytes, sectors, (size_t)in_stride, in_bytes, (size_t)n_streams, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d_st.p, states, sizeof(psxhip_adpcm_state_t) * chains.size(), hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    // the streams' sectors lie back to back: one launch takes them all apart (a stream's records are a whole number of sectors')
    rc = psxhip_xa_disassemble_device(device, d_in.as<uint8_t>(), (int)total_sectors, format, stereo, frequency, bits, d_u.as<uint8_t>(),
                                      d_status.as<int32_t>(), st);
    if (rc) return rc;
    rc = decode_chains(device, d_u.as<uint8_t>(), chains, base, 4, bits, d_st.as<psxhip_adpcm_state_t>(), d_s.as<int16_t>(), st);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(samples, (size_t)out_stride * sizeof(int16_t), d_s.p, per * sizeof(int16_t), per * sizeof(int16_t),
                             (size_t)n_streams, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(states, d_st.p, sizeof(psxhip_adpcm_state_t) * chains.size(), hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    if (sector_status)
        HIP_TRY(hipMemcpyAsync(sector_status, d_status.p, sizeof(int32_t) * total_sectors, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return per_channel;
}
