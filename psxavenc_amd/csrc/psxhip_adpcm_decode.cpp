// psxhip_adpcm_decode.cpp -- the ADPCM decoder's entry points (include/psxav_hip.h).  Device level: argument
// checks, the chunk tables and the verify passes of the chunked decode, the SSE and disassemble calls.  Host-buffer conveniences
// (psxhip_spu_decode_streams_host, psxhip_xa_decode_streams_host): their refusals and sizes are reader_plan.h's (StreamsHostShape);
// they build the chain descriptors, move buffers, call the former.  They launch adpcm_decode_kernels.hip and sector_kernels.hip; no
// decoding happens on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "device_buffer.h"
#include "host_layout.h"
#include "psxhip_adpcm_internal.h"
#include "psxhip_internal.h"
#include "reader_plan.h"
#include "verify_passes.h"

namespace {

bool bad_coding(int filter_count, int bits) {
    return (filter_count != 4 && filter_count != 5) || (bits != 4 && bits != 8) || (bits == 8 && filter_count == 5);
}

}  // namespace

// measurement (psxhip_adpcm_decode_set_timing): the calling thread's switch and its last chunked call's two durations
static thread_local bool g_timing = false;
static thread_local float g_spec_ms = 0.f, g_verify_ms = 0.f;

extern "C" int psxhip_adpcm_decode_set_timing(int on) {
    g_timing = on != 0;
    return PSXHIP_OK;
}

extern "C" int psxhip_adpcm_decode_last_timing(float* speculate_ms, float* verify_ms) {
    if (speculate_ms) *speculate_ms = g_spec_ms;
    if (verify_ms) *verify_ms = g_verify_ms;
    return PSXHIP_OK;
}

extern "C" const char* psxhip_adpcm_decode_kernel_rev(void) { return PSXHIP_ADPCM_DECODE_KERNEL_REV; }

extern "C" int psxhip_adpcm_decode_chains_device(int device, const uint8_t* d_units, const psxhip_adpcm_chain_t* d_chains,
                                                 const int32_t* d_unit_base, int n_chains, int filter_count, int bits,
                                                 psxhip_adpcm_state_t* d_states, int16_t* d_samples, uint8_t* d_unit_flags, int16_t* d_tail,
                                                 void* stream) {
    if (n_chains < 0 || bad_coding(filter_count, bits) || (n_chains > 0 && (!d_units || !d_chains || !d_unit_base || !d_states || !d_samples)) ||
        ((uintptr_t)d_units & 15) || ((uintptr_t)d_samples & 1) || ((uintptr_t)d_tail & 3)) {
        psxhip_set_error("adpcm_decode_chains: bad argument (bits 4 or 8, filter_count 4 or 5 and 4 with 8 bits, d_units 16-byte aligned, d_tail 4-byte)");
        return PSXHIP_EINVAL;
    }
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_chains == 0) return PSXHIP_OK;
    psxhip_adpcm_decode_job_t job;
    memset(&job, 0, sizeof job);
    job.units = d_units; job.chains = d_chains; job.unit_base = d_unit_base; job.n_items = n_chains; job.filter_count = filter_count;
    job.states = d_states; job.samples = d_samples; job.unit_flags = d_unit_flags; job.tail = d_tail;
    HIP_TRY(psxhip_adpcm_decode_launch(&job, 0, bits, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_adpcm_decode_chains_chunked(int device, const uint8_t* d_units, const psxhip_adpcm_chain_t* chains,
                                                  const int32_t* unit_base, int n_chains, int filter_count, int bits,
                                                  psxhip_adpcm_state_t* d_states, int16_t* d_samples, uint8_t* d_unit_flags, int16_t* d_tail,
                                                  int chunk_units, int warmup_units, int max_passes, void* stream) {
    if (n_chains < 0 || bad_coding(filter_count, bits) || (n_chains > 0 && (!d_units || !chains || !unit_base || !d_states || !d_samples)) ||
        ((uintptr_t)d_units & 15) || ((uintptr_t)d_samples & 1) || ((uintptr_t)d_tail & 3)) {
        psxhip_set_error("adpcm_decode_chains_chunked: bad argument (bits 4 or 8, filter_count 4 or 5 and 4 with 8 bits, d_units 16-byte aligned, d_tail 4-byte)");
        return PSXHIP_EINVAL;
    }
    long long total_units = 0;
    for (int c = 0; c < n_chains; c++) {
        if (chains[c].pitch < 1 || chains[c].n_units < 0) {
            psxhip_set_error("adpcm_decode_chains_chunked: chain %d has pitch %d, n_units %d", c, chains[c].pitch, chains[c].n_units);
            return PSXHIP_EINVAL;
        }
        total_units += chains[c].n_units;
    }
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (total_units == 0) return 0;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    if (chunk_units <= 0) {
        // the encoder's rule (pick_chunking) for wavefronts of 64 chunks: long chunks so that verify needs few passes, enough of them to
        // fill the device.  A decode wavefront holds 64 chunks and a CU eight such wavefronts: at least four rounds of them
        int w = 0, n_cu = 0;
        psxhip_adpcm_pick_chunking(total_units, 64, device, &chunk_units, &w);
        if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cu < 1) n_cu = 256;
        const long long fill = total_units / (4ll * 8 * 64 * n_cu);
        const long long want = fill < 256 ? 256 : fill;
        if (want < chunk_units) chunk_units = (int)want;
    }
    if (warmup_units < 0) warmup_units = 64;       // decoding is cheap: a long warm-up, not the encoder's

    // the chunk table: chain by chain, the two chains of an interleaved stereo pair chunk by chunk in turns
    std::vector<int32_t> chunk_chain, chunk_first, chunk_pred, last_chunk((size_t)n_chains, -1);
    for (int c = 0; c < n_chains;) {
        const bool pair = c + 1 < n_chains && chains[c].pitch == 2 && chains[c + 1].pitch == 2 && chains[c].n_units > 0 &&
                          chains[c + 1].sample_offset == chains[c].sample_offset + 1 && chains[c + 1].n_units == chains[c].n_units;
        const int span = pair ? 2 : 1;
        for (int f = 0; f < chains[c].n_units; f += chunk_units)
            for (int k = 0; k < span; k++) {
                const int32_t idx = (int32_t)chunk_chain.size();
                last_chunk[c + k] = idx;
                chunk_chain.push_back(c + k);
                chunk_first.push_back(f);
                chunk_pred.push_back(f ? idx - span : -1);
            }
        c += span;
    }
    const size_t n_chunks = chunk_chain.size();
    if (n_chunks > 0x7FFFFFFFu) {
        psxhip_set_error("adpcm_decode_chains_chunked: %zu chunks", n_chunks);
        return PSXHIP_EINVAL;
    }
    BumpOffsets o;
    const size_t o_chains = o.take(sizeof(psxhip_adpcm_chain_t) * n_chains), o_base = o.take(4 * (size_t)n_chains), o_cc = o.take(4 * n_chunks);
    const size_t o_cf = o.take(4 * n_chunks), o_cp = o.take(4 * n_chunks), o_last = o.take(4 * (size_t)n_chains);
    const size_t o_used = o.take(8 * n_chunks), o_end = o.take(8 * n_chunks), o_flags = o.take(sizeof(int) * kVerifyBatchMax);
    DeviceBuffer ws;
    const int rc_ws = ws.reserve(o.end);
    if (rc_ws) return rc_ws;
    uint8_t* const d = ws.as<uint8_t>();
    hipStream_t st = (hipStream_t)stream;
    // declared after the workspace: on every way out the stream has come to rest before the workspace goes, and the timing events go too
    struct AtExit {
        hipStream_t st;
        bool at_rest;
        hipEvent_t ev[3];
        ~AtExit() {
            if (!at_rest) (void)hipStreamSynchronize(st);
            for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        }
    } at_exit{st, false, {nullptr, nullptr, nullptr}};
    hipEvent_t* const ev = at_exit.ev;
    int h_flags[kVerifyBatchMax];
    HIP_TRY(hipMemcpyAsync(d + o_chains, chains, sizeof(psxhip_adpcm_chain_t) * n_chains, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + o_base, unit_base, 4 * (size_t)n_chains, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + o_cc, chunk_chain.data(), 4 * n_chunks, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + o_cf, chunk_first.data(), 4 * n_chunks, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + o_cp, chunk_pred.data(), 4 * n_chunks, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + o_last, last_chunk.data(), 4 * (size_t)n_chains, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    psxhip_adpcm_decode_job_t job;
    memset(&job, 0, sizeof job);
    job.units = d_units; job.chains = (const psxhip_adpcm_chain_t*)(d + o_chains); job.unit_base = (const int32_t*)(d + o_base);
    job.n_items = (int)n_chunks; job.filter_count = filter_count; job.states = d_states; job.samples = d_samples;
    job.unit_flags = d_unit_flags; job.tail = d_tail;
    job.chunk_chain = (const int32_t*)(d + o_cc); job.chunk_first = (const int32_t*)(d + o_cf);
    job.chunk_pred = (const int32_t*)(d + o_cp);
    job.chunk_units = chunk_units; job.warmup_units = warmup_units;
    job.start_used = (unsigned long long*)(d + o_used); job.chunk_end = (unsigned long long*)(d + o_end);
    int* d_flags = (int*)(d + o_flags);
    const bool timed = g_timing;
    if (timed)
        for (int i = 0; i < 3; i++) HIP_TRY(hipEventCreate(&ev[i]), PSXHIP_EDEVICE);
    if (timed) HIP_TRY(hipEventRecord(ev[0], st), PSXHIP_EDEVICE);
    HIP_TRY(psxhip_adpcm_decode_launch(&job, 0, bits, st), PSXHIP_EDEVICE);
    if (timed) HIP_TRY(hipEventRecord(ev[1], st), PSXHIP_EDEVICE);
    // verify passes until one changes nothing (verify_passes.h); an exhausted max_passes leaves the chains' states as they were
    bool changed;
    const int passes = run_verify_passes(
        [&](int* flag, const int* flag_before) {
            job.changed = flag;
            job.changed_before = flag_before;
            return psxhip_adpcm_decode_launch(&job, 1, bits, st);
        },
        d_flags, h_flags, st, max_passes, "adpcm_decode_chains_chunked", &changed);
    if (passes < 0) return passes;
    HIP_TRY(psxhip_adpcm_decode_final_launch((const int32_t*)(d + o_last), (const unsigned long long*)(d + o_end), n_chains, d_states, st),
            PSXHIP_EDEVICE);
    if (timed) {
        HIP_TRY(hipEventRecord(ev[2], st), PSXHIP_EDEVICE);
        HIP_TRY(hipEventSynchronize(ev[2]), PSXHIP_EDEVICE);
        HIP_TRY(hipEventElapsedTime(&g_spec_ms, ev[0], ev[1]), PSXHIP_EDEVICE);
        HIP_TRY(hipEventElapsedTime(&g_verify_ms, ev[1], ev[2]), PSXHIP_EDEVICE);
    }
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    at_exit.at_rest = true;
    return passes;
}

extern "C" int psxhip_adpcm_sse_device(int device, const int16_t* d_a, const int16_t* d_a_tail, const int16_t* d_b,
                                       const psxhip_adpcm_chain_t* d_chains, int n_chains, uint64_t* d_unit_sse, const int32_t* d_unit_base,
                                       uint64_t* d_chain_sums, void* stream) {
    if (n_chains < 0 || (n_chains > 0 && (!d_a || !d_b || !d_chains || (d_unit_sse && !d_unit_base))) || ((uintptr_t)d_a & 1) ||
        ((uintptr_t)d_b & 1) || ((uintptr_t)d_a_tail & 1) || ((uintptr_t)d_unit_sse & 7) || ((uintptr_t)d_chain_sums & 7)) {
        psxhip_set_error("adpcm_sse: NULL or misaligned argument, negative chain count, or d_unit_sse without d_unit_base");
        return PSXHIP_EINVAL;
    }
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_chains == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    if (d_chain_sums) HIP_TRY(hipMemsetAsync(d_chain_sums, 0, (size_t)n_chains * 2 * sizeof(uint64_t), (hipStream_t)stream), PSXHIP_EDEVICE);
    psxhip_adpcm_sse_job_t job;
    job.a = d_a; job.b = d_b; job.a_tail = d_a_tail; job.chains = d_chains; job.unit_base = d_unit_base;
    job.unit_sse = (unsigned long long*)d_unit_sse; job.chain_sums = (unsigned long long*)d_chain_sums;
    // the host does not know the chains' lengths: enough slices that a few long chains fill the device, few enough that many short
    // chains do not launch mostly idle wavefronts
    int slices = 16384 / n_chains;
    slices = slices < 1 ? 1 : (slices > 1024 ? 1024 : slices);
    HIP_TRY(psxhip_adpcm_sse_launch(&job, n_chains, slices, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_xa_disassemble_device(int device, const uint8_t* d_sectors, int n_sectors, int format, int stereo, int frequency,
                                            int bits, uint8_t* d_units, int32_t* d_sector_status, void* stream) {
    if (n_sectors < 0 || (format != 0 && format != 1) || (bits != 4 && bits != 8) || (n_sectors > 0 && (!d_sectors || !d_units)) ||
        ((uintptr_t)d_sectors & 3) || ((uintptr_t)d_units & 3) || ((uintptr_t)d_sector_status & 3)) {
        psxhip_set_error("xa_disassemble: bad argument (format 0 or 1, bits 4 or 8, pointers 4-byte aligned)");
        return PSXHIP_EINVAL;
    }
    int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_sectors == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    if ((rc = psxhip_sector_tables(device))) return rc;
    psxhip_xa_dis_job_t job;
    job.sectors = d_sectors; job.n_sectors = n_sectors; job.format = format; job.stereo = stereo; job.frequency = frequency; job.bits = bits;
    job.units = d_units; job.status = d_sector_status;
    static const uint32_t delta = [] {      // the EDC (bit by bit) of the form-2 span, sector bytes 0x10 .. 0x92B, with the two EOF bits alone
        uint32_t c = 0;
        for (int i = 0; i < 0x91C; i++) {
            c ^= (i == 2 || i == 6) ? 0x80u : 0u;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0xD8018001u : 0u);
        }
        return c;
    }();
    job.eof_edc_delta = delta;
    HIP_TRY(psxhip_xa_disassemble_launch(&job, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}
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
    StreamsHostShape p;
    int rc = spu_streams_host_shape(n_streams, in_stride, n_blocks, blocks && states && samples, out_stride, &p);
    if (rc) return rc;
    if ((rc = psxhip_ensure_device(device))) return rc;
    if (n_streams == 0 || n_blocks == 0) return p.per_channel;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    std::vector<psxhip_adpcm_chain_t> chains(p.n_chains);
    std::vector<int32_t> base(p.n_chains);
    fill_planar_chains(chains.data(), base.data(), n_streams, p.per_channel, 1, p.per_channel, n_blocks);
    DeviceBuffer d_u, d_st, d_s;
    if ((rc = alloc(d_u, p.unit_bytes)) || (rc = alloc(d_st, p.state_bytes)) || (rc = alloc(d_s, p.sample_bytes))) return rc;
    hipStream_t st = nullptr;
    HIP_TRY(hipMemcpy2DAsync(d_u.p, p.in_bytes, blocks, (size_t)p.in_stride, p.in_bytes, (size_t)n_streams, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d_st.p, states, p.state_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    rc = decode_chains(device, d_u.as<uint8_t>(), chains, base, 5, 4, d_st.as<psxhip_adpcm_state_t>(), d_s.as<int16_t>(), st);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(samples, (size_t)p.out_stride * sizeof(int16_t), d_s.p, p.per * sizeof(int16_t), p.per * sizeof(int16_t),
                             (size_t)n_streams, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(states, d_st.p, p.state_bytes, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return p.per_channel;
}

extern "C" int psxhip_xa_decode_streams_host(int device, int format, int stereo, int frequency, int bits, const uint8_t* sectors,
                                             int n_streams, int64_t in_stride, int n_sectors, psxhip_adpcm_state_t* states,
                                             int16_t* samples, int64_t out_stride, int32_t* sector_status) {
    StreamsHostShape p;
    int rc = xa_streams_host_shape(format, stereo, bits, n_streams, in_stride, n_sectors, sectors && states && samples, out_stride, &p);
    if (rc) return rc;
    if ((rc = psxhip_ensure_device(device))) return rc;
    if (n_streams == 0 || n_sectors == 0) return p.per_channel;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    std::vector<psxhip_adpcm_chain_t> chains(p.n_chains);
    std::vector<int32_t> base(p.n_chains);
    fill_interleaved_chains(chains.data(), base.data(), n_streams, p.channels, (int64_t)p.per, p.per_channel, p.units_per_stream);
    DeviceBuffer d_in, d_u, d_st, d_s, d_status;
    if ((rc = alloc(d_in, p.src_bytes)) || (rc = alloc(d_u, p.unit_bytes)) || (rc = alloc(d_st, p.state_bytes)) ||
        (rc = alloc(d_s, p.sample_bytes)) || (rc = alloc(d_status, p.status_bytes)))
        return rc;
    hipStream_t st = nullptr;
    HIP_TRY(hipMemcpy2DAsync(d_in.p, p.in_bytes, sectors, (size_t)p.in_stride, p.in_bytes, (size_t)n_streams, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d_st.p, states, p.state_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    // the streams' sectors lie back to back: one launch takes them all apart (a stream's records are a whole number of sectors')
    rc = psxhip_xa_disassemble_device(device, d_in.as<uint8_t>(), (int)p.total_sectors, format, stereo, frequency, bits, d_u.as<uint8_t>(),
                                      d_status.as<int32_t>(), st);
    if (rc) return rc;
    rc = decode_chains(device, d_u.as<uint8_t>(), chains, base, 4, bits, d_st.as<psxhip_adpcm_state_t>(), d_s.as<int16_t>(), st);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(samples, (size_t)p.out_stride * sizeof(int16_t), d_s.p, p.per * sizeof(int16_t), p.per * sizeof(int16_t),
                             (size_t)n_streams, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(states, d_st.p, p.state_bytes, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    if (sector_status) HIP_TRY(hipMemcpyAsync(sector_status, d_status.p, p.status_bytes, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return p.per_channel;
}
