// psxhip_adpcm_decode.cpp -- the ADPCM decoder's entry points (include/psxav_hip.h).  What they refuse, the
// chunk length, the chunk tables and the carving of the workspace, the route and the host-buffer shapes are adpcm_plan.cpp's, without
// HIP; here the plans are executed.  Device level: the chunked decode with its verify passes, the SSE and disassemble calls.
// Host-buffer conveniences (psxhip_spu_decode_streams_host, psxhip_xa_decode_streams_host): they build the chain descriptors, move
// buffers, call the former.  They launch adpcm_decode_kernels.hip and sector_kernels.hip; no decoding happens on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "device_buffer.h"
#include "adpcm_plan.h"
#include "psxhip_adpcm_internal.h"
#include "psxhip_internal.h"
#include "verify_passes.h"

static_assert(kVerifyBatchMax == kAdpcmVerifyBatchMax, "the workspace holds verify_passes.h's flag words");

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
    int rc = adpcm_decode_chains_check(false, (uintptr_t)d_units, d_chains != nullptr, d_unit_base != nullptr, (uintptr_t)d_states, (uintptr_t)d_samples,
                                       (uintptr_t)d_tail, n_chains, filter_count, bits);
    if (rc) return rc;
    if ((rc = psxhip_ensure_device(device))) return rc;
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
    int rc = adpcm_decode_chains_check(true, (uintptr_t)d_units, chains != nullptr, unit_base != nullptr, (uintptr_t)d_states, (uintptr_t)d_samples,
                                       (uintptr_t)d_tail, n_chains, filter_count, bits);
    if (rc) return rc;
    long long total_units;
    if ((rc = adpcm_decode_chunked_chains_check(chains, n_chains, &total_units))) return rc;
    if ((rc = psxhip_ensure_device(device))) return rc;
    if (total_units == 0) return 0;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    if (chunk_units <= 0) chunk_units = adpcm_decode_chunking(total_units, psxhip_adpcm_device_cus(device));
    if (warmup_units < 0) warmup_units = 64;       // decoding is cheap: a long warm-up, not the encoder's

    AdpcmDecodePlan p;
    if ((rc = adpcm_decode_plan(chains, n_chains, chunk_units, &p))) return rc;
    const size_t n_chunks = p.n_chunks;
    DeviceBuffer ws;
    if ((rc = ws.reserve(p.bytes))) return rc;
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
    HIP_TRY(hipMemcpyAsync(d + p.o_chains, chains, sizeof(psxhip_adpcm_chain_t) * n_chains, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + p.o_base, unit_base, 4 * (size_t)n_chains, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + p.o_cc, p.chunk_chain.data(), 4 * n_chunks, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + p.o_cf, p.chunk_first.data(), 4 * n_chunks, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + p.o_cp, p.chunk_pred.data(), 4 * n_chunks, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d + p.o_last, p.last_chunk.data(), 4 * (size_t)n_chains, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    psxhip_adpcm_decode_job_t job;
    memset(&job, 0, sizeof job);
    job.units = d_units; job.chains = (const psxhip_adpcm_chain_t*)(d + p.o_chains); job.unit_base = (const int32_t*)(d + p.o_base);
    job.n_items = (int)n_chunks; job.filter_count = filter_count; job.states = d_states; job.samples = d_samples;
    job.unit_flags = d_unit_flags; job.tail = d_tail;
    job.chunk_chain = (const int32_t*)(d + p.o_cc); job.chunk_first = (const int32_t*)(d + p.o_cf);
    job.chunk_pred = (const int32_t*)(d + p.o_cp);
    job.chunk_units = chunk_units; job.warmup_units = warmup_units;
    job.start_used = (unsigned long long*)(d + p.o_used); job.chunk_end = (unsigned long long*)(d + p.o_end);
    int* d_flags = (int*)(d + p.o_flags);
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
    HIP_TRY(psxhip_adpcm_decode_final_launch((const int32_t*)(d + p.o_last), (const unsigned long long*)(d + p.o_end), n_chains, d_states, st),
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
    int rc = adpcm_sse_check((uintptr_t)d_a, (uintptr_t)d_a_tail, (uintptr_t)d_b, (uintptr_t)d_chains, n_chains, (uintptr_t)d_unit_sse,
                             (uintptr_t)d_unit_base, (uintptr_t)d_chain_sums);
    if (rc) return rc;
    if ((rc = psxhip_ensure_device(device))) return rc;
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
    int rc = xa_disassemble_check((uintptr_t)d_sectors, n_sectors, format, bits, (uintptr_t)d_units, (uintptr_t)d_sector_status);
    if (rc) return rc;
    if ((rc = psxhip_ensure_device(device))) return rc;
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
    if (n > 0 && adpcm_route_chunked(chains[0].n_units, n)) {
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
