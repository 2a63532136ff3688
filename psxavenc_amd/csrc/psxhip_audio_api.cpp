// psxhip_audio_api.cpp -- host-buffer batches for the ADPCM path (include/psxav_hip.h): their refusals, shapes and routes are
// adpcm_plan.cpp's, without HIP; here are the scratch pools, and the plans are executed: the chain descriptors filled, buffers moved,
// the chain / pack / assemble kernels launched.  No encoding happens on the host.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "adpcm_plan.h"
#include "psxhip_adpcm_internal.h"
#include "psxhip_internal.h"

static_assert(PSXHIP_ADPCM_CALL_STAGE_MAX == kAdpcmCallStageMax, "the plan's fast-path gate and the call kernel stage the same number of elements");

// the surface of adpcm_plan.h's route and chunking rules
extern "C" int psxhip_adpcm_chunked_threshold(int n_chains) { return adpcm_chunked_threshold(n_chains); }

int psxhip_adpcm_device_cus(int device) {
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cu < 1) n_cu = 256;
    return n_cu;
}

extern "C" void psxhip_adpcm_pick_chunking(long long total_units, int rows, int device, int* chunk_units, int* warmup_units) {
    const AdpcmChunking k = adpcm_chunking(total_units, rows, psxhip_adpcm_device_cus(device));
    *chunk_units = k.chunk_units;
    *warmup_units = k.warmup_units;
}

namespace {

// Device scratch of the host-buffer entry points.  The reference calls psx_audio_spu_encode once per 28 samples and
// psx_audio_xa_encode once per sector (filefmt.c:243,184): allocating half a dozen device buffers per call would cost far
// more than the encode, so every host thread keeps its scratch buffers between calls (grown on demand, released by
// psxhip_release_scratch() or with the process).
struct ScratchPool {
    static constexpr int kSlots = 8;
    void* p[kSlots] = {nullptr};
    size_t cap[kSlots] = {0};
    int device = -1;
    void release() {
        for (int i = 0; i < kSlots; i++) {
            if (p[i]) (void)hipFree(p[i]);
            p[i] = nullptr;
            cap[i] = 0;
        }
    }
    hipError_t get(int slot, int dev, size_t n, void** out) {
        if (dev != device) {
            release();
            device = dev;
        }
        if (n > cap[slot]) {
            if (p[slot]) (void)hipFree(p[slot]);
            p[slot] = nullptr;
            cap[slot] = 0;
            const size_t want = n + n / 2 + 256;
            hipError_t e = hipMalloc(&p[slot], want);
            if (e != hipSuccess) return e;
            cap[slot] = want;
        }
        *out = p[slot];
        return hipSuccess;
    }
};
thread_local ScratchPool g_pool;
thread_local int g_pool_device = 0;

struct DevBuf {
    void* p = nullptr;
    int slot;
    explicit DevBuf(int s) : slot(s) {}
    hipError_t alloc(size_t n) { return g_pool.get(slot, g_pool_device, n ? n : 4, &p); }
    template <typename T> T* as() { return (T*)p; }
};

// The per-call fast path (the reference calls psx_audio_spu_encode once per 28 samples and psx_audio_xa_encode once per sector,
// filefmt.c:243,184): one page-locked, device-visible block per host thread -- samples in, blocks / sectors and states out -- and
// one stream.  A call is: copy the samples in (CPU), ONE launch (two for XA: chains, sector assembly), wait, copy the result out.
struct CallScratch {
    static constexpr size_t kIn = kAdpcmCallIn, kOut = kAdpcmCallOut, kStates = kAdpcmCallStates;
    uint8_t* h = nullptr;       // [kIn samples | kOut blocks or sectors | kStates]
    uint8_t* d = nullptr;       // the same block as the device addresses it
    hipStream_t stream = nullptr;
    int device = -1;
    bool disabled = false;
    void release() {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        if (h) (void)hipHostFree(h);
        h = nullptr;
        stream = nullptr;
        device = -1;
    }
    ~CallScratch() { release(); }
    bool ready(int dev) {
        if (disabled) return false;
        if (h && device == dev) return true;
        release();
        if (getenv("PSXHIP_NO_PERCALL_PATH")) { disabled = true; return false; }      // experiments / A-B measurements
        if (hipHostMalloc((void**)&h, kIn + kOut + kStates, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
            (void)hipGetLastError();
            h = nullptr;
            return false;
        }
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, h, 0) != hipSuccess || !dp) {
            (void)hipGetLastError();
            (void)hipHostFree(h);
            h = nullptr;
            return false;
        }
        d = (uint8_t*)dp;
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipHostFree(h);
            h = nullptr;
            stream = nullptr;
            return false;
        }
        device = dev;
        return true;
    }
    int16_t* in() { return (int16_t*)h; }
    uint8_t* out() { return h + kIn; }
    psxhip_adpcm_state_t* states() { return (psxhip_adpcm_state_t*)(h + kIn + kOut); }
    const int16_t* d_in() { return (const int16_t*)d; }
    uint8_t* d_out() { return d + kIn; }
    psxhip_adpcm_state_t* d_states() { return (psxhip_adpcm_state_t*)(d + kIn + kOut); }
};
thread_local CallScratch g_call;

}  // namespace

extern "C" void psxhip_release_scratch(void) {
    g_pool.release();
    g_call.release();
}

// the chains of a host-buffer batch: serial or cut along time (the uploads from the batch's host vectors have left them by then)
static int encode_batch_chains(int device, const int16_t* d_samples, const std::vector<psxhip_adpcm_chain_t>& chains,
                               const std::vector<int32_t>& base, const psxhip_adpcm_chain_t* d_chains, const int32_t* d_base,
                               int units_per_chain, int rows, int filter_count, int bits, int beam, psxhip_adpcm_state_t* d_states,
                               uint8_t* d_units, hipStream_t st) {
    const int n = (int)chains.size();
    const bool chunked = adpcm_route_chunked(units_per_chain, n);
    if (chunked) HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return psxhip_adpcm_encode_routed(device, d_samples, chains.data(), base.data(), d_chains, d_base, n, chunked, (long long)units_per_chain * n, rows,
                                      filter_count, bits, beam, d_states, d_units, st);
}

static int spu_encode_streams(int device, const int16_t* samples, int n_streams, int64_t stream_stride, int pitch, int samples_per_stream,
                              psxhip_adpcm_state_t* states, uint8_t* out, int64_t out_stride, int beam) {
    SpuEncodeShape p;
    int rc = spu_encode_shape(samples && states && out, n_streams, stream_stride, pitch, samples_per_stream, out_stride, &p);
    if (rc) return rc;
    const int n_units = p.n_units, bytes = p.bytes;
    if (p.empty) return bytes;
    if ((rc = psxhip_ensure_device(device))) return rc;

    // ---- the reference's call pattern (a few streams, a few blocks): one launch, no copies (see CallScratch)
    if (spu_call_fast_path(beam, n_streams, n_units, kAdpcmCallStageMax, CallScratch::kOut) && g_call.ready(device)) {
        psxhip_adpcm_call_job_t a;
        memset(&a, 0, sizeof a);
        const size_t row = p.row;       // staged row per stream: pitch 1, zero-padded to whole units
        int16_t* in = g_call.in();
        for (int i = 0; i < n_streams; i++) {
            const int16_t* src = samples + (size_t)i * (size_t)p.stream_stride;
            int16_t* dst = in + (size_t)i * row;
            if (pitch == 1) memcpy(dst, src, (size_t)samples_per_stream * sizeof(int16_t));
            else for (int k = 0; k < samples_per_stream; k++) dst[k] = src[(size_t)k * pitch];
            memset(dst + samples_per_stream, 0, (row - (size_t)samples_per_stream) * sizeof(int16_t));
            a.states_in[i] = states[i];
        }
        fill_planar_chains(a.chains, a.unit_base, n_streams, (int64_t)row, 1, samples_per_stream, n_units);
        a.samples = g_call.d_in();
        a.stage_elems = (int)(row * n_streams);
        a.n_chains = n_streams;
        a.filter_count = 5;
        a.range = 12;
        a.states_out = g_call.d_states();
        a.spu_out = g_call.d_out();
        HIP_TRY(psxhip_adpcm_call_launch(&a, g_call.stream), PSXHIP_EDEVICE);
        HIP_TRY(hipStreamSynchronize(g_call.stream), PSXHIP_EDEVICE);
        for (int i = 0; i < n_streams; i++) {
            memcpy(out + (size_t)i * (size_t)p.out_stride, g_call.out() + (size_t)i * bytes, (size_t)bytes);
            states[i] = g_call.states()[i];
        }
        return bytes;
    }

    std::vector<psxhip_adpcm_chain_t> chains(n_streams);
    std::vector<int32_t> base(n_streams);
    fill_planar_chains(chains.data(), base.data(), n_streams, (int64_t)p.per, pitch, samples_per_stream, n_units);
    g_pool_device = device;
    DevBuf d_s(0), d_c(1), d_b(2), d_st(3), d_u(4), d_o(5);
    HIP_TRY(d_s.alloc(p.sample_bytes), PSXHIP_ENOMEM);
    HIP_TRY(d_c.alloc(p.chain_bytes), PSXHIP_ENOMEM);
    HIP_TRY(d_b.alloc(p.base_bytes), PSXHIP_ENOMEM);
    HIP_TRY(d_st.alloc(p.state_bytes), PSXHIP_ENOMEM);
    HIP_TRY(d_u.alloc(p.unit_bytes), PSXHIP_ENOMEM);
    HIP_TRY(d_o.alloc(p.out_bytes), PSXHIP_ENOMEM);
    hipStream_t st = nullptr;
    HIP_TRY(hipMemsetAsync(d_s.p, 0, p.sample_bytes, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpy2DAsync(d_s.p, p.per * sizeof(int16_t), samples, (size_t)p.stream_stride * sizeof(int16_t),
                             p.readable * sizeof(int16_t), (size_t)n_streams, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d_c.p, chains.data(), p.chain_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d_b.p, base.data(), p.base_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d_st.p, states, p.state_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    rc = encode_batch_chains(device, d_s.as<int16_t>(), chains, base, d_c.as<psxhip_adpcm_chain_t>(), d_b.as<int32_t>(), n_units, 4, 5, 4, beam,
                             d_st.as<psxhip_adpcm_state_t>(), d_u.as<uint8_t>(), st);
    if (rc) return rc;
    rc = psxhip_spu_pack_device(device, d_u.as<uint8_t>(), n_streams * n_units, d_o.as<uint8_t>(), st);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)p.out_stride, d_o.p, (size_t)bytes, (size_t)bytes, (size_t)n_streams,
                             hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(states, d_st.p, p.state_bytes, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return bytes;
}

extern "C" int psxhip_spu_encode_streams_host(int device, const int16_t* samples, int n_streams, int64_t stream_stride,
                                              int pitch, int samples_per_stream, psxhip_adpcm_state_t* states,
                                              uint8_t* out, int64_t out_stride) {
    return spu_encode_streams(device, samples, n_streams, stream_stride, pitch, samples_per_stream, states, out, out_stride, 0);
}

extern "C" int psxhip_spu_encode_streams_host_beam(int device, const int16_t* samples, int n_streams, int64_t stream_stride,
                                                   int pitch, int samples_per_stream, psxhip_adpcm_state_t* states,
                                                   uint8_t* out, int64_t out_stride, int beam) {
    if (adpcm_host_beam_check("spu_encode_streams_host_beam", beam)) return PSXHIP_EINVAL;
    return spu_encode_streams(device, samples, n_streams, stream_stride, pitch, samples_per_stream, states, out, out_stride, beam);
}

static int xa_encode_streams(int device, int format, int stereo, int frequency, int bits, int file_number, int channel_number,
                             const int16_t* samples, int n_streams, int64_t stream_stride, int samples_per_stream, const int32_t* lbas,
                             psxhip_adpcm_state_t* states, uint8_t* out, int64_t out_stride, int finalize, const uint8_t* eof_flags, int beam);

extern "C" int psxhip_xa_encode_streams_host_beam(int device, int format, int stereo, int frequency, int bits, int file_number,
                                                  int channel_number, const int16_t* samples, int n_streams, int64_t stream_stride,
                                                  int samples_per_stream, const int32_t* lbas, psxhip_adpcm_state_t* states,
                                                  uint8_t* out, int64_t out_stride, int finalize, int beam) {
    if (adpcm_host_beam_check("xa_encode_streams_host_beam", beam)) return PSXHIP_EINVAL;
    return xa_encode_streams(device, format, stereo, frequency, bits, file_number, channel_number, samples, n_streams, stream_stride,
                             samples_per_stream, lbas, states, out, out_stride, finalize, nullptr, beam);
}

extern "C" int psxhip_xa_encode_streams_host(int device, int format, int stereo, int frequency, int bits, int file_number,
                                             int channel_number, const int16_t* samples, int n_streams,
                                             int64_t stream_stride, int samples_per_stream, const int32_t* lbas,
                                             psxhip_adpcm_state_t* states, uint8_t* out, int64_t out_stride, int finalize) {
    return psxhip_xa_encode_streams_host_flags(device, format, stereo, frequency, bits, file_number, channel_number, samples, n_streams,
                                               stream_stride, samples_per_stream, lbas, states, out, out_stride, finalize, nullptr);
}

// eof_flags (optional, n_streams x sectors): which sectors get the EOF submode bit -- the reference's encode_file_str
// finalises EVERY audio sector once its decoder has seen the end of the input (filefmt.c:492-493), not only the last one
extern "C" int psxhip_xa_encode_streams_host_flags(int device, int format, int stereo, int frequency, int bits, int file_number,
                                                   int channel_number, const int16_t* samples, int n_streams,
                                                   int64_t stream_stride, int samples_per_stream, const int32_t* lbas,
                                                   psxhip_adpcm_state_t* states, uint8_t* out, int64_t out_stride, int finalize,
                                                   const uint8_t* eof_flags) {
    return xa_encode_streams(device, format, stereo, frequency, bits, file_number, channel_number, samples, n_streams, stream_stride,
                             samples_per_stream, lbas, states, out, out_stride, finalize, eof_flags, 0);
}

static int xa_encode_streams(int device, int format, int stereo, int frequency, int bits, int file_number, int channel_number,
                             const int16_t* samples, int n_streams, int64_t stream_stride, int samples_per_stream, const int32_t* lbas,
                             psxhip_adpcm_state_t* states, uint8_t* out, int64_t out_stride, int finalize, const uint8_t* eof_flags, int beam) {
    XaEncodeShape p;
    int rc = xa_encode_shape(samples && states && out, format, stereo, bits, n_streams, stream_stride, samples_per_stream, out_stride, &p);
    if (rc) return rc;
    const XaLayout& xa = p.xa;
    const int ch = xa.channels, sectors = p.sectors, bytes = p.bytes, units_per_stream = p.units_per_stream;
    const size_t per = p.per;
    if (p.empty) return bytes;
    if ((rc = psxhip_ensure_device(device))) return rc;

    // ---- the reference's call pattern (one stream, a sector or two per call, filefmt.c:184,476-491): chains + assembly, two
    //      launches, no copies (see CallScratch)
    if (xa_call_fast_path(beam, n_streams, sectors, per, (size_t)bytes, kAdpcmCallStageMax, CallScratch::kOut) && g_call.ready(device)) {
        g_pool_device = device;
        DevBuf d_u(4);
        HIP_TRY(d_u.alloc((size_t)units_per_stream * PSXHIP_ADPCM_RECORD_BYTES), PSXHIP_ENOMEM);
        psxhip_adpcm_call_job_t a;
        memset(&a, 0, sizeof a);
        const size_t row = p.row;
        memcpy(g_call.in(), samples, per * sizeof(int16_t));
        memset(g_call.in() + per, 0, (row - per) * sizeof(int16_t));
        fill_interleaved_chains(a.chains, a.unit_base, 1, ch, 0, samples_per_stream, units_per_stream);
        for (int c = 0; c < ch; c++) a.states_in[c] = states[c];
        a.samples = g_call.d_in();
        a.stage_elems = (int)row;
        a.n_chains = ch;
        a.filter_count = 4;
        a.range = bits == 4 ? 12 : 8;
        a.states_out = g_call.d_states();
        a.units = d_u.as<uint8_t>();
        const uint32_t eof_bits = xa_encode_eof_bits(sectors, eof_flags, finalize);
        HIP_TRY(psxhip_adpcm_call_launch(&a, g_call.stream), PSXHIP_EDEVICE);
        rc = psxhip_xa_assemble_scatter(device, d_u.as<uint8_t>(), sectors, format, stereo, frequency, bits, file_number, channel_number,
                                        lbas ? lbas[0] : 0, nullptr, eof_bits, g_call.d_out(), nullptr, 1, 0, 0, g_call.stream);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(g_call.stream), PSXHIP_EDEVICE);
        memcpy(out, g_call.out(), (size_t)bytes);
        for (int c = 0; c < ch; c++) states[c] = g_call.states()[c];
        return bytes;
    }
    std::vector<psxhip_adpcm_chain_t> chains(p.n_chains);
    std::vector<int32_t> base(p.n_chains);
    fill_interleaved_chains(chains.data(), base.data(), n_streams, ch, (int64_t)per, samples_per_stream, units_per_stream);
    const std::vector<uint8_t> eof = xa_encode_eof_table(n_streams, sectors, eof_flags, finalize);

    g_pool_device = device;
    DevBuf d_s(0), d_c(1), d_b(2), d_st(3), d_u(4), d_o(5), d_e(6);
    HIP_TRY(d_s.alloc(p.sample_bytes), PSXHIP_ENOMEM);
    HIP_TRY(d_c.alloc(p.chain_bytes), PSXHIP_ENOMEM);
    HIP_TRY(d_b.alloc(p.base_bytes), PSXHIP_ENOMEM);
    HIP_TRY(d_st.alloc(p.state_bytes), PSXHIP_ENOMEM);
    HIP_TRY(d_u.alloc(p.unit_bytes), PSXHIP_ENOMEM);
    HIP_TRY(d_o.alloc(p.out_bytes), PSXHIP_ENOMEM);
    HIP_TRY(d_e.alloc(p.eof_bytes), PSXHIP_ENOMEM);
    hipStream_t st = nullptr;
    if (per)
        HIP_TRY(hipMemcpy2DAsync(d_s.p, per * sizeof(int16_t), samples, (size_t)p.stream_stride * sizeof(int16_t),
                                 per * sizeof(int16_t), (size_t)n_streams, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d_c.p, chains.data(), p.chain_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d_b.p, base.data(), p.base_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d_st.p, states, p.state_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(d_e.p, eof.data(), p.eof_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    rc = encode_batch_chains(device, d_s.as<int16_t>(), chains, base, d_c.as<psxhip_adpcm_chain_t>(), d_b.as<int32_t>(), p.units_per_chain,
                             beam ? 4 : 5, 4, bits, beam, d_st.as<psxhip_adpcm_state_t>(), d_u.as<uint8_t>(), st);
    if (rc) return rc;
    for (int i = 0; i < n_streams; i++) {
        rc = psxhip_xa_assemble_device(device, d_u.as<uint8_t>() + (size_t)i * units_per_stream * xa.record_bytes,
                                       sectors, format, stereo, frequency, bits, file_number, channel_number,
                                       lbas ? lbas[i] : 0, d_e.as<uint8_t>() + (size_t)i * sectors,
                                       d_o.as<uint8_t>() + (size_t)i * bytes, st);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)p.out_stride, d_o.p, (size_t)bytes, (size_t)bytes, (size_t)n_streams,
                             hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpyAsync(states, d_st.p, p.state_bytes, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return bytes;
}
