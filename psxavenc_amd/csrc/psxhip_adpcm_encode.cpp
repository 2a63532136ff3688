// psxhip_adpcm_encode.cpp -- the device-level entry points of the ADPCM encoder (include/psxav_hip.h): the speculate-and-verify
// session, the SPU pack and XA sector assembly calls.  What they refuse, the session's chunk tables and the carving of its block are
// adpcm_plan.cpp's, without HIP; here the plans are executed: the kernels' job structs filled and launched (adpcm_kernels.hip,
// adpcm_beam_kernels.hip, sector_kernels.hip).  No encoding happens on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "adpcm_plan.h"
#include "psxhip_adpcm_internal.h"
#include "psxhip_internal.h"
#include "verify_passes.h"

static_assert(kVerifyBatchMax == kAdpcmVerifyBatchMax, "the session's block holds verify_passes.h's flag words");

static void fill_chain_job(psxhip_adpcm_chain_job_t* job, const int16_t* d_samples, const psxhip_adpcm_chain_t* d_chains, const int32_t* d_unit_base,
                           int n_chains, int filter_count, int bits, psxhip_adpcm_state_t* d_states, uint8_t* d_units) {
    job->samples = d_samples;
    job->chains = d_chains;
    job->unit_base = d_unit_base;
    job->n_chains = n_chains;
    job->filter_count = filter_count;
    job->range = bits == 4 ? 12 : 8;
    job->states = d_states;
    job->units = d_units;
}

extern "C" int psxhip_adpcm_encode_chains_device(int device, const int16_t* d_samples, const psxhip_adpcm_chain_t* d_chains,
                                                 const int32_t* d_unit_base, int n_chains, int filter_count, int bits,
                                                 psxhip_adpcm_state_t* d_states, uint8_t* d_units, void* stream) {
    int rc = adpcm_encode_chains_check(kEncodeChains, (uintptr_t)d_samples, (uintptr_t)d_chains, (uintptr_t)d_unit_base, (uintptr_t)d_states,
                                       (uintptr_t)d_units, n_chains, filter_count, bits, 0, 0);
    if (rc) return rc;
    rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_chains == 0) return PSXHIP_OK;
    psxhip_adpcm_chain_job_t job;
    fill_chain_job(&job, d_samples, d_chains, d_unit_base, n_chains, filter_count, bits, d_states, d_units);
    HIP_TRY(psxhip_adpcm_chains_launch(&job, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

// "psxhip ADPCM beam v1" (DESIGN.md section 22): the contract of the call above, a beam of 1 .. 4 paths per candidate, and optionally
// the winner's squared error per record index
extern "C" int psxhip_adpcm_beam_encode_chains_device(int device, const int16_t* d_samples, const psxhip_adpcm_chain_t* d_chains,
                                                      const int32_t* d_unit_base, int n_chains, int filter_count, int bits, int beam,
                                                      psxhip_adpcm_state_t* d_states, uint8_t* d_units, uint32_t* d_unit_err, void* stream) {
    int rc = adpcm_encode_chains_check(kBeamEncodeChains, (uintptr_t)d_samples, (uintptr_t)d_chains, (uintptr_t)d_unit_base, (uintptr_t)d_states,
                                       (uintptr_t)d_units, n_chains, filter_count, bits, beam, (uintptr_t)d_unit_err);
    if (rc) return rc;
    rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_chains == 0) return PSXHIP_OK;
    psxhip_adpcm_beam_chain_job_t bj;
    fill_chain_job(&bj.job, d_samples, d_chains, d_unit_base, n_chains, filter_count, bits, d_states, d_units);
    bj.beam = beam;
    bj.unit_err = d_unit_err;
    HIP_TRY(psxhip_adpcm_beam_chains_launch(&bj, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

namespace {
// A session owns one block of device memory.  The one-call entry points (psxhip_adpcm_encode_chains_chunked and the *_host
// wrappers above it) build and drop a session per call, and a hipMalloc / hipFree pair costs more than encoding a
// minute of audio: freed blocks are parked per host thread and handed out again (smallest block that fits and is not more
// than four times too large).  psxhip_adpcm_release_blocks() empties the cache, and so does the thread's end.  A session
// synchronises its stream before it lets go of its block, so a parked block has no work in flight.
struct BlockCache {
    static constexpr int kMax = 32;
    struct Entry { void* p; size_t cap; int device; };
    Entry e[kMax];
    int n = 0;
    void* take(size_t need, int device, size_t* cap) {
        int best = -1;
        for (int i = 0; i < n; i++)
            if (e[i].device == device && e[i].cap >= need && e[i].cap <= 4 * need + 4096 && (best < 0 || e[i].cap < e[best].cap)) best = i;
        if (best < 0) return nullptr;
        void* p = e[best].p;
        *cap = e[best].cap;
        e[best] = e[--n];
        return p;
    }
    bool park(void* p, size_t cap, int device) {
        if (n == kMax) return false;
        e[n++] = Entry{p, cap, device};
        return true;
    }
    void release() {
        for (int i = 0; i < n; i++) (void)hipFree(e[i].p);
        n = 0;
    }
    ~BlockCache() { release(); }
};
thread_local BlockCache g_blocks;
}  // namespace

extern "C" void psxhip_adpcm_release_blocks(void) { g_blocks.release(); }

struct psxhip_adpcm_session {
    int device, n_chains, n_chunks;
    int beam = 0;               // 0: the plain encoder's kernels; 1 .. 4: adpcm_beam_kernels.hip (psxhip_adpcm_session_set_beam)
    bool speculated;
    hipStream_t stream;
    psxhip_adpcm_chunk_job_t job;
    // the block (from g_blocks, parked there again) and what lies in it besides the job's tables.  A block from the cache holds stale
    // bytes: everything a kernel reads is copied in by create / run or written by an earlier kernel of the same run
    uint8_t* block = nullptr;
    size_t block_cap = 0;
    psxhip_adpcm_state_t *d_cstates = nullptr, *d_final = nullptr;
    uint8_t* d_known = nullptr;
    int* d_flags = nullptr;
    int* h_flags = nullptr;     // page-locked: the verify passes' "changed" words travel back through it (a session's runs are serialised)
    // optional (psxhip_adpcm_session_set_timing): HIP events around the speculate launch and the verify passes of a run
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool timing = false;
    float spec_ms = 0.0f, verify_ms = 0.0f;
    ~psxhip_adpcm_session() {
        if (block && !g_blocks.park(block, block_cap, device)) (void)hipFree(block);
        if (h_flags) (void)hipHostFree(h_flags);
        for (int i = 0; i < 3; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
};

extern "C" int psxhip_adpcm_session_create(psxhip_adpcm_session_t** out, int device, const int16_t* d_samples,
                                           const psxhip_adpcm_chain_t* chains, const int32_t* unit_base,
                                           const int32_t* lead_units, int n_chains, int filter_count, int bits,
                                           uint8_t* d_units, int chunk_units, int warmup_units, void* stream) {
    if (!out) return PSXHIP_EINVAL;
    *out = nullptr;
    int rc = adpcm_session_create_check((uintptr_t)d_samples, chains != nullptr, unit_base != nullptr, (uintptr_t)d_units, n_chains, filter_count, bits,
                                        chunk_units, warmup_units);
    if (rc) return rc;
    rc = psxhip_ensure_device(device);
    if (rc) return rc;
    struct Guard {                       // frees the half-built session on every early return
        psxhip_adpcm_session* p;
        ~Guard() { delete p; }
    } guard{new psxhip_adpcm_session()};
    psxhip_adpcm_session* s = guard.p;
    s->device = device;
    s->n_chains = n_chains;
    s->speculated = false;
    s->stream = (hipStream_t)stream;

    AdpcmSessionPlan p;
    adpcm_session_plan(chains, lead_units, n_chains, chunk_units, &p);
    s->n_chunks = p.n_chunks;
    const size_t nc = (size_t)n_chains, nk = (size_t)p.n_chunks;
    s->block = (uint8_t*)g_blocks.take(p.bytes, device, &s->block_cap);
    if (!s->block) {
        void* fresh = nullptr;
        HIP_TRY(hipMalloc(&fresh, p.bytes), PSXHIP_ENOMEM);
        s->block = (uint8_t*)fresh;
        s->block_cap = p.bytes;
    }
    uint8_t* const d = s->block;
    hipStream_t st = s->stream;
    if (n_chains) {
        HIP_TRY(hipMemcpyAsync(d + p.o_chains, chains, sizeof(psxhip_adpcm_chain_t) * nc, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
        HIP_TRY(hipMemcpyAsync(d + p.o_base, unit_base, sizeof(int32_t) * nc, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
        HIP_TRY(hipMemcpyAsync(d + p.o_sbase, p.state_base.data(), sizeof(int64_t) * nc, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
        HIP_TRY(hipMemcpyAsync(d + p.o_lead, p.lead.data(), sizeof(int32_t) * nc, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    }
    if (s->n_chunks) {
        HIP_TRY(hipMemcpyAsync(d + p.o_cchain, p.chunk_chain.data(), sizeof(int32_t) * nk, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
        HIP_TRY(hipMemcpyAsync(d + p.o_cfirst, p.chunk_first.data(), sizeof(int32_t) * nk, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    }
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);    // the host vectors go out of scope

    psxhip_adpcm_chunk_job_t& job = s->job;
    job.samples = d_samples;
    job.chains = (const psxhip_adpcm_chain_t*)(d + p.o_chains);
    job.unit_base = (const int32_t*)(d + p.o_base);
    job.state_base = (const int64_t*)(d + p.o_sbase);
    job.chunk_chain = (const int32_t*)(d + p.o_cchain);
    job.chunk_first = (const int32_t*)(d + p.o_cfirst);
    job.n_chunks = s->n_chunks;
    job.chunk_units = chunk_units;
    job.warmup_units = warmup_units;
    job.filter_count = filter_count;
    job.range = bits == 4 ? 12 : 8;
    job.chain_states = s->d_cstates = (psxhip_adpcm_state_t*)(d + p.o_cstates);
    job.lead_units = (const int32_t*)(d + p.o_lead);
    job.start_known = s->d_known = d + p.o_known;
    job.unit_states = (psxhip_adpcm_state_t*)(d + p.o_ustates);
    job.start_used = (psxhip_adpcm_state_t*)(d + p.o_used);
    job.units = d_units;
    job.changed = nullptr;      // set by session_run, per pass
    job.changed_before = nullptr;
    s->d_final = (psxhip_adpcm_state_t*)(d + p.o_final);
    s->d_flags = (int*)(d + p.o_flags);
    guard.p = nullptr;                   // ownership passes to the caller
    *out = s;
    return PSXHIP_OK;
}

// HIP events around the speculate launch and around the verify passes of every run that speculates (i.e. the first run after a
// create / reset): bench.py's live kernel-level timing.  The events cost two extra packets per run; off by default.
extern "C" int psxhip_adpcm_session_set_timing(psxhip_adpcm_session_t* s, int on) {
    if (!s) return PSXHIP_EINVAL;
    if (on && !s->ev[0]) {
        HIP_TRY(hipSetDevice(s->device), PSXHIP_EDEVICE);
        for (int i = 0; i < 3; i++) HIP_TRY(hipEventCreate(&s->ev[i]), PSXHIP_EDEVICE);
    }
    s->timing = on != 0;
    return PSXHIP_OK;
}
extern "C" int psxhip_adpcm_session_last_timing(const psxhip_adpcm_session_t* s, float* speculate_ms, float* verify_ms) {
    if (!s) return PSXHIP_EINVAL;
    if (speculate_ms) *speculate_ms = s->spec_ms;
    if (verify_ms) *verify_ms = s->verify_ms;
    return PSXHIP_OK;
}
extern "C" const char* psxhip_adpcm_kernel_rev(void) { return PSXHIP_ADPCM_KERNEL_REV; }
extern "C" const char* psxhip_adpcm_beam_kernel_rev(void) { return PSXHIP_ADPCM_BEAM_KERNEL_REV; }

// Which unit encoder the session's launches run: 0 the plain one (the default), 1 .. 4 the beam.  The records a session holds come
// from one encoder: the width is set before the first run or after a reset, not in between.
extern "C" int psxhip_adpcm_session_set_beam(psxhip_adpcm_session_t* s, int beam) {
    const int rc = adpcm_session_beam_check(s != nullptr, beam, s && s->speculated);
    if (rc) return rc;
    s->beam = beam;
    return PSXHIP_OK;
}

// one speculate (verify = 0) or verify launch of the session's job with the unit encoder the session was given
static hipError_t session_launch(psxhip_adpcm_session* s, int verify, hipStream_t st) {
    if (s->beam == 0) return psxhip_adpcm_chunks_launch(&s->job, verify, st);
    psxhip_adpcm_beam_chunk_job_t bj;
    bj.job = s->job;
    bj.beam = s->beam;
    bj.unit_err = nullptr;
    return psxhip_adpcm_beam_chunks_launch(&bj, verify, st);
}

extern "C" void psxhip_adpcm_session_reset(psxhip_adpcm_session_t* s) {
    if (s) s->speculated = false;        // the next run speculates again from scratch (same block, same chunk tables)
}

extern "C" void psxhip_adpcm_session_destroy(psxhip_adpcm_session_t* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    delete s;
}

extern "C" int psxhip_adpcm_session_run(psxhip_adpcm_session_t* s, const psxhip_adpcm_state_t* start_states,
                                        const uint8_t* start_known, int max_passes, psxhip_adpcm_state_t* final_states,
                                        int* any_change) {
    if (!s || !start_states) {
        psxhip_set_error("adpcm_session_run: NULL argument");
        return PSXHIP_EINVAL;
    }
    if (any_change) *any_change = 0;
    HIP_TRY(hipSetDevice(s->device), PSXHIP_EDEVICE);
    hipStream_t st = s->stream;
    if (s->n_chains == 0) return 0;
    const size_t states_bytes = sizeof(psxhip_adpcm_state_t) * (size_t)s->n_chains;
    HIP_TRY(hipMemcpyAsync(s->d_cstates, start_states, states_bytes, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    if (start_known) HIP_TRY(hipMemcpyAsync(s->d_known, start_known, (size_t)s->n_chains, hipMemcpyHostToDevice, st), PSXHIP_EDEVICE);
    else HIP_TRY(hipMemsetAsync(s->d_known, 1, (size_t)s->n_chains, st), PSXHIP_EDEVICE);
    int passes = 0;
    if (s->n_chunks) {
        // the verify passes' words travel back through a page-locked buffer owned by the session (a run is synchronous; a buffer per
        // calling thread leaked one per worker thread of the multi-device calls)
        if (!s->h_flags && hipHostMalloc((void**)&s->h_flags, kVerifyBatchMax * sizeof(int), hipHostMallocDefault) != hipSuccess) {
            s->h_flags = nullptr;
            psxhip_set_error("adpcm_session_run: no page-locked memory for the verify flags");
            return PSXHIP_ENOMEM;
        }
        const bool timed = s->timing && !s->speculated;
        bool changed = false;
        if (!s->speculated) {
            s->job.changed = s->d_flags;
            s->job.changed_before = nullptr;
            if (timed) HIP_TRY(hipEventRecord(s->ev[0], st), PSXHIP_EDEVICE);
            HIP_TRY(session_launch(s, 0, st), PSXHIP_EDEVICE);
            if (timed) HIP_TRY(hipEventRecord(s->ev[1], st), PSXHIP_EDEVICE);
            s->speculated = true;
            if (any_change) *any_change = 1;
        }
        passes = run_verify_passes(
            [&](int* flag, const int* flag_before) {
                s->job.changed = flag;
                s->job.changed_before = flag_before;
                return session_launch(s, 1, st);
            },
            s->d_flags, s->h_flags, st, max_passes, "adpcm_session_run", &changed);
        if (passes < 0) return passes;
        if (changed && any_change) *any_change = 1;
        if (timed) {
            HIP_TRY(hipEventRecord(s->ev[2], st), PSXHIP_EDEVICE);
            HIP_TRY(hipEventSynchronize(s->ev[2]), PSXHIP_EDEVICE);
            HIP_TRY(hipEventElapsedTime(&s->spec_ms, s->ev[0], s->ev[1]), PSXHIP_EDEVICE);
            HIP_TRY(hipEventElapsedTime(&s->verify_ms, s->ev[1], s->ev[2]), PSXHIP_EDEVICE);
        }
    }
    // chains without units keep their start state
    HIP_TRY(hipMemcpyAsync(s->d_final, s->d_cstates, states_bytes, hipMemcpyDeviceToDevice, st), PSXHIP_EDEVICE);
    HIP_TRY(psxhip_adpcm_final_states_launch(s->job.chains, s->job.state_base, s->n_chains, s->job.unit_states, s->d_final, st), PSXHIP_EDEVICE);
    if (final_states) HIP_TRY(hipMemcpyAsync(final_states, s->d_final, states_bytes, hipMemcpyDeviceToHost, st), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), PSXHIP_EDEVICE);
    return passes;
}

// the chunked call with either unit encoder (the plain entry: beam 0)
static int encode_chains_chunked(bool beam_entry, int device, const int16_t* d_samples, const psxhip_adpcm_chain_t* chains, const int32_t* unit_base,
                                 int n_chains, int filter_count, int bits, int beam, psxhip_adpcm_state_t* d_states, uint8_t* d_units,
                                 int chunk_units, int warmup_units, int max_passes, void* stream) {
    int rc = adpcm_encode_chunked_check(beam_entry, beam, (uintptr_t)d_states);
    if (rc) return rc;
    if (n_chains == 0) return 0;
    psxhip_adpcm_session_t* s = nullptr;
    rc = psxhip_adpcm_session_create(&s, device, d_samples, chains, unit_base, nullptr, n_chains, filter_count, bits, d_units,
                                         chunk_units, warmup_units, stream);
    if (rc) return rc;
    s->beam = beam;
    // d_states travels on the caller's stream, like everything else here: earlier work on that stream may still be writing it (a serial
    // psxhip_adpcm_encode_chains_device, say), and a copy on the null stream does not wait for a non-blocking stream
    std::vector<psxhip_adpcm_state_t> st((size_t)n_chains);
    const size_t states_bytes = sizeof(psxhip_adpcm_state_t) * (size_t)n_chains;
    hipStream_t hs = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(st.data(), d_states, states_bytes, hipMemcpyDeviceToHost, hs);
    if (e == hipSuccess) e = hipStreamSynchronize(hs);
    int passes = PSXHIP_EDEVICE;
    if (e == hipSuccess) {
        passes = psxhip_adpcm_session_run(s, st.data(), nullptr, max_passes, st.data(), nullptr);
        if (passes >= 0) {
            e = hipMemcpyAsync(d_states, st.data(), states_bytes, hipMemcpyHostToDevice, hs);
            if (e == hipSuccess) e = hipStreamSynchronize(hs);       // the call synchronises (and `st` goes out of scope)
        }
    }
    psxhip_adpcm_session_destroy(s);
    if (e != hipSuccess) {
        psxhip_set_error("adpcm_encode_chains_chunked: state copy failed: %s", hipGetErrorString(e));
        return PSXHIP_EDEVICE;
    }
    return passes;
}

extern "C" int psxhip_adpcm_encode_chains_chunked(int device, const int16_t* d_samples, const psxhip_adpcm_chain_t* chains,
                                                  const int32_t* unit_base, int n_chains, int filter_count, int bits,
                                                  psxhip_adpcm_state_t* d_states, uint8_t* d_units, int chunk_units,
                                                  int warmup_units, int max_passes, void* stream) {
    return encode_chains_chunked(false, device, d_samples, chains, unit_base, n_chains, filter_count, bits, 0, d_states, d_units, chunk_units,
                                 warmup_units, max_passes, stream);
}

extern "C" int psxhip_adpcm_beam_encode_chains_chunked(int device, const int16_t* d_samples, const psxhip_adpcm_chain_t* chains,
                                                       const int32_t* unit_base, int n_chains, int filter_count, int bits,
                                                       psxhip_adpcm_state_t* d_states, uint8_t* d_units, int beam, int chunk_units,
                                                       int warmup_units, int max_passes, void* stream) {
    return encode_chains_chunked(true, device, d_samples, chains, unit_base, n_chains, filter_count, bits, beam, d_states, d_units, chunk_units,
                                 warmup_units, max_passes, stream);
}

// The one place the unit encoder (beam 0: the plain one) and the route meet, for the host-buffer batches and the sound bank: serial
// under the chain tables on the device, or cut along time under the same tables on the host (that call synchronises).  rows: chunks
// per wavefront of the encoder that runs (adpcm_chunking)
int psxhip_adpcm_encode_routed(int device, const int16_t* d_samples, const psxhip_adpcm_chain_t* chains, const int32_t* unit_base,
                               const psxhip_adpcm_chain_t* d_chains, const int32_t* d_unit_base, int n_chains, bool chunked, long long total_units,
                               int rows, int filter_count, int bits, int beam, psxhip_adpcm_state_t* d_states, uint8_t* d_units, void* stream) {
    if (!chunked)
        return beam ? psxhip_adpcm_beam_encode_chains_device(device, d_samples, d_chains, d_unit_base, n_chains, filter_count, bits, beam, d_states,
                                                             d_units, nullptr, stream)
                    : psxhip_adpcm_encode_chains_device(device, d_samples, d_chains, d_unit_base, n_chains, filter_count, bits, d_states, d_units, stream);
    const AdpcmChunking k = adpcm_chunking(total_units, rows, psxhip_adpcm_device_cus(device));
    const int rc = beam ? psxhip_adpcm_beam_encode_chains_chunked(device, d_samples, chains, unit_base, n_chains, filter_count, bits, d_states, d_units,
                                                                  beam, k.chunk_units, k.warmup_units, 0, stream)
                        : psxhip_adpcm_encode_chains_chunked(device, d_samples, chains, unit_base, n_chains, filter_count, bits, d_states, d_units,
                                                             k.chunk_units, k.warmup_units, 0, stream);
    return rc < 0 ? rc : PSXHIP_OK;
}

extern "C" int psxhip_spu_pack_device(int device, const uint8_t* d_units, int n_blocks, uint8_t* d_out, void* stream) {
    int rc = spu_pack_check((uintptr_t)d_units, n_blocks, (uintptr_t)d_out);
    if (rc) return rc;
    rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_blocks == 0) return PSXHIP_OK;
    HIP_TRY(psxhip_spu_pack_launch(d_units, n_blocks, d_out, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_xa_assemble_device(int device, const uint8_t* d_units, int n_sectors, int format, int stereo,
                                         int frequency, int bits, int file_number, int channel_number, int first_lba,
                                         const uint8_t* d_eof_flags, uint8_t* d_out, void* stream) {
    return psxhip_xa_assemble_scatter(device, d_units, n_sectors, format, stereo, frequency, bits, file_number, channel_number, first_lba,
                                      d_eof_flags, 0u, d_out, nullptr, 1, 0, 0, stream);
}

// ... n_streams streams of n_sectors sectors each (unit records units_stream_stride bytes apart, outputs out_stream_stride apart), every
// sector s written to slot d_dst_sector[s] of its stream's output (NULL: slot s), its header address first_lba + that slot
extern "C" int psxhip_xa_assemble_scatter(int device, const uint8_t* d_units, int n_sectors, int format, int stereo,
                                          int frequency, int bits, int file_number, int channel_number, int first_lba,
                                          const uint8_t* d_eof_flags, uint32_t eof_bits, uint8_t* d_out, const int32_t* d_dst_sector,
                                          int n_streams, size_t units_stream_stride, size_t out_stream_stride, void* stream) {
    int rc = xa_assemble_check((uintptr_t)d_units, (uintptr_t)d_out, n_sectors, n_streams, format, bits, units_stream_stride, out_stream_stride);
    if (rc) return rc;
    rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_sectors == 0) return PSXHIP_OK;
    rc = psxhip_sector_tables(device);
    if (rc) return rc;
    psxhip_xa_job_t job;
    job.units = d_units;
    job.n_sectors = n_sectors;
    job.format = format;
    job.stereo = stereo;
    job.frequency = frequency;
    job.bits = bits;
    job.file_number = file_number;
    job.channel_number = channel_number;
    job.first_lba = first_lba;
    job.eof_flags = d_eof_flags;
    job.eof_bits = eof_bits;
    job.out = d_out;
    job.dst_sector = d_dst_sector;
    job.units_stream_stride = units_stream_stride;
    job.out_stream_stride = out_stream_stride;
    HIP_TRY(psxhip_xa_assemble_launch(&job, n_streams, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}
