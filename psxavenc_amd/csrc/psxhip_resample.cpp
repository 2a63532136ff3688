// psxhip_resample.cpp -- host side of the audio front-end (psxhip_resampler_*, include/psxav_hip.h): the
// handle with its stream counters and history double buffer, the staging of the host entry and the launches
// (audio_frontend_kernels.hip).  The filter design, the counts, the refusals, the launch's shape and cut are resample_plan.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <new>

#include "device_buffer.h"
#include "psxhip_internal.h"
#include "resample_plan.h"

struct psxhip_resampler {
    int device;
    ResamplerPlan p;
    ResamplerShape shape;
    DeviceBuffer d_coef;
    DeviceBuffer d_hist;             // [2][dch][T - 1]: the current history and the one the next launch writes
    int cur = 0;
    int64_t consumed = 0;
    bool flushed = false;
    DeviceBuffer d_in, d_out;        // convert_host's staging buffers, grown on demand

    size_t hist_bytes() const { return 2 * (size_t)p.dch * (p.d.T - 1) * sizeof(int16_t); }
};

extern "C" const char* psxhip_resampler_kernel_rev(void) { return PSXHIP_AFE_KERNEL_REV; }

extern "C" void psxhip_resampler_destroy(psxhip_resampler_t* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    delete r;
}

extern "C" int psxhip_resampler_create(psxhip_resampler_t** out, int device, int src_format, int src_channels, int src_rate,
                                       int dst_channels, int dst_rate, const int16_t* mix) {
    if (!out) return PSXHIP_EINVAL;
    *out = nullptr;
    ResamplerPlan plan;
    int rc = resampler_create_plan(src_format, src_channels, src_rate, dst_channels, dst_rate, mix, &plan);
    if (rc) return rc;
    rc = psxhip_ensure_device(device);
    if (rc) return rc;
    psxhip_resampler* r = new (std::nothrow) psxhip_resampler;
    if (!r) return PSXHIP_ENOMEM;
    struct Guard { psxhip_resampler* p; ~Guard() { if (p) psxhip_resampler_destroy(p); } } guard{r};
    r->device = device;
    r->p = std::move(plan);
    const Design& d = r->p.d;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device), PSXHIP_EDEVICE);
    const int n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (!d.bypass) {
        const size_t table_bytes = r->p.table.size() * sizeof(int16_t);
        if ((rc = r->d_coef.reserve(table_bytes))) return rc;
        HIP_TRY(hipMemcpy(r->d_coef.p, r->p.table.data(), table_bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
        if ((rc = r->d_hist.reserve(r->hist_bytes()))) return rc;
        HIP_TRY(hipMemset(r->d_hist.p, 0, r->hist_bytes()), PSXHIP_EDEVICE);
    }
    if ((rc = resampler_shape(d, r->p.dch, prop.maxSharedMemoryPerMultiProcessor, n_cu, &r->shape))) return rc;
    if (!d.bypass) HIP_TRY(psxhip_afe_prepare(r->p.dch, r->shape.coef_lds, r->shape.lds_bytes), PSXHIP_EDEVICE);
    guard.p = nullptr;
    *out = r;
    return PSXHIP_OK;
}

extern "C" void psxhip_resampler_reset(psxhip_resampler_t* r) {
    if (!r) return;
    r->consumed = 0;
    r->flushed = false;
    r->cur = 0;
    if (r->d_hist.p) {
        (void)hipSetDevice(r->device);
        (void)hipDeviceSynchronize();        // launches still in flight read the history
        (void)hipMemset(r->d_hist.p, 0, r->hist_bytes());
    }
}

namespace {

// one launch: l.n new samples (src pointers already offset), outputs at d_dst
int launch_one(psxhip_resampler* r, const ResamplerLaunch& l, const void* const* src, int16_t* d_dst, void* stream) {
    const ResamplerPlan& p = r->p;
    const Design& d = p.d;
    if (!l.grid) return PSXHIP_OK;
    psxhip_afe_job_t j;
    memset(&j, 0, sizeof j);
    for (int k = 0; k < resampler_nsrc(p.fmt, p.sch); k++) j.src[k] = src ? src[k] : nullptr;
    j.fmt = p.fmt; j.sch = p.sch; j.dch = p.dch;
    j.bypass = d.bypass;
    j.n_in = l.n; j.n_out = l.n_out;
    j.L = d.L; j.M = d.M; j.P = d.P; j.T = d.T; j.H = d.H;
    j.coef = r->d_coef.as<int16_t>(); j.coef_lds = r->shape.coef_lds; j.span = r->shape.span;
    j.dst = d_dst;
    memcpy(j.mix, p.mix, sizeof j.mix);
    if (!d.bypass) {
        j.i0 = l.i0;
        j.r0 = l.r0;
        const size_t hn = (size_t)p.dch * (d.T - 1);
        j.hist_in = r->d_hist.as<int16_t>() + (size_t)r->cur * hn;
        j.hist_out = r->d_hist.as<int16_t>() + (size_t)(r->cur ^ 1) * hn;
    }
    HIP_TRY(psxhip_afe_launch(&j, l.grid, stream), PSXHIP_EDEVICE);
    if (!d.bypass) r->cur ^= 1;
    r->consumed += l.n;
    return PSXHIP_OK;
}

}  // namespace

extern "C" int psxhip_resampler_convert_device(psxhip_resampler_t* r, const void* const* src, int64_t n_in, int16_t* d_dst,
                                               int64_t* n_out, int flush, void* stream) {
    if (n_out) *n_out = 0;
    int64_t count;
    bool go;
    const int bad = resampler_convert_check(false, r ? &r->p : nullptr, r && r->flushed, r ? r->consumed : 0, src, n_in, d_dst != nullptr, 0, flush, &count, &go);
    if (bad || !go) return bad;
    HIP_TRY(hipSetDevice(r->device), PSXHIP_EDEVICE);
    const int nsrc = resampler_nsrc(r->p.fmt, r->p.sch);
    const size_t step = resampler_frame_bytes(r->p.fmt, r->p.sch);
    int64_t done = 0, written = 0;
    do {
        const ResamplerLaunch l = resampler_launch(r->p.d, r->consumed, n_in - done, flush, r->shape.grid_max);
        const void* p[8] = {};
        for (int k = 0; l.n > 0 && k < nsrc; k++) p[k] = (const char*)src[k] + (size_t)done * step;
        const int rc = launch_one(r, l, l.n > 0 ? p : nullptr, d_dst ? d_dst + (size_t)written * r->p.dch : nullptr, stream);
        if (rc) return rc;
        written += l.n_out;
        done += l.n;
    } while (done < n_in);
    if (flush) r->flushed = true;
    if (n_out) *n_out = written;
    return PSXHIP_OK;
}

extern "C" int psxhip_resampler_convert_host(psxhip_resampler_t* r, const void* const* src, int64_t n_in, int16_t* dst,
                                             int64_t dst_cap, int64_t* n_out, int flush) {
    if (n_out) *n_out = 0;
    int64_t count;
    bool go;
    int rc = resampler_convert_check(true, r ? &r->p : nullptr, r && r->flushed, r ? r->consumed : 0, src, n_in, dst != nullptr, dst_cap, flush, &count, &go);
    if (rc) return rc;
    const int nsrc = resampler_nsrc(r->p.fmt, r->p.sch);
    const size_t plane = (size_t)n_in * resampler_frame_bytes(r->p.fmt, r->p.sch);
    HIP_TRY(hipSetDevice(r->device), PSXHIP_EDEVICE);
    if ((rc = r->d_in.reserve(plane * nsrc)) || (rc = r->d_out.reserve((size_t)count * r->p.dch * sizeof(int16_t)))) return rc;
    const void* p[8] = {};
    for (int k = 0; n_in > 0 && k < nsrc; k++) {
        p[k] = r->d_in.as<char>() + (size_t)k * plane;
        HIP_TRY(hipMemcpy((void*)p[k], src[k], plane, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    }
    int64_t got = 0;
    rc = psxhip_resampler_convert_device(r, n_in > 0 ? p : nullptr, n_in, r->d_out.as<int16_t>(), &got, flush, nullptr);
    if (rc) return rc;
    if (got) HIP_TRY(hipMemcpy(dst, r->d_out.p, (size_t)got * r->p.dch * sizeof(int16_t), hipMemcpyDeviceToHost), PSXHIP_EDEVICE);
    HIP_TRY(hipDeviceSynchronize(), PSXHIP_EDEVICE);
    if (n_out) *n_out = got;
    return PSXHIP_OK;
}
