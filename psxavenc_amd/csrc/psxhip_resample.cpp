// psxhip_resample.cpp -- host side of the audio front-end (psxhip_resampler_*, include/psxav_hip.h): the
// filter design in double, the handle with its stream counters and history double buffer, and the launch
// (audio_frontend_kernels.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "device_buffer.h"
#include "psxhip_internal.h"

namespace {

constexpr int kFilterSize = 32;         // libswresample's defaults: filter_size, phase_shift (1 << 10 phases), cutoff, Kaiser beta
constexpr int kMaxPhases = 1 << 10;
constexpr double kCutoff = 0.97;
constexpr double kBeta = 9.0;
constexpr int64_t kLaunchMaxIn = 1 << 28;   // new samples per launch (longer calls are cut; the history carries across)

struct Design {
    int L, M, P, T, H;
    bool bypass;
    double factor;
};

int64_t gcd64(int64_t a, int64_t b) {
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
}

bool design_params(int src, int dst, Design* d) {
    if (src < 1000 || src > 384000 || dst < 1000 || dst > 384000) return false;
    if ((int64_t)dst * 16 < src || (int64_t)src * 16 < dst) return false;
    const int g = (int)gcd64(src, dst);
    d->L = dst / g;
    d->M = src / g;
    d->bypass = src == dst;
    if (d->bypass) {
        d->P = 1; d->T = 0; d->H = 0; d->factor = 1.0;
        return true;
    }
    d->factor = std::min(kCutoff * dst / src, 1.0);
    int T = (int)std::ceil(kFilterSize / d->factor);
    T += T & 1;
    d->T = T;
    d->H = T / 2;
    d->P = d->L <= kMaxPhases ? d->L : kMaxPhases;
    return true;
}

double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * k);
        sum += term;
        if (term < sum * 1e-17) break;
    }
    return sum;
}

// the Q15 table, [P][T]; false when some half of some phase has sum |h| > 65535
bool design_table(const Design& d, std::vector<int16_t>* out) {
    const int T = d.T, H = d.H;
    out->assign((size_t)d.P * T, 0);
    std::vector<double> h(T);
    std::vector<int> q(T), order(T);
    const double i0b = bessel_i0(kBeta);
    for (int ph = 0; ph < d.P; ph++) {
        double sum = 0.0;
        for (int k = 0; k < T; k++) {
            const double x = k - (H - 1) - (double)ph / d.P;
            const double t = d.factor * x;
            const double sinc = t == 0.0 ? 1.0 : std::sin(M_PI * t) / (M_PI * t);
            const double w = 1.0 - (x / H) * (x / H);
            h[k] = d.factor * sinc * bessel_i0(kBeta * std::sqrt(w > 0.0 ? w : 0.0)) / i0b;
            sum += h[k];
        }
        int total = 0;
        for (int k = 0; k < T; k++) {
            q[k] = (int)std::max(-32768.0, std::min(32767.0, std::nearbyint(h[k] / sum * 32768.0)));   // half to even
            total += q[k];
        }
        // the rounding residue: to the largest tap (lowest k on ties), and on down the taps in that order as far as int16 allows
        int residue = 32768 - total;
        for (int k = 0; k < T; k++) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return q[a] > q[b]; });
        for (int i = 0; i < T && residue; i++) {
            const int k = order[i];
            const int v = std::max(-32768, std::min(32767, q[k] + residue));
            residue -= v - q[k];
            q[k] = v;
        }
        if (residue) return false;
        int lo = 0, hi = 0;
        for (int k = 0; k < T; k++) (k < H ? lo : hi) += std::abs(q[k]);
        if (lo > 65535 || hi > 65535) return false;
        for (int k = 0; k < T; k++) (*out)[(size_t)ph * T + k] = (int16_t)q[k];
    }
    return true;
}

int64_t ceil_div(__int128 a, int64_t b) { return (int64_t)((a + b - 1) / b); }     // a >= 0

// outputs per channel that exist after n samples without flush, and in all after a flush
int64_t avail(const Design& d, int64_t n) { return d.bypass ? n : (n <= d.H ? 0 : ceil_div((__int128)(n - d.H) * d.L, d.M)); }
int64_t total(const Design& d, int64_t n) { return d.bypass ? n : ceil_div((__int128)n * d.L, d.M); }

int sample_bytes(int fmt) { return fmt <= PSXHIP_PCM_S16P ? 2 : 4; }

}  // namespace

struct psxhip_resampler {
    int device, fmt, sch, dch;
    Design d;
    int16_t mix[8][8];
    std::vector<int16_t> table;
    int16_t* d_coef = nullptr;
    int16_t* d_hist = nullptr;       // [2][dch][T - 1]: the current history and the one the next launch writes
    int cur = 0;
    int64_t consumed = 0;
    bool flushed = false;
    int coef_lds = 0, span = 0, grid_max = 1;
    DeviceBuffer d_in, d_out;        // convert_host's staging buffers, grown on demand
};

extern "C" const char* psxhip_resampler_kernel_rev(void) { return PSXHIP_AFE_KERNEL_REV; }

extern "C" int psxhip_resampler_design(int src_rate, int dst_rate, int* phases, int* taps, int16_t* coef, int cap) {
    Design d;
    if (!design_params(src_rate, dst_rate, &d)) {
        psxhip_set_error("psxhip_resampler_design: rates %d -> %d out of range (1 000 .. 384 000 Hz, at most 16x)", src_rate, dst_rate);
        return PSXHIP_EINVAL;
    }
    if (phases) *phases = d.P;
    if (taps) *taps = d.T;
    if (coef && !d.bypass && cap >= d.P * d.T) {
        std::vector<int16_t> t;
        if (!design_table(d, &t)) {
            psxhip_set_error("psxhip_resampler_design: %d -> %d: a half of some phase exceeds the accumulator bound", src_rate, dst_rate);
            return PSXHIP_EINVAL;
        }
        memcpy(coef, t.data(), t.size() * sizeof(int16_t));
    }
    return d.P;
}

extern "C" int64_t psxhip_resampler_output_count(int src_rate, int dst_rate, int64_t consumed, int64_t n_in, int flush) {
    Design d;
    if (!design_params(src_rate, dst_rate, &d) || consumed < 0 || n_in < 0 || consumed > INT64_MAX / 2 - n_in) return PSXHIP_EINVAL;
    return (flush ? total(d, consumed + n_in) : avail(d, consumed + n_in)) - avail(d, consumed);
}

extern "C" void psxhip_resampler_destroy(psxhip_resampler_t* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->d_coef) (void)hipFree(r->d_coef);
    if (r->d_hist) (void)hipFree(r->d_hist);
    delete r;
}

extern "C" int psxhip_resampler_create(psxhip_resampler_t** out, int device, int src_format, int src_channels, int src_rate,
                                       int dst_channels, int dst_rate, const int16_t* mix) {
    if (!out) return PSXHIP_EINVAL;
    *out = nullptr;
    Design d;
    if (src_format < PSXHIP_PCM_S16 || src_format > PSXHIP_PCM_F32P || src_channels < 1 || src_channels > 8 || dst_channels < 1 ||
        dst_channels > 8 || !design_params(src_rate, dst_rate, &d)) {
        psxhip_set_error("psxhip_resampler_create: bad format %d, channels %d -> %d (1 .. 8) or rates %d -> %d (1 000 .. 384 000 Hz, at most 16x)",
                         src_format, src_channels, dst_channels, src_rate, dst_rate);
        return PSXHIP_EINVAL;
    }
    int16_t m[8][8];
    memset(m, 0, sizeof m);
    const int S = src_channels, D = dst_channels;
    if (mix) {
        for (int c = 0; c < D; c++)
            for (int k = 0; k < S; k++) m[c][k] = mix[c * S + k];
    } else if (S == D) {
        for (int c = 0; c < D; c++) m[c][c] = 16384;
    } else if (S == 2 && D == 1) {
        m[0][0] = m[0][1] = 8192;
    } else if (S == 1 && D == 2) {
        m[0][0] = m[1][0] = 16384;
    } else if (S == 6 && D == 2) {             // FL FR FC LFE BL BR (SL SR): LFE dropped
        m[0][0] = 6786; m[0][2] = 4799; m[0][4] = 4799;
        m[1][1] = 6786; m[1][2] = 4799; m[1][5] = 4799;
    } else {
        psxhip_set_error("psxhip_resampler_create: no default matrix for %d -> %d channels", S, D);
        return PSXHIP_EINVAL;
    }
    for (int c = 0; c < D; c++) {
        int s = 0;
        for (int k = 0; k < S; k++) s += std::abs((int)m[c][k]);
        if (s > 65535) {
            psxhip_set_error("psxhip_resampler_create: matrix row %d has sum |m| = %d > 65535", c, s);
            return PSXHIP_EINVAL;
        }
    }
    std::vector<int16_t> table;
    if (!d.bypass && !design_table(d, &table)) {
        psxhip_set_error("psxhip_resampler_create: %d -> %d: a half of some phase exceeds the accumulator bound", src_rate, dst_rate);
        return PSXHIP_EINVAL;
    }
    int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    psxhip_resampler* r = new (std::nothrow) psxhip_resampler;
    if (!r) return PSXHIP_ENOMEM;
    struct Guard { psxhip_resampler* p; ~Guard() { if (p) psxhip_resampler_destroy(p); } } guard{r};
    r->device = device; r->fmt = src_format; r->sch = S; r->dch = D; r->d = d;
    memcpy(r->mix, m, sizeof m);
    r->table.swap(table);
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device), PSXHIP_EDEVICE);
    const int n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const size_t lds_max = prop.maxSharedMemoryPerMultiProcessor;
    size_t lds = 0;
    if (!d.bypass) {
        HIP_TRY(hipMalloc((void**)&r->d_coef, r->table.size() * sizeof(int16_t)), PSXHIP_ENOMEM);
        HIP_TRY(hipMemcpy(r->d_coef, r->table.data(), r->table.size() * sizeof(int16_t), hipMemcpyHostToDevice), PSXHIP_EDEVICE);
        HIP_TRY(hipMalloc((void**)&r->d_hist, 2 * (size_t)D * (d.T - 1) * sizeof(int16_t)), PSXHIP_ENOMEM);
        HIP_TRY(hipMemset(r->d_hist, 0, 2 * (size_t)D * (d.T - 1) * sizeof(int16_t)), PSXHIP_EDEVICE);
        // the input span of a tile: the last output's offset from the first (at most (L - 1 + 255 M) / L samples) plus T
        const int64_t reach = ((int64_t)d.L - 1 + (int64_t)(PSXHIP_AFE_TILE - 1) * d.M) / d.L + d.T;
        r->span = (int)((reach + 1) & ~(int64_t)1);
        // the launch's own LDS size (psxhip_afe_lds_bytes: header, table when in LDS, spans) decides everything below
        psxhip_afe_job_t probe;
        memset(&probe, 0, sizeof probe);
        probe.dch = D; probe.P = d.P; probe.T = d.T; probe.span = r->span;
        probe.coef_lds = (size_t)d.P * d.T * 2 <= 48 * 1024;
        if (psxhip_afe_lds_bytes(&probe) > lds_max) probe.coef_lds = 0;
        r->coef_lds = probe.coef_lds;
        lds = psxhip_afe_lds_bytes(&probe);
        if (lds > lds_max) {
            psxhip_set_error("psxhip_resampler_create: the input span (%zu bytes of LDS) does not fit a compute unit", lds);
            return PSXHIP_EINVAL;
        }
        HIP_TRY(psxhip_afe_prepare(D, r->coef_lds, lds), PSXHIP_EDEVICE);
    }
    // a persistent grid: as many 256-lane groups as the LDS lets a compute unit hold, at most 8 (32 wavefronts)
    const int per_cu = lds ? (int)std::max<size_t>(1, std::min<size_t>(8, lds_max / lds)) : 8;
    r->grid_max = n_cu * per_cu;
    guard.p = nullptr;
    *out = r;
    return PSXHIP_OK;
}

extern "C" void psxhip_resampler_reset(psxhip_resampler_t* r) {
    if (!r) return;
    r->consumed = 0;
    r->flushed = false;
    r->cur = 0;
    if (r->d_hist) {
        (void)hipSetDevice(r->device);
        (void)hipDeviceSynchronize();        // launches still in flight read the history
        (void)hipMemset(r->d_hist, 0, 2 * (size_t)r->dch * (r->d.T - 1) * sizeof(int16_t));
    }
}

namespace {

// one launch: n new samples (src pointers already offset), outputs at d_dst
int launch_one(psxhip_resampler* r, const void* const* src, int64_t n, int16_t* d_dst, int flush, void* stream) {
    const Design& d = r->d;
    const int64_t N0 = r->consumed, N1 = N0 + n;
    const int64_t a0 = avail(d, N0), a1 = flush ? total(d, N1) : avail(d, N1);
    psxhip_afe_job_t j;
    memset(&j, 0, sizeof j);
    const int nsrc = (r->fmt & 1) ? r->sch : 1;
    for (int k = 0; k < nsrc; k++) j.src[k] = src ? src[k] : nullptr;
    j.fmt = r->fmt; j.sch = r->sch; j.dch = r->dch;
    j.bypass = d.bypass;
    j.n_in = n; j.n_out = a1 - a0;
    j.L = d.L; j.M = d.M; j.P = d.P; j.T = d.T; j.H = d.H;
    j.coef = r->d_coef; j.coef_lds = r->coef_lds; j.span = r->span;
    j.dst = d_dst;
    memcpy(j.mix, r->mix, sizeof j.mix);
    int64_t work;
    if (d.bypass) {
        work = (j.n_out + PSXHIP_AFE_TILE - 1) / PSXHIP_AFE_TILE;
        if (!work) return PSXHIP_OK;
    } else {
        const __int128 pos = (__int128)a0 * d.M;
        j.i0 = (int64_t)(pos / d.L) - N0;
        j.r0 = (int)(pos % d.L);
        const size_t hn = (size_t)r->dch * (d.T - 1);
        j.hist_in = r->d_hist + (size_t)r->cur * hn;
        j.hist_out = r->d_hist + (size_t)(r->cur ^ 1) * hn;
        work = (j.n_out + PSXHIP_AFE_TILE - 1) / PSXHIP_AFE_TILE + 1;      // + the history tile
    }
    const int grid = (int)std::min<int64_t>(work, r->grid_max);
    HIP_TRY(psxhip_afe_launch(&j, grid, stream), PSXHIP_EDEVICE);
    if (!d.bypass) r->cur ^= 1;
    r->consumed = N1;
    return PSXHIP_OK;
}

}  // namespace

extern "C" int psxhip_resampler_convert_device(psxhip_resampler_t* r, const void* const* src, int64_t n_in, int16_t* d_dst,
                                               int64_t* n_out, int flush, void* stream) {
    if (n_out) *n_out = 0;
    if (!r || n_in < 0 || (n_in > 0 && !src)) {
        psxhip_set_error("psxhip_resampler_convert_device: NULL argument or negative count");
        return PSXHIP_EINVAL;
    }
    if (r->flushed) {
        psxhip_set_error("psxhip_resampler_convert_device: the stream was flushed; reset the handle first");
        return PSXHIP_EINVAL;
    }
    const int nsrc = (r->fmt & 1) ? r->sch : 1;
    for (int k = 0; n_in > 0 && k < nsrc; k++)
        if (!src[k]) {
            psxhip_set_error("psxhip_resampler_convert_device: source pointer %d is NULL", k);
            return PSXHIP_EINVAL;
        }
    const Design& d = r->d;
    const int64_t count = (flush ? total(d, r->consumed + n_in) : avail(d, r->consumed + n_in)) - avail(d, r->consumed);
    if (count > 0 && !d_dst) {
        psxhip_set_error("psxhip_resampler_convert_device: NULL destination");
        return PSXHIP_EINVAL;
    }
    if (n_in == 0 && !flush) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(r->device), PSXHIP_EDEVICE);
    const int bytes = sample_bytes(r->fmt);
    int64_t done = 0, written = 0;
    do {
        const int64_t n = std::min(n_in - done, kLaunchMaxIn);
        const bool last = done + n == n_in;
        const void* p[8] = {};
        for (int k = 0; n > 0 && k < nsrc; k++)
            p[k] = (const char*)src[k] + (size_t)done * bytes * ((r->fmt & 1) ? 1 : r->sch);
        const int64_t before = avail(d, r->consumed);
        const int64_t after = (last && flush) ? total(d, r->consumed + n) : avail(d, r->consumed + n);
        const int rc = launch_one(r, n > 0 ? p : nullptr, n, d_dst ? d_dst + (size_t)written * r->dch : nullptr, last && flush, stream);
        if (rc) return rc;
        written += after - before;
        done += n;
    } while (done < n_in);
    if (flush) r->flushed = true;
    if (n_out) *n_out = written;
    return PSXHIP_OK;
}

extern "C" int psxhip_resampler_convert_host(psxhip_resampler_t* r, const void* const* src, int64_t n_in, int16_t* dst,
                                             int64_t dst_cap, int64_t* n_out, int flush) {
    if (n_out) *n_out = 0;
    if (!r || n_in < 0 || (n_in > 0 && !src)) return PSXHIP_EINVAL;
    if (r->flushed) {
        psxhip_set_error("psxhip_resampler_convert_host: the stream was flushed; reset the handle first");
        return PSXHIP_EINVAL;
    }
    const Design& d = r->d;
    const int64_t count = (flush ? total(d, r->consumed + n_in) : avail(d, r->consumed + n_in)) - avail(d, r->consumed);
    if (count > dst_cap || (count > 0 && !dst)) {
        psxhip_set_error("psxhip_resampler_convert_host: %lld outputs do not fit dst_cap %lld", (long long)count, (long long)dst_cap);
        return PSXHIP_EINVAL;
    }
    const int nsrc = (r->fmt & 1) ? r->sch : 1;
    const size_t plane = (size_t)n_in * sample_bytes(r->fmt) * ((r->fmt & 1) ? 1 : r->sch);
    for (int k = 0; n_in > 0 && k < nsrc; k++)
        if (!src[k]) return PSXHIP_EINVAL;
    HIP_TRY(hipSetDevice(r->device), PSXHIP_EDEVICE);
    int rc;
    if ((rc = r->d_in.reserve(plane * nsrc)) || (rc = r->d_out.reserve((size_t)count * r->dch * sizeof(int16_t)))) return rc;
    const void* p[8] = {};
    for (int k = 0; n_in > 0 && k < nsrc; k++) {
        p[k] = r->d_in.as<char>() + (size_t)k * plane;
        HIP_TRY(hipMemcpy((void*)p[k], src[k], plane, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    }
    int64_t got = 0;
    rc = psxhip_resampler_convert_device(r, n_in > 0 ? p : nullptr, n_in, r->d_out.as<int16_t>(), &got, flush, nullptr);
    if (rc) return rc;
    if (got) HIP_TRY(hipMemcpy(dst, r->d_out.p, (size_t)got * r->dch * sizeof(int16_t), hipMemcpyDeviceToHost), PSXHIP_EDEVICE);
    HIP_TRY(hipDeviceSynchronize(), PSXHIP_EDEVICE);
    if (n_out) *n_out = got;
    return PSXHIP_OK;
}
