// resample_plan.cpp -- the audio front-end's plans (resample_plan.h): design, counts, refusals, the launch's shape and cut.  No HIP.
#include "resample_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

int64_t gcd64(int64_t a, int64_t b) {
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
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

int64_t ceil_div(__int128 a, int64_t b) { return (int64_t)((a + b - 1) / b); }     // a >= 0

}  // namespace

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

int64_t avail(const Design& d, int64_t n) { return d.bypass ? n : (n <= d.H ? 0 : ceil_div((__int128)(n - d.H) * d.L, d.M)); }
int64_t total(const Design& d, int64_t n) { return d.bypass ? n : ceil_div((__int128)n * d.L, d.M); }

// ---- the two entry points that need no device

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
    return outputs_of(d, consumed, n_in, flush);
}

// ---- create

int resampler_create_plan(int src_format, int src_channels, int src_rate, int dst_channels, int dst_rate, const int16_t* mix, ResamplerPlan* out) {
    Design d;
    if (src_format < PSXHIP_PCM_S16 || src_format > PSXHIP_PCM_F32P || src_channels < 1 || src_channels > 8 || dst_channels < 1 ||
        dst_channels > 8 || !design_params(src_rate, dst_rate, &d)) {
        psxhip_set_error("psxhip_resampler_create: bad format %d, channels %d -> %d (1 .. 8) or rates %d -> %d (1 000 .. 384 000 Hz, at most 16x)",
                         src_format, src_channels, dst_channels, src_rate, dst_rate);
        return PSXHIP_EINVAL;
    }
    int16_t (&m)[8][8] = out->mix;
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
    out->table.clear();
    if (!d.bypass && !design_table(d, &out->table)) {
        psxhip_set_error("psxhip_resampler_create: %d -> %d: a half of some phase exceeds the accumulator bound", src_rate, dst_rate);
        return PSXHIP_EINVAL;
    }
    out->fmt = src_format; out->sch = S; out->dch = D; out->d = d;
    return PSXHIP_OK;
}

int resampler_shape(const Design& d, int dch, size_t lds_per_cu, int n_cu, ResamplerShape* out) {
    *out = ResamplerShape();
    if (!d.bypass) {
        const int64_t reach = ((int64_t)d.L - 1 + (int64_t)(PSXHIP_AFE_TILE - 1) * d.M) / d.L + d.T;
        out->span = (int)((reach + 1) & ~(int64_t)1);
        out->coef_lds = (size_t)d.P * d.T * 2 <= 48 * 1024 && afe_lds_bytes(false, true, d.P, d.T, dch, out->span) <= lds_per_cu;
        out->lds_bytes = afe_lds_bytes(false, out->coef_lds != 0, d.P, d.T, dch, out->span);
        if (out->lds_bytes > lds_per_cu) {
            psxhip_set_error("psxhip_resampler_create: the input span (%zu bytes of LDS) does not fit a compute unit", out->lds_bytes);
            return PSXHIP_EINVAL;
        }
    }
    const int per_cu = out->lds_bytes ? (int)std::max<size_t>(1, std::min<size_t>(8, lds_per_cu / out->lds_bytes)) : 8;
    out->grid_max = n_cu * per_cu;
    return PSXHIP_OK;
}

// ---- convert

int resampler_convert_check(bool host, const ResamplerPlan* p, bool flushed, int64_t consumed, const void* const* src, int64_t n_in, bool dst,
                            int64_t dst_cap, int flush, int64_t* count, bool* go) {
    const char* who = host ? "psxhip_resampler_convert_host" : "psxhip_resampler_convert_device";
    *count = 0;
    *go = false;
    if (!p || n_in < 0 || (n_in > 0 && !src)) {
        if (!host) psxhip_set_error("%s: NULL argument or negative count", who);
        return PSXHIP_EINVAL;
    }
    if (flushed) {
        psxhip_set_error("%s: the stream was flushed; reset the handle first", who);
        return PSXHIP_EINVAL;
    }
    // a NULL source pointer: the device entry looks before it counts, the host entry after
    auto null_source = [&]() {
        for (int k = 0; n_in > 0 && k < resampler_nsrc(p->fmt, p->sch); k++)
            if (!src[k]) {
                if (!host) psxhip_set_error("%s: source pointer %d is NULL", who, k);
                return true;
            }
        return false;
    };
    if (!host && null_source()) return PSXHIP_EINVAL;
    *count = outputs_of(p->d, consumed, n_in, flush);
    if (host ? (*count > dst_cap || (*count > 0 && !dst)) : (*count > 0 && !dst)) {
        if (host) psxhip_set_error("%s: %lld outputs do not fit dst_cap %lld", who, (long long)*count, (long long)dst_cap);
        else psxhip_set_error("%s: NULL destination", who);
        return PSXHIP_EINVAL;
    }
    if (host && null_source()) return PSXHIP_EINVAL;
    *go = host || n_in > 0 || flush;
    return PSXHIP_OK;
}

ResamplerLaunch resampler_launch(const Design& d, int64_t consumed, int64_t left, int flush, int grid_max) {
    ResamplerLaunch l;
    l.n = std::min(left, kLaunchMaxIn);
    l.flush = flush && l.n == left;
    l.n_out = outputs_of(d, consumed, l.n, l.flush);
    l.i0 = 0;
    l.r0 = 0;
    l.work = (l.n_out + PSXHIP_AFE_TILE - 1) / PSXHIP_AFE_TILE;
    if (!d.bypass) {
        const __int128 pos = (__int128)avail(d, consumed) * d.M;
        l.i0 = (int64_t)(pos / d.L) - consumed;
        l.r0 = (int)(pos % d.L);
        l.work++;                       // + the history tile
    }
    l.grid = (int)std::min<int64_t>(l.work, grid_max);
    return l;
}
