// resample_plan_check.cpp -- runs a table of calls through psxavenc_amd/csrc/resample_plan.cpp and prints what the plans derive, for
// tests/test_resample_plan_cpu.py (restatements, tests/golden/resample_plan_parent.json) and tests/test_gpu_front_end_plan_seams.py.
// Built from resample_plan.cpp and this file alone, with a host compiler: every case is arithmetic.
//
//   resample_plan_check <calls> <blob>
// calls: one call a line, "<kind> <k> <k numbers>"; each kind says below what it takes
// blob:  the coefficient tables "design" makes are appended here as raw int16
// out:   a line of constants, then per call "<kind> : <rc> | <error text>" for a refusal, "<kind> : 0 | device" where the entry point
//        goes on to the device, "<kind> : 0 | early <v>" where it returns v before that, "<kind> : 0 | <numbers>" otherwise.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../psxavenc_amd/csrc/resample_plan.h"

// the error sink: the one symbol the plan module links against
static char g_error[512];
extern "C" void psxhip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

typedef long long ll;

static void answer(const char* kind, int rc, bool early = false, int value = 0) {
    if (rc) printf("%s : %d | %s\n", kind, rc, g_error);
    else if (early) printf("%s : 0 | early %d\n", kind, value);
    else printf("%s : 0 | device\n", kind);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "r");
    FILE* blob = fopen(argv[2], "wb");
    if (!in || !blob) return 2;
    size_t blob_at = 0;
    printf("const %d %d %lld %d %d\n", kAfeHeaderBytes, PSXHIP_AFE_TILE, (ll)kLaunchMaxIn, kFilterSize, kMaxPhases);
    char kind[32];
    int k;
    while (fscanf(in, "%31s %d", kind, &k) == 2) {
        if (k < 0 || k > 100000) return 3;
        std::vector<ll> a((size_t)k);
        for (ll& v : a)
            if (fscanf(in, "%lld", &v) != 1) return 3;
        g_error[0] = 0;
        const std::string name = kind;
        if (name == "design" && k == 4) {               // src_rate, dst_rate, coef given, cap (-1: room for the table): P, T and where the table went
            int P = -1, T = -1;
            std::vector<int16_t> coef(1024 * 600);
            const int rc = psxhip_resampler_design((int)a[0], (int)a[1], &P, &T, a[2] ? coef.data() : nullptr, a[3] < 0 ? (int)coef.size() : (int)a[3]);
            if (rc < 0) {
                answer(kind, rc);
                continue;
            }
            const size_t n = a[2] && a[3] < 0 ? (size_t)P * T * 2 : 0;
            fwrite(coef.data(), 1, n, blob);
            printf("%s : 0 | %d %d %d %zu %zu\n", kind, rc, P, T, blob_at, n);
            blob_at += n;
        } else if (name == "count" && k == 5) {         // src_rate, dst_rate, consumed, n_in, flush
            printf("%s : 0 | %lld\n", kind, (ll)psxhip_resampler_output_count((int)a[0], (int)a[1], a[2], a[3], (int)a[4]));
        } else if (name == "create" && k >= 6) {        // src_format, src_channels, src_rate, dst_channels, dst_rate, mix given, then the matrix
            std::vector<int16_t> mix(a.begin() + 6, a.end());
            mix.push_back(0);
            ResamplerPlan p;
            const int rc = resampler_create_plan((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], a[5] ? mix.data() : nullptr, &p);
            if (rc) {
                answer(kind, rc);
                continue;
            }
            printf("%s : 0 | device |", kind);
            for (int c = 0; c < 8; c++)
                for (int s = 0; s < 8; s++) printf(" %d", p.mix[c][s]);
            printf("\n");
        } else if (name == "shape" && k == 5) {         // src_rate, dst_rate, dst_channels, LDS bytes per CU, CUs
            Design d;
            if (!design_params((int)a[0], (int)a[1], &d)) return 4;
            ResamplerShape s;
            const int rc = resampler_shape(d, (int)a[2], (size_t)a[3], (int)a[4], &s);
            if (rc) answer(kind, rc);
            else printf("%s : 0 | %d %d %zu %d | %d %d %d %d %d %d\n", kind, s.span, s.coef_lds, s.lds_bytes, s.grid_max, d.L, d.M, d.P, d.T, d.H, (int)d.bypass);
        } else if ((name == "convdev" || name == "convhost") && k == 9) {
            // handle (S16P, 2 -> 2 channels, 48000 -> 37800), flushed, consumed, src given, the source pointer that is NULL (-1: none), n_in, dst given,
            // dst_cap, flush: the call's outputs behind "device"
            ResamplerPlan p;
            if (resampler_create_plan(PSXHIP_PCM_S16P, 2, 48000, 2, 37800, nullptr, &p)) return 4;
            const void* src[8] = {};
            for (int i = 0; i < 8; i++) src[i] = i == a[4] ? nullptr : (const void*)0x100000;
            int64_t count;
            bool go;
            const int rc = resampler_convert_check(name == "convhost", a[0] ? &p : nullptr, a[1] != 0, a[2], a[3] ? src : nullptr, a[5], a[6] != 0, a[7], (int)a[8], &count, &go);
            if (rc || !go) answer(kind, rc, true, 0);
            else printf("%s : 0 | device %lld\n", kind, (ll)count);
        } else if (name == "cut" && k == 6) {           // src_rate, dst_rate, consumed, n_in, flush, grid_max: outputs_of and avail(consumed), then every launch
            Design d;
            if (!design_params((int)a[0], (int)a[1], &d)) return 4;
            printf("%s : 0 | %lld %lld", kind, (ll)outputs_of(d, a[2], a[3], (int)a[4]), (ll)avail(d, a[2]));
            int64_t consumed = a[2], done = 0;
            do {
                const ResamplerLaunch l = resampler_launch(d, consumed, a[3] - done, (int)a[4], (int)a[5]);
                printf(" | %lld %d %lld %d %lld %lld %d", (ll)l.n, (int)l.flush, (ll)l.i0, l.r0, (ll)l.n_out, (ll)l.work, l.grid);
                consumed += l.n;
                done += l.n;
            } while (done < a[3]);
            printf("\n");
        } else {
            fprintf(stderr, "unknown call %s with %d numbers\n", kind, k);
            return 3;
        }
    }
    fclose(blob);
    return 0;
}
