// picture_plan_check.cpp -- runs a table of calls through psxavenc_amd/csrc/picture_plan.cpp and prints what the plans derive, for
// tests/test_picture_plan_cpu.py (restatements, tests/golden/picture_plan_parent.json) and tests/test_gpu_front_end_plan_seams.py.
// Built from picture_plan.cpp and this file alone, with a host compiler: every case is arithmetic, so a call may name made-up
// addresses without anything being read through them.
//
//   picture_plan_check <calls> <blob>
// calls: one call a line, "<kind> <k> <k numbers>".  A kind named after an entry point takes the entry point's arguments in its own
//        order (pointers as addresses; device, stream and handle pointers left out unless said) and calls the plan functions in the
//        order the entry point calls them.  An environment switch comes as its number, -1 for "not set".
// blob:  the scaler's bank tables are appended here as raw bytes (per bank: left int32, coef int16, digits uint32)
// out:   a line of constants, then per call "<kind> : <rc> | <error text>" for a refusal, "<kind> : 0 | device" where the entry point
//        goes on to the device, "<kind> : 0 | early <v>" where it returns v before that, "<kind> : 0 | <numbers>" otherwise.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../psxavenc_amd/csrc/picture_plan.h"

// the error sink: the one symbol the plan module links against
static char g_error[512];
extern "C" void psxhip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

typedef long long ll;
typedef uintptr_t up;

static void answer(const char* kind, int rc, bool early = false, int value = 0) {
    if (rc) printf("%s : %d | %s\n", kind, rc, g_error);
    else if (early) printf("%s : 0 | early %d\n", kind, value);
    else printf("%s : 0 | device\n", kind);
}

// an environment switch as the launch file would read it
static const char* env_text(ll v, char (&buf)[32]) {
    if (v < 0) return nullptr;
    snprintf(buf, sizeof buf, "%lld", v);
    return buf;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "r");
    FILE* blob = fopen(argv[2], "wb");
    if (!in || !blob) return 2;
    size_t blob_at = 0;
    printf("const %d %d %d %d", kScalerPlanePad, kScalerLdsSlack, kScalerTileRowBytes, kScalerLaunchFrames);
    for (const auto& s : kScalerShapes) printf(" %d %d", s[0], s[1]);
    printf("\n");
    char kind[32];
    int k;
    while (fscanf(in, "%31s %d", kind, &k) == 2) {
        if (k < 0 || k > 100000) return 3;
        std::vector<ll> a((size_t)k);
        for (ll& v : a)
            if (fscanf(in, "%lld", &v) != 1) return 3;
        g_error[0] = 0;
        const std::string name = kind;
        char buf[32];
        if (name == "screate" && k == 6) {              // src_format, src_width, src_height, src_full_range, dst_width, dst_height
            answer(kind, scaler_geometry_check((int)a[0], (int)a[1], (int)a[2], (int)a[4], (int)a[5]));
        } else if (name == "tile" && k == 9) {          // ..., the device's LDS bytes per CU and CU count, PSXHIP_SCALER_TILE
            const bool yuv = a[0] == PSXHIP_PIX_YUV420P;
            HostBank h[4];
            int rc = scaler_geometry_check((int)a[0], (int)a[1], (int)a[2], (int)a[4], (int)a[5]);
            if (!rc) rc = scaler_design_banks((int)a[0], (int)a[1], (int)a[2], (int)a[4], (int)a[5], h);
            psxhip_scaler_job_t j;
            memset(&j, 0, sizeof j);
            size_t lds = 0;
            if (!rc) rc = scaler_choose_tile(h, yuv, (int)a[4], (int)a[5], (size_t)a[6], env_text(a[8], buf), &j, &lds);
            if (rc) {
                answer(kind, rc);
                continue;
            }
            printf("%s : 0 | %d %d %d %d %d %d %d %d %zu |", kind, j.TW, j.TH, j.reg_rows, j.reg_cols, j.creg_rows, j.creg_cols, j.tiles_x, j.tiles_y, lds);
            const ScalerLds s = scaler_job_lds(j, yuv);
            printf(" %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d |", s.plane_bytes, s.cplane_bytes, s.ring_l, s.ring_c, s.v_words, s.p0, s.p1, s.p2, s.tmp_l,
                   s.tmp_c, s.g_lh, s.g_ch, s.l_lh, s.l_ch, s.v_tab, s.t_rows, s.total);
            const psxhip_scaler_bank_t* banks[4] = {&j.lh, &j.lv, &j.ch, &j.cv};
            for (int i = 0; i < 4; i++) {
                const size_t nl = h[i].left.size() * 4, nc = h[i].coef.size() * 2, nd = h[i].digits.size() * 4;
                fwrite(h[i].left.data(), 1, nl, blob);
                fwrite(h[i].coef.data(), 1, nc, blob);
                fwrite(h[i].digits.data(), 1, nd, blob);
                printf(" %d %d %zu %zu %zu %zu", banks[i]->taps, banks[i]->taps4, blob_at, nl, nc, nd);
                blob_at += nl + nc + nd;
            }
            printf("\n");
        } else if (name == "vsegs" && k == 5) {         // CUs, tiles_x, tiles_y, n_frames, PSXHIP_SCALER_VSEGS: vsegs, then every launch's frames
            printf("%s : 0 | %d |", kind, scaler_vsegs((int)a[0], (int)a[1], (int)a[2], (int)a[3], env_text(a[4], buf)));
            for (int f0 = 0; f0 < (int)a[3]; f0 += kScalerLaunchFrames) printf(" %d", scaler_launch_frames((int)a[3], f0));
            printf("\n");
        } else if ((name == "sconvdev" || name == "sconvhost") && k == 9) {
            // handle, src, dst, n_frames, src_stride, frame_stride; and of the handle: src_bytes, dst_width, dst_height
            bool go;
            const bool dev = name == "sconvdev";
            const int rc = scaler_convert_check(dev ? "psxhip_scaler_convert_device" : "psxhip_scaler_convert_host", a[0] != 0, (up)a[1], (up)a[2], (int)a[3], dev,
                                                (size_t)a[4], (size_t)a[5], (size_t)a[6], (int)a[7], (int)a[8], &go);
            answer(kind, rc, !rc && !go, 0);
        } else if (name == "icreate" && k >= 10) {
            // handle pointer given, src_format, width, height, planes given, n_planes, matrix, full_range, out_format, options, then (offset, pitch)
            // per plane given.  The entry point ends here: it needs no device
            if (!a[0]) {
                answer(kind, picture_bad("psxhip_ingest_create", "NULL argument"));
                continue;
            }
            const ll* b = a.data() + 1;
            const size_t given = (size_t)(k - 10) / 2;
            std::vector<psxhip_ingest_plane_t> planes(given + 1);
            for (size_t p = 0; p < given; p++) { planes[p].offset = (size_t)b[9 + 2 * p]; planes[p].pitch = (size_t)b[10 + 2 * p]; }
            IngestPlan plan;
            const int rc = ingest_create_plan((int)b[0], (int)b[1], (int)b[2], b[3] ? planes.data() : nullptr, (int)b[4], (int)b[5], (int)b[6], (int)b[7], (uint32_t)b[8], &plan);
            if (rc) answer(kind, rc);
            else
                printf("%s : 0 | %zu %zu %d %d %d %d %d %d %d\n", kind, plan.src_bytes, plan.out_bytes, plan.d.cy, plan.d.rv, plan.d.gu, plan.d.gv, plan.d.bu, plan.d.yoff,
                       plan.d.coff);
        } else if ((name == "iconvdev" || name == "iconvhost") && k == 11) {
            // the handle's source: src_format, width, height, out_format (one tight plane set, BT.601 full range; src_format < 0: no handle);
            // then src, src_stride, n_src, index, n_out, dst, out_stride
            const bool dev = name == "iconvdev";
            IngestPlan plan;
            bool have = a[0] >= 0;
            if (have) {
                IngestDesc d = {};
                d.f = ingest_format((int)a[0]);
                d.w = (int)a[1]; d.h = (int)a[2];
                psxhip_ingest_plane_t planes[3];
                size_t at = 0;
                for (int p = 0; p < d.f.planes; p++) {
                    planes[p].offset = at; planes[p].pitch = (size_t)ing_row_bytes(d, p);
                    at += planes[p].pitch * (size_t)ing_plane_rows(d, p);
                }
                if (ingest_create_plan((int)a[0], (int)a[1], (int)a[2], planes, d.f.planes, PSXHIP_MATRIX_BT601, 1, (int)a[3], 0, &plan)) return 4;
            }
            bool go;
            const int rc = ingest_check(dev ? "psxhip_ingest_convert_device" : "psxhip_ingest_convert_host", have ? &plan : nullptr, (up)a[4], (size_t)a[5], (int)a[6],
                                        (int)a[8], (up)a[9], (size_t)a[10], dev, &go);
            answer(kind, rc, !rc && !go, 0);
        } else if ((name == "dconvdev" && k == 11) || (name == "dconvhost" && k == 7)) {
            psxhip_display_job_t j;
            memset(&j, 0, sizeof j);
            if (name == "dconvdev") {       // d_frames, frame_stride, width, height, n_frames, d_decoded, out_format, options, d_dst, dst_pitch, dst_stride
                j.d_frames = (const uint8_t*)(up)a[0]; j.frame_stride = (size_t)a[1]; j.width = (int)a[2]; j.height = (int)a[3]; j.n_frames = (int)a[4];
                j.out_format = (int)a[6]; j.options = (uint32_t)a[7]; j.d_dst = (uint8_t*)(up)a[8]; j.dst_pitch = (size_t)a[9]; j.dst_stride = (size_t)a[10];
                answer(kind, psxhip_display_check("psxhip_display_convert_device", &j, true));
            } else {                        // frames, width, height, n_frames, out_format, options, dst: the job as the entry point fills it
                const int width = (int)a[1], height = (int)a[2];
                const size_t row = psxhip_display_row_bytes((int)a[4], width), rows = height > 0 ? (size_t)height : 0;
                j.d_frames = (const uint8_t*)(up)a[0]; j.frame_stride = (width > 0 ? (size_t)width : 0) * rows * 3 / 2;
                j.d_dst = (uint8_t*)(up)a[6]; j.dst_pitch = row; j.dst_stride = row * rows;
                j.width = width; j.height = height; j.n_frames = (int)a[3]; j.out_format = (int)a[4]; j.options = (uint32_t)a[5];
                answer(kind, psxhip_display_check("psxhip_display_convert_host", &j, false));
            }
        } else if (name == "fit" && k == 6) {           // ..., dst pointers given: the return code, then w and h
            int w = -1, h = -1;
            const int rc = psxhip_ingest_fit((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], a[5] ? &w : nullptr, a[5] ? &h : nullptr);
            if (rc) answer(kind, rc);
            else printf("%s : 0 | %d %d\n", kind, w, h);
        } else if (name == "recommend" && k == 4) {
            const int rc = psxhip_ingest_recommend((int)a[0], (int)a[1], (int)a[2], (int)a[3]);
            if (rc < 0) answer(kind, rc);
            else printf("%s : 0 | %d\n", kind, rc);
        } else if (name == "pace" && k >= 7) {          // pts given, tb_num, tb_den, fps_num, fps_den, out given, cap, then the pts: the count, then the indices
            std::vector<int64_t> pts(a.begin() + 7, a.end());
            pts.push_back(0);
            std::vector<int32_t> out((size_t)(a[6] > 0 ? a[6] : 0) + 1, -7);
            const int rc = psxhip_ingest_pace(a[0] ? pts.data() : nullptr, k - 7, (int)a[1], (int)a[2], (int)a[3], (int)a[4], a[5] ? out.data() : nullptr, (int)a[6]);
            if (rc < 0) {
                answer(kind, rc);
                continue;
            }
            printf("%s : 0 | %d |", kind, rc);
            for (int i = 0; i < rc && i < (int)a[6]; i++) printf(" %d", out[(size_t)i]);
            printf("\n");
        } else {
            fprintf(stderr, "unknown call %s with %d numbers\n", kind, k);
            return 3;
        }
    }
    fclose(blob);
    return 0;
}
