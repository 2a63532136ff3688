// mdec_plan_check.cpp -- prints what psxavenc_amd/csrc/mdec_plan.cpp derives, one line per case with the case's own parameters in
// front, for tests/test_mdec_plan_cpu.py to compare with its restatements.  Built from mdec_plan.cpp and this file alone, with a host
// compiler and the host sanitizers: the geometry, the pass order, the split geometry, the launch policy, the host call's checks and
// the test switch's parser run without a device, and every buffer is exactly as long as the callee is told.
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <vector>

#include "../../psxavenc_amd/csrc/mdec_layout.h"
#include "../../psxavenc_amd/csrc/mdec_plan.h"

// the error sink: the one symbol mdec_plan.cpp links against
static char g_error[512];
extern "C" void psxhip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

static const int kSizes[6] = {16, 48, 160, 320, 640, 1024};
static const int kOrderSizes[4][2] = {{16, 16}, {48, 32}, {320, 240}, {640, 480}};

static void print_words(const std::vector<uint32_t>& v) {
    for (uint32_t x : v) printf(" %x", x);
    printf("\n");
}

static void print_split(int codec, int w, int h, int budget, int n_frames, int n_cu) {
    psxhip_mdec_split_geo_t g;
    const int ok = psxhip_mdec_split_geometry(codec, w, h, budget, n_frames, n_cu, &g);
    printf("split %d %d %d %d %d %d : %d %d %d %d %zu %zu %zu %zu %zu %zu\n", codec, w, h, budget, n_frames, n_cu, ok, g.seg_mbs, g.segs, g.img_words,
           g.ws_stride, g.ws_slots, g.ws_dcq, g.ws_img, g.ws_done, g.lds_bytes);
}

static void print_policy(const MdecLaunchConsts& k, int nb, int n_frames, int stats, int no_split) {
    const MdecLaunchPlan p = mdec_launch_policy(k, nb, n_frames, stats != 0, no_split != 0);
    printf("policy %d %d %d %d %d %d %d %d %d %d | %d %d %d %d : %d %d %d %d %d %d %d %d %d\n", k.codec, k.width, k.height, k.max_frame_size, k.n_cu, k.groups_max,
           k.large, k.split_max, k.retry_cap, (int)k.order_large, nb, n_frames, stats, no_split, (int)p.split, p.geo.seg_mbs, p.geo.segs, (int)p.small_batch, p.large,
           p.trips, p.it_step, p.grid, (int)p.queue);
}

static void print_check(int max_frame_size, std::vector<int32_t> sizes, int n_frames, int uniform, size_t out_stride, int row_bytes) {
    MdecHostCall hc = {-1, 0};
    g_error[0] = 0;
    const int rc = mdec_host_call_check(max_frame_size, n_frames, sizes.empty() ? nullptr : sizes.data(), uniform, out_stride, row_bytes, &hc);
    printf("check %d %d %d %zu %d", max_frame_size, n_frames, uniform, out_stride, row_bytes);
    for (int32_t s : sizes) printf(" %d", s);
    printf(" : %d | %d %zu | %s\n", rc, hc.max_size, hc.dstride, g_error);
}

int main() {
    printf("const %d %d %d %d %d %d %u %d %d %d %d %d %d %d\n", kWavesSmall, kWavesLarge, kTileStride, kZStride, kPilotMax, kMaxTiles, kNoMb, (int)S_COUNT,
           kWaveTileBytes, BS_LUT_SIZE, kSplitWaves, kSplitRound, kSplitRounds, kSplitWbufWords);
    printf("threads %d %d\n", psxhip_mdec_threads_per_group(0), psxhip_mdec_threads_per_group(1));

    // ---- geometry, and the largest budget of every size
    for (size_t lds_cu : {(size_t)65536, (size_t)163840})
        for (int w : kSizes)
            for (int h : kSizes) {
                for (int budget : {8, 512, 8192, 20000, 80000, 131072, 262140}) {
                    int large = -1, ow = -1, sw = -1;
                    size_t need = 0;
                    const int fits = mdec_geometry(w, h, budget, lds_cu, &large, &ow, &sw, &need);
                    printf("geo %d %d %d %zu : %d %d %d %d %zu\n", w, h, budget, lds_cu, fits, large, ow, sw, need);
                }
                const int limit = mdec_max_budget(w, h, lds_cu);
                printf("maxb %d %d %zu : %d %d", w, h, lds_cu, limit, limit ? mdec_geometry(w, h, limit, lds_cu, nullptr, nullptr, nullptr, nullptr) : 0);
                for (int d = 1; d <= 8; d++) printf(" %d", mdec_geometry(w, h, limit + d, lds_cu, nullptr, nullptr, nullptr, nullptr));
                printf("\n");
            }
    printf("args %d %d %d %d %d %d %d %d %d\n", (int)mdec_args_ok(0, 16, 16, 8), (int)mdec_args_ok(2, 1024, 1024, 8), (int)mdec_args_ok(3, 16, 16, 8),
           (int)mdec_args_ok(-1, 16, 16, 8), (int)mdec_args_ok(0, 24, 16, 8), (int)mdec_args_ok(0, 16, 1040, 8), (int)mdec_args_ok(0, 0, 16, 8),
           (int)mdec_args_ok(0, 16, 16, 7), (int)mdec_args_ok(1, 320, 240, 8192));

    // ---- pass order and table: whole, and with a cap short of the end (the buffers are exactly cap entries long)
    for (const auto& sz : kOrderSizes)
        for (int large = 0; large < 2; large++) {
            const int w = sz[0], h = sz[1];
            const int n = psxhip_mdec_pass_order(w, h, large, nullptr, 0);
            for (int cap : {n, n > 7 ? 7 : n - 1}) {
                std::vector<uint32_t> o((size_t)cap, 0xDEADBEEFu);
                printf("order %d %d %d %d : %d |", w, h, large, cap, psxhip_mdec_pass_order(w, h, large, o.data(), cap));
                print_words(o);
            }
            for (int cap : {n + 1, n, n > 7 ? 7 : n - 1}) {
                std::vector<uint32_t> t((size_t)cap * 2, 0xDEADBEEFu);
                printf("table %d %d %d %d : %d %d |", w, h, large, cap, psxhip_mdec_pass_table(w, h, large, nullptr, 0), psxhip_mdec_pass_table(w, h, large, t.data(), cap));
                print_words(t);
            }
            printf("trips %d %d %d : %d %d\n", w, h, large, mdec_trips(w, h, large), mdec_pick_it_step(mdec_trips(w, h, large)));
        }

    // ---- split geometry
    for (int n_cu : {256, 8, 1})
        for (int w : kSizes)
            for (int h : kSizes)
                for (int n_frames : {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 64}) print_split(w == 16 ? 0 : 1, w, h, 8192, n_frames, n_cu);
    for (int budget : {8, 4096, 262140})
        for (int codec = 0; codec < 3; codec++) print_split(codec, 320, 240, budget, 1, 256);
    print_split(0, 320, 240, 8192, 0, 256);
    print_split(0, 320, 240, 8192, 1, 0);

    // ---- the cases of tests/golden/mdec_plan_parent.json (recorded from the library before the plan module existed)
    for (const auto& sz : {std::initializer_list<int>{16, 16}, {48, 32}, {160, 112}, {320, 240}, {336, 240}, {640, 480}, {1024, 1024}})
        for (int large = 0; large < 2; large++) {
            const int w = sz.begin()[0], h = sz.begin()[1], n = psxhip_mdec_pass_table(w, h, large, nullptr, 0);
            std::vector<uint32_t> t(((size_t)n + 1) * 2, 0xDEADBEEFu);
            printf("gtable %d %d %d : %d |", w, h, large, psxhip_mdec_pass_table(w, h, large, t.data(), n + 1));
            print_words(t);
        }
    print_split(0, 320, 240, 8192, 1, 256);
    print_split(1, 320, 240, 8192, 12, 256);
    print_split(2, 640, 480, 20000, 1, 256);
    print_split(1, 640, 480, 20000, 5, 256);
    print_split(0, 48, 32, 4096, 2, 256);
    print_split(1, 1024, 1024, 80000, 1, 256);
    print_split(1, 1024, 1024, 80000, 3, 8);
    print_split(0, 16, 16, 8, 64, 1);
    print_split(2, 160, 112, 262140, 7, 64);

    // ---- launch policy: n_frames at and either side of every threshold
    for (int variant = 0; variant < 5; variant++) {
        MdecLaunchConsts k;
        k.codec = 1; k.width = 320; k.height = 240; k.max_frame_size = 8192;
        k.n_cu = 256; k.groups_max = 512; k.large = 0; k.split_max = 12; k.retry_cap = 1 << 16;
        if (variant == 1) k.retry_cap = 1000;                           // (between grid and 8 x grid: the queue's own size binds)
        if (variant == 2) k.retry_cap = 0;
        if (variant == 3) { k.large = 1; k.groups_max = 256; }
        if (variant == 4) k.split_max = 0;
        for (int order_large = 0; order_large < 2; order_large++) {
            k.order_large = order_large && !k.large;
            for (int t : {k.split_max, k.n_cu, k.groups_max, 8 * k.groups_max, k.retry_cap, 1})
                for (int n_frames = t - 1; n_frames <= t + 1; n_frames++)
                    for (int nb = 1; nb <= 2; nb++)
                        for (int stats = 0; stats < 2; stats++)
                            for (int no_split = 0; no_split < 2; no_split++)
                                if (n_frames >= nb) print_policy(k, nb, n_frames, stats, no_split);
        }
    }

    // ---- the host call's checks: every refusal, and the accepted edges
    print_check(4096, {}, 3, 8, 8, 0);
    print_check(4096, {}, 3, 4096, 4096, 0);
    print_check(4096, {}, 3, 7, 4096, 0);
    print_check(4096, {}, 3, 4097, 8192, 0);
    print_check(4096, {}, 3, 1001, 1000, 0);
    print_check(4096, {}, 3, 1001, 1001, 0);
    print_check(4096, {8, 4096, 777}, 3, 0, 4096, 0);
    print_check(4096, {8, 7, 777}, 3, 0, 4096, 0);
    print_check(4096, {8, 512, 4097}, 3, 0, 8192, 0);
    print_check(4096, {8, 512, 777}, 3, 0, 776, 0);
    print_check(4096, {8, 512, 777}, 3, 0, 777, 0);
    print_check(4096, {8, 512, 777}, 3, 0, 4096, 777);
    print_check(4096, {8, 512, 777}, 3, 0, 4096, 776);
    print_check(4096, {8, 512, 777}, 3, 0, 4096, 4096);
    print_check(4096, {8, 512, 777}, 3, 0, 8192, 4097);
    print_check(4096, {8, 512, 777}, 3, 0, 2047, 2048);
    print_check(4096, {}, 1, 512, 4096, 2048);
    print_check(4096, {}, 1, 512, 4096, 511);

    // ---- PSXHIP_MDEC_SPLIT_WITHHOLD, and what a segment's name means in a launch
    for (const char* spec : {"0:mid", "1:-1:2:1", "2:1000", "3:4:5", "0:0:1:7", "", "mid", "0", "x:1", "-1:0", "0:1:0", "0:1:-2", "0::1", "4:mid:3:0"}) {
        const MdecWithhold w = mdec_parse_withhold(spec);
        printf("withhold [%s] : %d %d %d %d\n", spec, w.frame, w.seg == INT_MIN ? -999999 : w.seg, w.launches, w.residue);
    }
    for (int segs : {1, 2, 7, 150})
        for (int seg : {INT_MIN, -1000, -2, -1, 0, 1, 6, 7, 149, 150, 1000}) printf("whseg %d %d : %d\n", seg == INT_MIN ? -999999 : seg, segs, mdec_withhold_segment(seg, segs));

    // ---- chunk size at its three bounds
    for (int groups_max : {512, 256, 1040, 1})
        for (size_t frame_bytes : {(size_t)2304, (size_t)115200, (size_t)460800, (size_t)1572864, (size_t)200 << 20})
            for (int n_frames : {1, 2, 63, 64, 65, 191, 192, 193, 383, 384, 385, 779, 780, 781, 100000})
                printf("chunk %d %zu %d : %d\n", groups_max, frame_bytes, n_frames, mdec_chunk_frames(groups_max, frame_bytes, n_frames));
    return 0;
}
