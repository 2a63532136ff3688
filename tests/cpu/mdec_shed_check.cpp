// mdec_shed_check.cpp -- the refinement's plain-C++ core (psxavenc_amd/csrc/mdec_shed_core.h) and its plan (mdec_plan.cpp) as a stand-alone
// program: tests/test_mdec_shed_core_cpu.py builds it with g++ -fsanitize=address,undefined and holds what it prints to the numpy
// statement (tests/mdec_shed_ref.py).
//
//   mdec_shed_check frames IN    IN: int32 count, then per frame int32 codec, blocks, budget, N, K and blocks x 64 int16 coefficients
//                                (raster order, blocks in the encoder's order).  Prints per frame
//                                "frame step count d_plain d_shed refined scale bytes blocks hwords bits rowhash" (hash: FNV-1a 64 of the
//                                budget's bytes of a refined row, else 0)
//   mdec_shed_check fdct IN OUT  IN: int32 count, then count x 64 int16 samples; OUT: count x 64 int16 coefficients
//   mdec_shed_check plan         every refusal of mdec_refine_call_check, and workspace layouts: "refuse name rc text", "ws ..."
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../psxavenc_amd/csrc/mdec_plan.h"
#include "../../psxavenc_amd/csrc/mdec_shed_core.h"

static char g_err[512];
extern "C" void psxhip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

static bool read_exact(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

static int run_frames(const char* path) {
    FILE* f = fopen(path, "rb");
    int32_t count = 0;
    if (!f || !read_exact(f, &count, 4)) return 2;
    for (int i = 0; i < count; i++) {
        int32_t h[5];
        if (!read_exact(f, h, sizeof h)) return 2;
        const int codec = h[0], nblk = h[1], b = h[2], N = h[3], K = h[4];
        std::vector<int16_t> raster((size_t)nblk * 64), fz((size_t)nblk * 64);
        if (!read_exact(f, raster.data(), raster.size() * 2)) return 2;
        for (int blk = 0; blk < nblk; blk++)
            for (int z = 0; z < 64; z++) fz[(size_t)blk * 64 + z] = raster[(size_t)blk * 64 + bs_zagzig[z]];
        ShedDecision d = {0, 0, 0, 0, 0, 0, 0};
        int32_t res[4] = {0, 0, 0, 0};
        uint64_t hash = 0;
        if (shed_frame_eligible(N)) {
            std::vector<int64_t> acc((size_t)kShedRows * 64, 0);
            int last[3] = {0, 0, 0};
            int64_t dc_bits = 0;
            for (int blk = 0; blk < nblk; blk++) {
                shed_analyse_block_host(&fz[(size_t)blk * 64], N - 1, N, acc.data());
                const int comp = blk % 6 < 2 ? blk % 6 : 2;
                dc_bits += shed_dc_code(codec, comp, shed_dc_level(fz[(size_t)blk * 64]), &last[comp]) >> 24;
            }
            d = shed_decide(acc.data(), dc_bits, nblk, b, K);
            if (d.refined) {
                shed_result(d, nblk, N - 1, res);
                std::vector<uint8_t> row((size_t)b);
                shed_emit_row_host(codec, fz.data(), nblk, N - 1, d, b, row.data());
                hash = 1469598103934665603ull;
                for (uint8_t v : row) hash = (hash ^ v) * 1099511628211ull;
            }
        }
        printf("frame %d %d %" PRId64 " %" PRId64 " %d %d %d %d %d %" PRId64 " %" PRIu64 "\n", d.step, d.count, d.d_plain, d.d_shed, d.refined,
               res[0], res[1], res[2], res[3], d.bits, hash);
    }
    fclose(f);
    return 0;
}

static int run_fdct(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    int32_t count = 0;
    if (!f || !read_exact(f, &count, 4)) return 2;
    std::vector<int16_t> blk((size_t)count * 64);
    if (!read_exact(f, blk.data(), blk.size() * 2)) return 2;
    fclose(f);
    for (int i = 0; i < count; i++) shed_fdct8x8(&blk[(size_t)i * 64]);
    FILE* o = fopen(out, "wb");
    if (!o || fwrite(blk.data(), 2, blk.size(), o) != blk.size()) return 2;
    fclose(o);
    return 0;
}

static void refuse(const char* name, int max_frame_size, size_t frame_bytes, const MdecRefineCall& a) {
    g_err[0] = 0;
    const int rc = mdec_refine_call_check(max_frame_size, frame_bytes, a);
    printf("refuse %s %d %s\n", name, rc, g_err);
}

static int run_plan() {
    alignas(16) static uint8_t mem[64];
    const MdecRefineCall ok = {mem, mem + 16, mem + 32, 384, 512, 4, false, 500, 1};
    refuse("sound", 512, 384, ok);
    MdecRefineCall a = ok;
    a.per_frame_budgets = true, a.uniform_max_size = 0;
    refuse("sound_per_frame", 512, 384, a);
    a = ok, a.n_frames = 0;
    refuse("sound_no_frames", 512, 384, a);
    a = ok, a.d_frames = nullptr;
    refuse("null_frames", 512, 384, a);
    a = ok, a.d_out = nullptr;
    refuse("null_out", 512, 384, a);
    a = ok, a.d_results = nullptr;
    refuse("null_results", 512, 384, a);
    a = ok, a.n_frames = -1;
    refuse("negative_frames", 512, 384, a);
    a = ok, a.max_magnitude = 0;
    refuse("magnitude_0", 512, 384, a);
    a = ok, a.max_magnitude = 4;
    refuse("magnitude_4", 512, 384, a);
    a = ok, a.frame_stride = 380;
    refuse("frame_stride_small", 512, 384, a);
    a = ok, a.frame_stride = 386;
    refuse("frame_stride_misaligned", 512, 384, a);
    a = ok, a.out_stride = 514;
    refuse("out_stride_misaligned", 512, 384, a);
    a = ok, a.d_frames = mem + 2;
    refuse("frames_misaligned", 512, 384, a);
    a = ok, a.d_out = mem + 18;
    refuse("out_misaligned", 512, 384, a);
    a = ok, a.uniform_max_size = 7;
    refuse("budget_small", 512, 384, a);
    a = ok, a.uniform_max_size = 513, a.out_stride = 1024;
    refuse("budget_above_context", 512, 384, a);
    a = ok, a.out_stride = 496;
    refuse("budget_above_stride", 512, 384, a);
    a = ok, a.n_frames = 0x1000000;
    refuse("too_many_frames", 512, 384, a);
    for (int nblk : {6, 12, 36, 1800, 24576}) {
        const MdecShedWs w = mdec_shed_workspace(nblk);
        printf("ws %d %zu %zu %zu %zu %zu %zu %zu\n", nblk, w.acc, w.decision, w.zeroed, w.dc_level, w.dc_code, w.block_off, w.stride);
    }
    for (int nmb : {1, 16, 17, 300, 4096}) printf("groups %d %d\n", nmb, mdec_shed_analyse_groups(nmb));
    printf("rows %d\n", (int)kShedRows);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "frames")) return run_frames(argv[2]);
    if (argc == 4 && !strcmp(argv[1], "fdct")) return run_fdct(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "plan")) return run_plan();
    fprintf(stderr, "usage: mdec_shed_check frames IN | fdct IN OUT | plan\n");
    return 2;
}
