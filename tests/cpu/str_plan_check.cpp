// str_plan_check.cpp -- prints what psxavenc_amd/csrc/str_plan.cpp derives, one line per case with the case's own parameters in
// front, for tests/test_str_plan_cpu.py to compare with the restatements (tests/strspu_ref.py, tests/str_reference_loop.py).  Built
// from str_plan.cpp and this file alone, with a host compiler and the host sanitizers: the sector loop, its 64-bit budget arithmetic
// and the block placement run without a device, and the buffers are exactly as long as the callees are told.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <vector>

#include "../../psxavenc_amd/csrc/str_plan.h"

// the error sink: the one symbol str_plan.cpp links against
static char g_error[512];
extern "C" void psxhip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

static psxhip_str_settings_t settings(int format, int fnum, int fden, int speed, int trailing, int ch, int freq, int bits, int tail, uint32_t options = 0x0001,
                                      int video_id = 0x8001) {
    psxhip_str_settings_t s;
    memset(&s, 0, sizeof s);
    s.format = format;
    s.video_codec = 0;
    s.video_width = 48;
    s.video_height = 32;
    s.str_fps_num = fnum;
    s.str_fps_den = fden;
    s.str_cd_speed = speed;
    s.str_video_id = video_id;
    s.trailing_audio = trailing;
    s.audio_channels = ch;
    s.audio_frequency = freq;
    s.audio_bit_depth = bits;
    s.audio_xa_file = 1;
    s.audio_xa_channel = 0;
    s.tail_mode = tail;
    s.strspu_options = (int32_t)options;
    return s;
}

// ": rc | the public plan, n_audio, audio_samples, base, den | budgets | rows" -- or ": rc | the error text"
static void print_plan(const psxhip_str_settings_t& s, int n_frames, long long pcm) {
    Plan pl;
    g_error[0] = 0;
    const int rc = make_plan(&s, n_frames, pcm, &pl);
    printf(" : %d |", rc);
    if (rc) {
        printf(" %s\n", g_error);
        return;
    }
    const psxhip_str_plan_t& p = pl.pub;
    printf(" %d %d %d %d %d %d %d %d %d %lld %lld %lld |", p.n_sectors, p.n_video_sectors, p.n_audio_sectors, p.sector_size, p.interleave,
           p.audio_samples_per_sector, p.max_frame_size, p.n_frames_encoded, pl.n_audio, (long long)pl.audio_samples, (long long)pl.rates.base,
           (long long)pl.rates.den);
    for (int32_t b : pl.budgets) printf(" %d", b);
    printf(" |");
    for (const psxhip_str_sector_t& r : pl.sectors) printf(" %d %d %d %d", r.kind, r.frame, r.index, r.eof);
    printf("\n");
}

// the bytes the placement and the header cases read: x <- (1103515245 x + 12345) mod 2^31 from x = seed, byte i = bits 16-23 of the
// i-th x after the seed
static std::vector<uint8_t> recurrence(uint32_t seed, size_t n) {
    std::vector<uint8_t> out(n);
    uint32_t x = seed;
    for (size_t i = 0; i < n; i++) {
        x = (1103515245u * x + 12345u) & 0x7FFFFFFFu;
        out[i] = (uint8_t)(x >> 16);
    }
    return out;
}

static void print_hex(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
    printf("\n");
}

int main() {
    const int REFERENCE = PSXHIP_STR_TAIL_REFERENCE, COMPLETE = PSXHIP_STR_TAIL_COMPLETE;
    const int fps[][2] = {{15, 1}, {30, 1}, {30000, 1001}};
    // ---- format 8: every rate, frame rate and audio position of tests/test_strspu_plan.py, 0 .. 5 frames
    const int rates[][3] = {{44100, 2, 2}, {44100, 1, 2}, {44100, 2, 1}, {32000, 2, 2}, {48000, 2, 1}, {11025, 1, 2}};
    for (const auto& r : rates)
        for (const auto& f : fps)
            for (int trailing = 0; trailing < 2; trailing++)
                for (int n_frames = 0; n_frames < 6; n_frames++) {
                    printf("plan8 %d %d %d %d %d %d %d", r[0], r[1], r[2], f[0], f[1], trailing, n_frames);
                    print_plan(settings(FORMAT_STRSPU, f[0], f[1], r[2], trailing, r[1], r[0], 4, COMPLETE), n_frames, 0);
                }
    // ---- formats 6 / 7 / 9, the reference's tail: the cases of test_str_plan_follows_the_reference_sector_loop
    const int cases[][8] = {{7, 2, 4, 37800, 2, 15, 1, 0},         {7, 2, 4, 37800, 2, 15, 1, 1},  {6, 1, 4, 37800, 2, 15, 1, 0}, {6, 2, 8, 18900, 1, 10, 1, 0},
                            {9, 0, 4, 37800, 2, 15, 1, 0},         {7, 2, 4, 37800, 2, 30000, 1001, 0}, {6, 1, 8, 37800, 2, 25, 1, 1}};
    for (const auto& c : cases) {
        const psxhip_str_settings_t s = settings(c[0], c[5], c[6], c[4], c[7], c[1], c[3], c[2], REFERENCE);
        Plan probe;
        if (make_plan(&s, 4, 0, &probe)) return 2;
        const long long sps = probe.pub.audio_samples_per_sector;
        for (int n_frames : {1, 2, 3, 4, 7, 24})
            for (long long n_audio : {1000000ll, 0ll, 1ll, sps - 1, sps, sps + 1, 2 * sps, 3 * sps + 77, 7 * sps}) {
                if (!c[1] && n_audio) continue;                 // (no audio stream: one length)
                printf("planref %d %d %d %d %d %d %d %d %d %lld", c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], n_frames, n_audio);
                print_plan(s, n_frames, n_audio);
            }
    }
    // ---- no frame at all: both tails, with and without audio
    const int zero[][3] = {{9, 0, 0}, {7, 2, 0}, {7, 2, 1}, {7, 1, 1}};
    for (const auto& z : zero)
        for (int tail : {REFERENCE, COMPLETE})
            for (long long pcm : {0ll, 1000ll, 5000ll, 1ll << 40}) {
                printf("zero %d %d %d %d %lld", z[0], z[1], z[2], tail, pcm);
                print_plan(settings(z[0], 15, 1, 2, z[2], z[1], 37800, 4, tail), 0, pcm);
            }
    // ---- every refusal of test_every_refusal, what is accepted next to them, and base or den past an int in every format
    {
        const uint32_t LOOP = PSXHIP_STRSPU_LOOP, NODUMMY = PSXHIP_STRSPU_NO_LEADING_DUMMY;
        const psxhip_str_settings_t list[] = {
            settings(FORMAT_STRSPU, 15, 1, 2, 0, 2, 44100, 4, REFERENCE),
            settings(FORMAT_STRSPU, 15, 1, 1, 0, 2, 200000, 4, COMPLETE),
            settings(FORMAT_STRSPU, 15, 1, 1, 0, 2, 132300, 4, COMPLETE),
            settings(FORMAT_STRSPU, 15, 1, 2, 0, 2, 44100, 4, COMPLETE, 0x0001u | 1u << 18),
            settings(FORMAT_STRSPU, 15, 1, 2, 0, 2, 44100, 4, COMPLETE, 0x0001u | 1u << 24),
            settings(FORMAT_STRSPU, 15, 1, 2, 0, 2, 44100, 4, COMPLETE, 0x0001u | 1u << 31),
            settings(FORMAT_STRSPU, 15, 1, 2, 0, 2, 44100, 4, COMPLETE, 0x8001),
            settings(FORMAT_STRSPU, 15, 1, 2, 0, 2, 44100, 4, COMPLETE, 0x0042, 0x0042),
            settings(FORMAT_STRSPU, 15, 1, 2, 0, 3, 44100, 4, COMPLETE),
            settings(FORMAT_STRSPU, 15, 1, 2, 0, 2, 0, 4, COMPLETE),
            settings(FORMAT_STRSPU, 15, 1, 2, 0, 2, -44100, 4, COMPLETE),
            settings(FORMAT_STRSPU, 2000000, 1, 2, 0, 2, 32000, 4, COMPLETE),
            settings(FORMAT_STRSPU, 151, 1, 2, 0, 2, 44100, 4, COMPLETE),
            settings(FORMAT_STRSPU, 15, 1, 1, 0, 2, 100000, 4, COMPLETE),
            settings(FORMAT_STRSPU, 15, 1, 2, 0, 2, 44100, 4, COMPLETE, 0xFFFFu | LOOP | NODUMMY),
            settings(FORMAT_STRSPU, 1, 2000000, 2, 0, 2, 32000, 4, COMPLETE),
            settings(FORMAT_STRCD, 1, 1 << 30, 2, 0, 2, 37800, 4, REFERENCE),
            settings(FORMAT_STRCD, 0x7FFFFFFF, 1, 2, 0, 2, 37800, 4, COMPLETE),
            settings(FORMAT_STRV, 1, 0x7FFFFFFF, 2, 0, 0, 37800, 4, COMPLETE),
            settings(FORMAT_STRV, 0x7FFFFFFF, 0x7FFFFFFF / 150, 2, 0, 0, 37800, 4, COMPLETE),
        };
        for (const psxhip_str_settings_t& s : list) {
            printf("settings %d %d %d %d %d %d %d %d %u %d", s.format, s.str_fps_num, s.str_fps_den, s.str_cd_speed, s.audio_channels, s.audio_frequency,
                   s.audio_bit_depth, s.tail_mode, (unsigned)s.strspu_options, s.str_video_id);
            print_plan(s, 3, 0);
        }
    }
    // ---- strspu_place_host over blocks of the recurrence (seed 1 + channels + 10 K)
    for (int ch = 1; ch <= 2; ch++)
        for (int K = 1; K <= 3; K++)
            for (uint32_t flags : {0u, (uint32_t)PSXHIP_STRSPU_LOOP, (uint32_t)PSXHIP_STRSPU_NO_LEADING_DUMMY,
                                   (uint32_t)(PSXHIP_STRSPU_LOOP | PSXHIP_STRSPU_NO_LEADING_DUMMY)}) {
                const uint32_t options = 0x0001u | flags;
                const StrspuLayout x = strspu_layout(ch, 44100, 2);
                const size_t U = (size_t)K * x.blocks - strspu_dummy_of(options);
                const std::vector<uint8_t> blocks = recurrence(1u + ch + 10u * K, (size_t)ch * U * 16);
                std::vector<uint8_t> out((size_t)K * 2048, 0xEE);
                strspu_place_host(x, 44100, options, K, blocks.data(), out.data());
                printf("place %d %d %u : ", ch, K, options);
                print_hex(out.data(), out.size());
            }
    // ---- str_video_chunk_header: the first and the last chunk of a frame of three, bitstream bytes from the recurrence (seed 7)
    {
        psxhip_str_settings_t s = settings(FORMAT_STRV, 15, 1, 2, 0, 0, 37800, 4, COMPLETE);
        s.video_width = 320;
        s.video_height = 240;
        const int budget = 3 * 2016, frame = 299;
        const std::vector<uint8_t> bs = recurrence(7, 8);       // (the header quotes the bitstream's first 8 bytes and no more)
        for (int chunk : {0, 2}) {
            std::vector<uint8_t> hd(32, 0xEE);
            str_video_chunk_header(hd.data(), &s, frame, chunk, budget, 5004, bs.data());
            printf("vhdr %d %d %d %d %d %d %d : ", s.str_video_id, s.video_width, s.video_height, frame, chunk, budget, 5004);
            print_hex(hd.data(), hd.size());
        }
    }
    return 0;
}
