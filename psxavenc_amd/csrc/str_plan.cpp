// str_plan.cpp -- the STR muxer's sector plan and the bytes the host writes itself (str_plan.h).  What psxavenc's encode_file_str
// decides sector by sector (psxavenc/filefmt.c:391-520 around encode_sector_str, mdec.c:757-836) is a function of the settings, the
// frame count and the amount of audio: make_plan runs the loop dry.  No HIP and no device: psxhip_str.cpp encodes what the plan names.
#include "str_plan.h"

#include <math.h>
#include <string.h>

#include "../../include/psxav_audio.h"

static void put_le16(uint8_t* p, unsigned v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
static void put_le32(uint8_t* p, unsigned v) { put_le16(p, v & 0xFFFF); put_le16(p + 2, v >> 16); }

void str_video_chunk_header(uint8_t* hd, const psxhip_str_settings_t* s, int frame, int chunk, int budget, uint32_t bytes_used, const uint8_t* frame_bs) {
    put_le16(hd + 0x00, 0x0160);
    put_le16(hd + 0x02, (unsigned)s->str_video_id);
    put_le16(hd + 0x04, (unsigned)chunk);
    put_le16(hd + 0x06, (unsigned)(budget / 2016));
    put_le32(hd + 0x08, (unsigned)(frame + 1));                         // frame_index counts from 1
    put_le32(hd + 0x0C, bytes_used);
    put_le16(hd + 0x10, (unsigned)s->video_width);
    put_le16(hd + 0x12, (unsigned)s->video_height);
    memcpy(hd + 0x14, frame_bs, 8);
    put_le32(hd + 0x1C, 0);
}

// (bytes not set here are zero)
void strspu_chunk_header(uint8_t* hd, const StrspuLayout& x, int frequency, uint32_t options, int k, int K) {
    const int d = strspu_dummy_of(options);
    memset(hd, 0, 32);
    put_le16(hd + 0x00, 0x0160);
    put_le16(hd + 0x02, options & PSXHIP_STRSPU_ID_MASK);
    put_le16(hd + 0x04, 0);
    put_le16(hd + 0x06, 1);
    put_le32(hd + 0x08, (unsigned)(k + 1));
    put_le32(hd + 0x0C, 2016);
    put_le16(hd + 0x10, (unsigned)x.channels);
    put_le16(hd + 0x12, (unsigned)x.lane_bytes);
    put_le32(hd + 0x14, (unsigned)frequency);
    put_le32(hd + 0x18, k == 0 ? 0u : 28u * (unsigned)(k * x.blocks - d));
    put_le16(hd + 0x1C, (k == K - 1 ? 1u : 0u) | ((k == 0 && d) ? 2u : 0u) | ((options & PSXHIP_STRSPU_LOOP) ? 4u : 0u));
}

void strspu_place_host(const StrspuLayout& x, int frequency, uint32_t options, int K, const uint8_t* blocks, uint8_t* out) {
    const int d = strspu_dummy_of(options), B = x.blocks;
    const size_t U = (size_t)K * B - d;
    for (int k = 0; k < K; k++) {
        uint8_t* sec = out + (size_t)k * 2048;
        strspu_chunk_header(sec, x, frequency, options, k, K);
        for (int c = 0; c < x.channels; c++) {
            uint8_t* lane = sec + 0x20 + (size_t)c * x.lane_bytes;
            for (int b = 0; b < B; b++) {
                const long long u = (long long)k * B + b - d;
                if (u < 0) memset(lane + 16 * b, 0, 16);                        // leading silent block, filefmt.c:331-335
                else memcpy(lane + 16 * b, blocks + ((size_t)c * U + (size_t)u) * 16, 16);
            }
            uint8_t* last = lane + 16 * (B - 1);                                // filefmt.c:343-358
            if (options & PSXHIP_STRSPU_LOOP) {
                last[1] = PSX_AUDIO_SPU_LOOP_REPEAT;
            } else if (k == K - 1) {
                memset(last, 0, 16);
                last[1] = PSX_AUDIO_SPU_LOOP_TRAP;
            }
        }
    }
}

const char* settings_error(const psxhip_str_settings_t* s) {
    static const char* const bad = "psxhip_str: bad settings";
    if (!s) return bad;
    if (s->format != FORMAT_STR && s->format != FORMAT_STRCD && s->format != FORMAT_STRV && s->format != FORMAT_STRSPU) return bad;
    if (s->video_codec < 0 || s->video_codec > 2 || s->video_width <= 0 || s->video_height <= 0 ||
        (s->video_width % 16) || (s->video_height % 16))
        return bad;
    if (s->str_fps_num <= 0 || s->str_fps_den <= 0 || (s->str_cd_speed != 1 && s->str_cd_speed != 2)) return bad;
    if (s->audio_channels < 0 || s->audio_channels > 2) return bad;
    if (s->tail_mode != PSXHIP_STR_TAIL_REFERENCE && s->tail_mode != PSXHIP_STR_TAIL_COMPLETE) return bad;
    if (s->format == FORMAT_STRSPU) {
        if (s->tail_mode != PSXHIP_STR_TAIL_COMPLETE)
            return "psxhip_str: format 8 (STRSPU) defines PSXHIP_STR_TAIL_COMPLETE only: the reference has no strspu loop whose tail could be mirrored";
        if ((uint32_t)s->strspu_options & ~kStrspuOptionBits) return "psxhip_str: unknown bit set in strspu_options";
        if (s->audio_channels) {
            if (((uint32_t)s->strspu_options & PSXHIP_STRSPU_ID_MASK) == ((uint32_t)s->str_video_id & 0xFFFFu))
                return "psxhip_str: the audio chunk id of strspu_options equals str_video_id";
            if (s->audio_frequency <= 0) return bad;
            const StrspuLayout x = strspu_layout(s->audio_channels, s->audio_frequency, s->str_cd_speed);
            if (x.p >= x.q) return "psxhip_str: audio rate too high for this CD speed";
        }
        return nullptr;
    }
    if (s->audio_channels && ((s->audio_frequency != 18900 && s->audio_frequency != 37800) ||
                              (s->audio_bit_depth != 4 && s->audio_bit_depth != 8)))
        return bad;
    return nullptr;
}

StrRates str_rates(const psxhip_str_settings_t* s) {
    StrRates r = {};
    const int ch = s->audio_channels;
    r.interleave = r.vpb = 1;
    r.spu = s->format == FORMAT_STRSPU && ch;
    r.sector_size = s->format == FORMAT_STRSPU ? 2048 : xa_layout(s->format == FORMAT_STRCD, ch == 2, s->audio_bit_depth).sector_bytes;
    if (r.spu) {
        // p / q of the sectors are audio: the budgets are mdec.c:768-775's with (q - p) / q of 75 x speed sectors a second for video
        // -- for p / q = 1 / N the numbers of filefmt.c:428-429
        const StrspuLayout& x = r.spu_layout = strspu_layout(ch, s->audio_frequency, s->str_cd_speed);
        r.samples_per_sector = x.samples_per_sector;
        r.interleave = x.q % x.p == 0 ? (int)(x.q / x.p) : 0;
        r.base = 75ll * s->str_cd_speed * (x.q - x.p) * s->str_fps_den;
        r.den = x.q * s->str_fps_num;
        return r;
    }
    if (ch) {                             // 1/N audio, (N-1)/N video, filefmt.c:399-403
        r.interleave = xa_sector_interleave(ch == 2, s->audio_frequency, s->audio_bit_depth) * s->str_cd_speed;
        r.samples_per_sector = xa_layout(0, ch == 2, s->audio_bit_depth).samples_per_sector / ch;
        r.vpb = r.interleave - 1;
    }
    r.base = 75ll * s->str_cd_speed * r.vpb * s->str_fps_den;
    r.den = (int64_t)r.interleave * s->str_fps_num;
    return r;
}

// The sector loop of encode_file_str (filefmt.c:450-503) run dry: which frame slice / audio sector lands in which sector
// follows from the frame count, the amount of audio and the settings alone.
//
// tail_mode PSXHIP_STR_TAIL_REFERENCE models the reference's decoder (decoding.c:510-560) for an input that is all there:
// ensure_av_data(needed_audio, frames_needed) raises end_of_input as soon as no more than one sector's worth of audio or no
// more than `frames_needed` frames are left to hand out (its loop polls while count <= needed, and the only way out with
// nothing left to read is end_of_input = true).  From then on the loop runs until the current frame is written out
// (filefmt.c:450) -- the last frames_needed frames are never encoded (the FIXME at :442) -- every audio sector is finalised
// (:492-493), and an audio slot with no samples left stays as the sector buffer was (zero here) and widens the video share of
// the trailing-audio schedule (:483-484).
// PSXHIP_STR_TAIL_COMPLETE: every frame is encoded, the stream ends with the last frame's last sector, short audio is padded
// with silence and only the last audio sector carries EOF.
int make_plan(const psxhip_str_settings_t* s, int n_frames, int64_t pcm_samples_per_channel, Plan* pl) {
    if (const char* why = settings_error(s)) {
        psxhip_set_error("%s", why);
        return PSXHIP_EINVAL;
    }
    if (n_frames < 0 || pcm_samples_per_channel < 0) {
        psxhip_set_error("psxhip_str: bad settings");
        return PSXHIP_EINVAL;
    }
    memset(&pl->pub, 0, sizeof pl->pub);
    pl->budgets.clear();
    pl->sectors.clear();
    pl->n_audio = 0;
    pl->audio_samples = 0;
    const StrRates& r = pl->rates = str_rates(s);
    const int ch = s->audio_channels, sps = r.samples_per_sector, interleave = r.interleave;
    const int64_t base = r.base, den = r.den;
    if (base > 0x7FFFFFFFll || den > 0x7FFFFFFFll) {
        psxhip_set_error("psxhip_str: frame rate and audio rate do not fit the budget arithmetic (base %lld, den %lld)", (long long)base, (long long)den);
        return PSXHIP_EINVAL;
    }
    pl->pub.sector_size = r.sector_size;
    pl->pub.interleave = interleave;
    pl->pub.audio_samples_per_sector = sps;
    if (base / den < 1) {
        psxhip_set_error("psxhip_str: a frame would get no sector (frame rate too high for this CD speed)");
        return PSXHIP_EINVAL;
    }
    // filefmt.c:443-446
    int vpb = r.vpb;
    const double frame_size = (double)base / (double)den;
    int frames_needed = (int)ceil((double)vpb / frame_size);
    if (frames_needed < 2) frames_needed = 2;
    const bool reference = s->tail_mode == PSXHIP_STR_TAIL_REFERENCE;

    long long V = n_frames;                                    // frames the decoder still holds
    long long A = ch ? pcm_samples_per_channel * ch : 0;       // interleaved samples the decoder still holds
    bool eoi = false;
    int offset = 0, max_size = 0, frame = -1, audio_sectors = 0, video_sectors = 0, max_budget = 0;
    long long num = 0;
    // complete mode: the audio slots of the whole stream are filled (silence when the PCM runs out)
    for (long long n = 0;; n++) {
        if (reference) {
            if (eoi && offset >= max_size) break;              // loop condition, filefmt.c:450
            const long long needed_audio = (long long)sps * ch;
            if ((needed_audio && A <= needed_audio) || V <= frames_needed) eoi = true;     // ensure_av_data, decoding.c:540-553
        } else if (frame + 1 >= n_frames && offset >= max_size) {
            break;
        }
        if (n > 0x7FFFFFF0ll) {
            psxhip_set_error("psxhip_str: stream too long");
            return PSXHIP_EINVAL;
        }
        bool video;                                            // filefmt.c:454-461
        if (!sps) video = true;
        else if (r.spu) video = strspu_audio_before(r.spu_layout, s->trailing_audio != 0, n + 1) == strspu_audio_before(r.spu_layout, s->trailing_audio != 0, n);
        else if (s->trailing_audio) video = (n % interleave) < vpb;
        else video = (n % interleave) > 0;
        psxhip_str_sector_t sec = {PSXHIP_STR_SECTOR_EMPTY, -1, -1, 0};
        if (video) {
            // a video slot with no frame left to start (n_frames == 0: the reference asserts in its decoder's retire_av_data, there
            // is nothing to mirror): the stream ends here -- empty, or the audio sectors before this slot
            if (offset >= max_size && V <= 0) break;
            while (offset >= max_size) {                       // encode_sector_str moves on to the next frame, mdec.c:768-780
                frame++;
                num += base;                                   // (base + den - 1 < 2^32: no overflow in 64 bits)
                max_size = (int)(num / den * 2016);
                num %= den;
                offset = 0;
                pl->budgets.push_back(max_size);
                if (max_size > max_budget) max_budget = max_size;
                V--;
            }
            sec.kind = PSXHIP_STR_SECTOR_VIDEO;
            sec.frame = frame;
            sec.index = offset / 2016;
            offset += 2016;
            video_sectors++;
        } else if (reference) {
            long long sl = A / ch;                             // filefmt.c:476-484
            if (sl > sps) sl = sps;
            if (!sl) vpb++;
            if (sl) {
                sec.kind = PSXHIP_STR_SECTOR_AUDIO;
                sec.index = audio_sectors++;
                sec.eof = eoi ? 1 : 0;                         // :492-493 (finalize does nothing to a sector of length 0)
                pl->audio_samples += sl;
                A -= sl * ch;
            }
        } else {
            sec.kind = PSXHIP_STR_SECTOR_AUDIO;
            sec.index = audio_sectors++;
            pl->audio_samples += sps;
        }
        pl->sectors.push_back(sec);
    }
    if (!reference && audio_sectors > 0)                       // only the last audio sector carries EOF
        for (size_t i = pl->sectors.size(); i-- > 0;)
            if (pl->sectors[i].kind == PSXHIP_STR_SECTOR_AUDIO) { pl->sectors[i].eof = 1; break; }
    // STRSPU: the K audio sectors hold K B blocks per channel, the first of them the dummy block: the chains encode U = K B - d units,
    // the PCM is fitted to 28 U samples (silence behind a shorter one)
    if (r.spu && 28ll * audio_sectors * r.spu_layout.blocks > 0x7FFFFFFFll) {          // (a chain's sample limit is an int)
        psxhip_set_error("psxhip_str: stream too long");
        return PSXHIP_EINVAL;
    }
    if (r.spu) pl->audio_samples = audio_sectors ? 28ll * ((long long)audio_sectors * r.spu_layout.blocks - strspu_dummy_of((uint32_t)s->strspu_options)) : 0;
    pl->n_audio = audio_sectors;
    pl->pub.n_sectors = (int32_t)pl->sectors.size();
    pl->pub.n_video_sectors = video_sectors;
    pl->pub.n_audio_sectors = (int32_t)pl->sectors.size() - video_sectors;
    pl->pub.n_frames_encoded = frame + 1;
    pl->pub.max_frame_size = max_budget;
    return PSXHIP_OK;
}
