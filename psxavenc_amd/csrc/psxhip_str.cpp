// psxhip_str.cpp -- batched STR / STRCD / STRV muxer (include/psxav_hip.h, psxhip_str_*).
//
// What psxavenc's encode_file_str does sector by sector (psxavenc/filefmt.c:391-520 with :73-91, around
// encode_sector_str, mdec.c:757-836, and psx_audio_xa_encode, adpcm.c:293-332), restated for inputs that are all
// there up front: the sector loop is first run dry (make_plan: which frame slice / audio sector lands where, which
// frames are part of the stream at all, which audio sectors carry EOF -- incl. the reference's end-of-input model);
// the per-frame byte budgets are a closed-form function of the frame index (mdec.c:768-775), so every frame is encoded
// in ONE batched MDEC call sharded over the handle's devices; the audio is one XA stream encoded by the ADPCM kernels
// concurrently (its own host thread and stream); the host then cuts the finished frames into sectors and interleaves
// them with the finished audio sectors.  No encoding happens on the host.  No process-global state: everything kept
// between calls lives in a psxhip_str_ctx_t.
//
// Format 8 (STRSPU, "psxhip STRSPU v1") is the same muxer with another audio leg: the sector schedule is a
// rational share p / q of audio sectors (host_layout.h: strspu_layout), the audio is one SPU-ADPCM chain per channel (5 filters,
// 4-bit), and an audio sector is a chunk header and 126 SPU blocks placed as the SPUI writer places them (filefmt.c:323-371) --
// on the device by strspu_kernels.hip, on the host by strspu_place_host below.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/psxav_audio.h"
#include "../../include/psxav_hip.h"
#include "../../include/psxav_mdec.h"
#include "device_buffer.h"
#include "host_layout.h"
#include "psxhip_adpcm_internal.h"
#include "psxhip_internal.h"

namespace {
struct Sector {
    int32_t frame;      // >= 0: video sector of that frame; -1: audio sector; -2: audio slot with no samples left
    int32_t at;         // video: byte offset into the frame's bitstream; audio: index of the XA sector
    uint8_t eof;        // audio: EOF submode bit (psx_audio_xa_encode_finalize)
};

struct Plan {
    psxhip_str_plan_t pub;
    int base, den;                // frame_block_base_overflow / frame_block_overflow_den, filefmt.c:431-432
    std::vector<int32_t> budgets; // frame_max_size of every frame in the stream, mdec.c:768-775
    std::vector<Sector> sectors;
    int64_t audio_samples;        // per channel, handed to the XA encoder over the whole stream
};
}  // namespace

struct psxhip_str_ctx {
    // One multi-device MDEC encoder is kept between calls (creating one allocates pinned staging buffers per device, which
    // costs more than encoding a thousand frames), re-created when the geometry changes
    std::vector<int> devices;
    psxhip_mdec_multi_t* mdec = nullptr;
    int key[4] = {-1, -1, -1, -1};          // codec, width, height, max_frame_size
    // ... and so is the buffer the frames' bitstreams land in before they are cut into sectors: page-locked, so the MDEC
    // host path writes it by DMA
    uint8_t* bs = nullptr;
    size_t bs_cap = 0;
    std::mutex mu;                          // calls on ONE handle are serialised; handles are independent of each other
    // ---- psxhip_str_encode_device: everything stays in HBM (device devices[0]).  Kept between calls with the same shape: the
    //      plan's tables on the device, the buffers the frames' bitstreams / unit records pass through, one encoder context, one
    //      ADPCM session over the caller's PCM, a stream + events for the audio leg
    struct __attribute__((visibility("hidden"))) Dev {
        psxhip_str_settings_t settings;
        int n_frames = -1, n_streams = 0;
        int64_t pcm_samples = -1;
        const int16_t* d_pcm = nullptr;
        int64_t pcm_stream_stride = 0;
        bool chunked = false;           // the XA tracks of the cached shape run as a speculate-and-verify session (else: serial chains)
        Plan plan;
        int n_vtab = 0, na = 0, nf = 0;
        struct { DeviceBuffer vtab, budgets, adst, eof, bs, res, units; } buf;      // of the cached shape: dropped together
        struct { DeviceBuffer chains, base, states; } tab;                           // short audio: the serial chains kernel's tables
        psxhip_mdec_result_t* h_res = nullptr;                                 // page-locked
        psxhip_mdec_ctx_t* mdec = nullptr;
        int mdec_key[4] = {-1, -1, -1, -1};
        psxhip_adpcm_session_t* session = nullptr;
        hipStream_t astream = nullptr;
        hipEvent_t ev_in = nullptr, ev_audio = nullptr;
    } dev;
};

namespace {

void put_le16(uint8_t* p, unsigned v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
void put_le32(uint8_t* p, unsigned v) { put_le16(p, v & 0xFFFF); put_le16(p + 2, v >> 16); }

int strspu_dummy_of(uint32_t options) { return (options & PSXHIP_STRSPU_NO_LEADING_DUMMY) ? 0 : 1; }      // d: blocks the leading dummy takes

// The 32-byte chunk header of STRSPU audio sector k of K; bytes not set here are zero
void strspu_chunk_header(uint8_t* hd, const StrspuLayout& x, int frequency, uint32_t options, int k, int K) {
    const int d = strspu_dummy_of(options);
    const bool loop = (options & PSXHIP_STRSPU_LOOP) != 0;
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
    put_le16(hd + 0x1C, (k == K - 1 ? 1u : 0u) | ((k == 0 && d) ? 2u : 0u) | (loop ? 4u : 0u));
}

// The host path's block placement: K audio sectors from every channel's U = K B - d encoded blocks (blocks: channel c's at
// c * U * 16), as strspu_audio_sector_kernel builds them on the device
void strspu_place_host(const StrspuLayout& x, int frequency, uint32_t options, int K, const uint8_t* blocks, uint8_t* out) {
    const int d = strspu_dummy_of(options), B = x.blocks;
    const bool loop = (options & PSXHIP_STRSPU_LOOP) != 0;
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
            if (loop) {
                last[1] = PSX_AUDIO_SPU_LOOP_REPEAT;
            } else if (k == K - 1) {
                memset(last, 0, 16);
                last[1] = PSX_AUDIO_SPU_LOOP_TRAP;
            }
        }
    }
}

psx_audio_xa_settings_t xa_settings_of(const psxhip_str_settings_t* s) {
    psx_audio_xa_settings_t x;          // args_to_libpsxav_xa_audio, filefmt.c:55-71
    memset(&x, 0, sizeof x);
    x.bits_per_sample = s->audio_bit_depth;
    x.frequency = s->audio_frequency;
    x.stereo = s->audio_channels == 2;
    x.file_number = s->audio_xa_file;
    x.channel_number = s->audio_xa_channel;
    x.format = s->format == FORMAT_STRCD ? PSX_AUDIO_XA_FORMAT_XACD : PSX_AUDIO_XA_FORMAT_XA;
    return x;
}

constexpr uint32_t kStrspuOptionBits = PSXHIP_STRSPU_ID_MASK | PSXHIP_STRSPU_LOOP | PSXHIP_STRSPU_NO_LEADING_DUMMY;

// nullptr, or what is wrong with the settings
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
    pl->audio_samples = 0;
    const psx_audio_xa_settings_t xa = xa_settings_of(s);
    const int ch = s->audio_channels;
    const bool spu = s->format == FORMAT_STRSPU && ch;          // (STRSPU without audio is STRV: the branch below, 2048-byte sectors)
    StrspuLayout sx = {};
    int interleave = 1, sps = 0, vpb = 1;
    if (spu) {
        // p / q of the sectors are audio: the budgets are mdec.c:768-775's with (q - p) / q of 75 x speed sectors a second for video
        // -- for p / q = 1 / N the numbers of filefmt.c:428-429
        sx = strspu_layout(ch, s->audio_frequency, s->str_cd_speed);
        sps = sx.samples_per_sector;
        const int64_t base = 75ll * s->str_cd_speed * (sx.q - sx.p) * s->str_fps_den, den = sx.q * s->str_fps_num;
        if (base > 0x7FFFFFFFll || den > 0x7FFFFFFFll) {
            psxhip_set_error("psxhip_str: frame rate and audio rate do not fit the budget arithmetic (base %lld, den %lld)", (long long)base, (long long)den);
            return PSXHIP_EINVAL;
        }
        pl->base = (int)base;
        pl->den = (int)den;
        interleave = sx.q % sx.p == 0 ? (int)(sx.q / sx.p) : 0;
    } else {
        if (ch) {                             // 1/N audio, (N-1)/N video, filefmt.c:399-403
            interleave = (int)psx_audio_xa_get_sector_interleave(xa) * s->str_cd_speed;
            sps = (int)psx_audio_xa_get_samples_per_sector(xa);
            vpb = interleave - 1;
        }
        pl->base = 75 * s->str_cd_speed * vpb * s->str_fps_den;
        pl->den = interleave * s->str_fps_num;
    }
    pl->pub.sector_size = s->format == FORMAT_STRSPU ? 2048 : (int32_t)psx_audio_xa_get_buffer_size_per_sector(xa);
    pl->pub.interleave = interleave;
    pl->pub.audio_samples_per_sector = sps;
    if (pl->base / pl->den < 1) {
        psxhip_set_error("psxhip_str: a frame would get no sector (frame rate too high for this CD speed)");
        return PSXHIP_EINVAL;
    }
    // filefmt.c:443-446
    const double frame_size = (double)pl->base / (double)pl->den;
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
        else if (spu) video = strspu_audio_before(sx, s->trailing_audio != 0, n + 1) == strspu_audio_before(sx, s->trailing_audio != 0, n);
        else if (s->trailing_audio) video = (n % interleave) < vpb;
        else video = (n % interleave) > 0;
        Sector sec;
        if (video) {
            // a video slot with no frame left to start (n_frames == 0: the reference asserts in its decoder's retire_av_data, there
            // is nothing to mirror): the stream ends here -- empty, or the audio sectors before this slot
            if (offset >= max_size && V <= 0) break;
            while (offset >= max_size) {                       // encode_sector_str moves on to the next frame, mdec.c:768-780
                frame++;
                num += pl->base;                               // (base + den - 1 < 2^32: no overflow in 64 bits)
                max_size = (int)(num / pl->den * 2016);
                num %= pl->den;
                offset = 0;
                pl->budgets.push_back(max_size);
                if (max_size > max_budget) max_budget = max_size;
                V--;
            }
            sec.frame = frame;
            sec.at = offset;
            sec.eof = 0;
            offset += 2016;
            video_sectors++;
        } else if (reference) {
            long long sl = A / ch;                             // filefmt.c:476-484
            if (sl > sps) sl = sps;
            if (!sl) vpb++;
            sec.frame = sl ? -1 : -2;
            sec.at = sl ? audio_sectors : 0;
            sec.eof = (eoi && sl) ? 1 : 0;                     // :492-493 (finalize does nothing to a sector of length 0)
            if (sl) {
                audio_sectors++;
                pl->audio_samples += sl;
                A -= sl * ch;
            }
        } else {
            sec.frame = -1;
            sec.at = audio_sectors++;
            sec.eof = 0;
            pl->audio_samples += sps;
        }
        pl->sectors.push_back(sec);
    }
    if (!reference && audio_sectors > 0)                       // only the last audio sector carries EOF
        for (size_t i = pl->sectors.size(); i-- > 0;)
            if (pl->sectors[i].frame == -1) { pl->sectors[i].eof = 1; break; }
    // STRSPU: the K audio sectors hold K B blocks per channel, the first of them the dummy block: the chains encode U = K B - d units,
    // the PCM is fitted to 28 U samples (silence behind a shorter one)
    if (spu && 28ll * audio_sectors * sx.blocks > 0x7FFFFFFFll) {          // (a chain's sample limit is an int)
        psxhip_set_error("psxhip_str: stream too long");
        return PSXHIP_EINVAL;
    }
    if (spu) pl->audio_samples = audio_sectors ? 28ll * ((long long)audio_sectors * sx.blocks - strspu_dummy_of((uint32_t)s->strspu_options)) : 0;
    pl->pub.n_sectors = (int32_t)pl->sectors.size();
    pl->pub.n_video_sectors = video_sectors;
    pl->pub.n_audio_sectors = (int32_t)pl->sectors.size() - video_sectors;
    pl->pub.n_frames_encoded = frame + 1;
    pl->pub.max_frame_size = max_budget;
    return PSXHIP_OK;
}

}  // namespace

namespace {
void free_dev(psxhip_str_ctx* c) {
    psxhip_str_ctx::Dev& d = c->dev;
    (void)hipSetDevice(c->devices[0]);
    if (d.astream) (void)hipStreamSynchronize(d.astream);
    if (d.session) psxhip_adpcm_session_destroy(d.session);
    if (d.mdec) psxhip_mdec_destroy(d.mdec);
    d.buf = {};
    d.tab = {};
    if (d.h_res) (void)hipHostFree(d.h_res);
    if (d.ev_in) (void)hipEventDestroy(d.ev_in);
    if (d.ev_audio) (void)hipEventDestroy(d.ev_audio);
    if (d.astream) (void)hipStreamDestroy(d.astream);
    d.h_res = nullptr; d.ev_in = nullptr; d.ev_audio = nullptr; d.astream = nullptr; d.session = nullptr; d.mdec = nullptr;
    d.n_frames = -1;
}
}  // namespace

extern "C" int psxhip_str_create(psxhip_str_ctx_t** out, const int* devices, int n_devices) {
    if (!out) return PSXHIP_EINVAL;
    *out = nullptr;
    if (!devices || n_devices < 1 || n_devices > 64) {
        psxhip_set_error("psxhip_str_create: need 1..64 devices");
        return PSXHIP_EINVAL;
    }
    const int have = psxhip_device_count();
    if (have <= 0) return psxhip_no_device();
    for (int i = 0; i < n_devices; i++)
        if (devices[i] < 0 || devices[i] >= have) {
            psxhip_set_error("psxhip_str_create: device %d out of range (%d visible)", devices[i], have);
            return PSXHIP_EINVAL;
        }
    psxhip_str_ctx* c = new (std::nothrow) psxhip_str_ctx;
    if (!c) return PSXHIP_ENOMEM;
    c->devices.assign(devices, devices + n_devices);
    *out = c;
    return PSXHIP_OK;
}

extern "C" void psxhip_str_destroy(psxhip_str_ctx_t* c) {
    if (!c) return;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        psxhip_mdec_multi_destroy(c->mdec);
        c->mdec = nullptr;
        if (c->bs) {
            (void)hipSetDevice(c->devices[0]);
            (void)hipHostFree(c->bs);
        }
        c->bs = nullptr;
        free_dev(c);
    }
    delete c;
}

extern "C" int psxhip_str_plan(const psxhip_str_settings_t* settings, int n_frames, int64_t pcm_samples_per_channel,
                               psxhip_str_plan_t* plan) {
    Plan pl;
    const int rc = make_plan(settings, n_frames, pcm_samples_per_channel, &pl);
    if (plan) *plan = pl.pub;
    return rc;
}

extern "C" int psxhip_str_plan_sectors(const psxhip_str_settings_t* settings, int n_frames, int64_t pcm_samples_per_channel,
                                       psxhip_str_sector_t* sectors, int cap) {
    Plan pl;
    const int rc = make_plan(settings, n_frames, pcm_samples_per_channel, &pl);
    if (rc) return rc;
    const int n = (int)pl.sectors.size();
    for (int i = 0; i < n && i < cap && sectors; i++) {
        const Sector& sc = pl.sectors[(size_t)i];
        sectors[i].kind = sc.frame >= 0 ? PSXHIP_STR_SECTOR_VIDEO : (sc.frame == -1 ? PSXHIP_STR_SECTOR_AUDIO : PSXHIP_STR_SECTOR_EMPTY);
        sectors[i].frame = sc.frame >= 0 ? sc.frame : -1;
        sectors[i].index = sc.frame >= 0 ? sc.at / 2016 : (sc.frame == -1 ? sc.at : -1);
        sectors[i].eof = sc.eof;
    }
    return n;
}

extern "C" int psxhip_str_frame_budgets(const psxhip_str_settings_t* settings, int first_frame, int n_frames, int32_t* budgets) {
    if (!budgets || first_frame < 0 || n_frames < 0) return PSXHIP_EINVAL;
    // the budget sequence does not depend on how the stream ends: plan all frames in the complete mode (mdec.c:768-775)
    psxhip_str_settings_t s2;
    if (const char* why = settings_error(settings)) {          // (a tail the format does not define is refused here too)
        psxhip_set_error("%s", why);
        return PSXHIP_EINVAL;
    }
    s2 = *settings;
    s2.tail_mode = PSXHIP_STR_TAIL_COMPLETE;
    Plan pl;
    const int rc = make_plan(&s2, first_frame + n_frames, 0, &pl);
    if (rc) return rc;
    for (int i = 0; i < n_frames; i++) budgets[i] = pl.budgets[(size_t)(first_frame + i)];
    return PSXHIP_OK;
}

extern "C" int psxhip_str_encode_host(psxhip_str_ctx_t* c, const psxhip_str_settings_t* s, const uint8_t* frames, int n_frames,
                                      const int16_t* pcm, int64_t pcm_samples_per_channel, uint8_t* out, size_t out_size,
                                      psxhip_str_plan_t* plan_out) {
    if (!c) {
        psxhip_set_error("psxhip_str_encode_host: NULL handle");
        return PSXHIP_EINVAL;
    }
    Plan pl;
    int rc = make_plan(s, n_frames, pcm_samples_per_channel, &pl);
    if (plan_out) *plan_out = pl.pub;
    if (rc) return rc;
    const int ns = pl.pub.n_sectors;
    if (ns == 0) return PSXHIP_OK;
    const int nf = pl.pub.n_frames_encoded;
    if (nf > n_frames) {      // (a plan never takes a frame the caller did not hand over)
        psxhip_set_error("psxhip_str_encode_host: internal error: plan encodes %d of %d frames", nf, n_frames);
        return PSXHIP_EINVAL;
    }
    if ((nf && !frames) || !out || (s->audio_channels && !pcm && pcm_samples_per_channel > 0)) {
        psxhip_set_error("psxhip_str_encode_host: NULL argument");
        return PSXHIP_EINVAL;
    }
    const size_t ssz = (size_t)pl.pub.sector_size;
    if (out_size < ssz * (size_t)ns) {
        psxhip_set_error("psxhip_str_encode_host: output needs %zu bytes, %zu given", ssz * (size_t)ns, out_size);
        return PSXHIP_EINVAL;
    }

    // ---- video: every frame of the stream in one batched call, sharded over the handle's devices
    std::lock_guard<std::mutex> call(c->mu);
    const int device = c->devices[0];
    const size_t ostride = (size_t)pl.pub.max_frame_size;
    if ((size_t)nf * ostride > c->bs_cap) {
        if (hipSetDevice(device) != hipSuccess) { psxhip_set_error("psxhip_str_encode_host: no such device %d", device); return PSXHIP_EDEVICE; }
        if (c->bs) (void)hipHostFree(c->bs);
        c->bs = nullptr;
        c->bs_cap = 0;
        // page-locked for every device of the list (the default flags of a multi-GPU process map it for all of them)
        if (hipHostMalloc((void**)&c->bs, (size_t)nf * ostride, hipHostMallocPortable) != hipSuccess) {
            (void)hipGetLastError();
            psxhip_set_error("psxhip_str_encode_host: out of pinned host memory (%zu bytes)", (size_t)nf * ostride);
            return PSXHIP_ENOMEM;
        }
        c->bs_cap = (size_t)nf * ostride;
    }
    uint8_t* const bs = c->bs;
    std::vector<psxhip_mdec_result_t> res((size_t)(nf ? nf : 1));
    int rc_video = PSXHIP_OK;
    char err_video[256] = "";
    std::vector<uint8_t> xa_out;
    int geo_size = 0, sub_at = 0, at = 0;                       // `at`: where a sector keeps its chunk header
    (void)str_sector_geometry(s->format, &geo_size, &sub_at, &at);
    // Which frame slice / audio sector lands in which sector is in the plan; the sectors themselves (2 KiB of copying and a
    // 2 KiB EDC each) are built by a few threads, each on its own range.
    // `video`: build the video sectors of [n0, n1), else its audio sectors -- the two kinds are built by different threads at
    // different times (whichever of the frame encode and the XA encode finishes first has its sectors cut while the other runs)
    auto build = [&](int n0, int n1, bool video) {
        uint8_t sector[PSX_CDROM_SECTOR_SIZE];
        for (int n = n0; n < n1; n++) {
            uint8_t* dst = out + (size_t)n * ssz;
            const Sector& sc = pl.sectors[(size_t)n];
            const int frame = sc.frame, offset = sc.at;
            if ((frame >= 0) != video) continue;
            if (frame >= 0) {
                const int budget = pl.budgets[(size_t)frame];
                memset(sector, 0, sizeof sector);            // the reference's buffer is an uninitialised stack array
                // init_sector_buffer_video, filefmt.c:73-91
                psx_cdrom_sector_xa_subheader_t* sub = nullptr;
                if (s->format == FORMAT_STRCD) {
                    psx_cdrom_init_sector((psx_cdrom_sector_t*)sector, n, PSX_CDROM_SECTOR_TYPE_MODE2_FORM1);
                    sub = ((psx_cdrom_sector_t*)sector)->mode2.subheader;
                } else if (s->format == FORMAT_STR) {
                    sub = (psx_cdrom_sector_xa_subheader_t*)sector;
                }
                if (sub) {
                    sub->file = (uint8_t)s->audio_xa_file;
                    sub->channel = (uint8_t)(s->audio_xa_channel & PSX_CDROM_SECTOR_XA_CHANNEL_MASK);
                    sub->submode = PSX_CDROM_SECTOR_XA_SUBMODE_DATA | PSX_CDROM_SECTOR_XA_SUBMODE_RT;
                    sub->coding = 0;
                    sub[1] = sub[0];
                }
                // the 32-byte chunk header + 2016 payload bytes of encode_sector_str, mdec.c:782-832
                const uint8_t* fo = bs + (size_t)frame * ostride;
                uint8_t* hd = sector + at;
                put_le16(hd + 0x00, 0x0160);
                put_le16(hd + 0x02, (unsigned)s->str_video_id);
                put_le16(hd + 0x04, (unsigned)(offset / 2016));
                put_le16(hd + 0x06, (unsigned)(budget / 2016));
                put_le32(hd + 0x08, (unsigned)(frame + 1));                         // frame_index counts from 1
                put_le32(hd + 0x0C, (unsigned)res[(size_t)frame].bytes_used);
                put_le16(hd + 0x10, (unsigned)s->video_width);
                put_le16(hd + 0x12, (unsigned)s->video_height);
                memcpy(hd + 0x14, fo, 8);
                put_le32(hd + 0x1C, 0);
                memcpy(hd + 0x20, fo + offset, 2016);
                psx_cdrom_calculate_checksums((psx_cdrom_sector_t*)sector, PSX_CDROM_SECTOR_TYPE_MODE2_FORM1);
                memcpy(dst, sector, ssz);
            } else if (frame == -2) {
                // no samples left: psx_audio_xa_encode writes nothing (adpcm.c:310) and the reference puts out whatever its
                // stack buffer held; zero here
                memset(dst, 0, ssz);
            } else {
                memcpy(dst, xa_out.data() + (size_t)offset * ssz, ssz);
                if (s->format == FORMAT_STRCD) {
                    // the audio sectors were assembled with consecutive addresses; the header carries this sector's own LBA
                    // (psx_cdrom_init_sector, cdrom.c:55-74).  The form-2 EDC does not cover the header.
                    psx_cdrom_sector_t tmp;
                    psx_cdrom_init_sector(&tmp, n, PSX_CDROM_SECTOR_TYPE_MODE2_FORM2);
                    memcpy(dst + 12, (const uint8_t*)&tmp + 12, 3);
                }
            }
        }
    };
    auto build_all = [&](bool video) {
        const unsigned hw = std::thread::hardware_concurrency();
        int nt = ns >= 2048 ? (hw >= 64 ? 16 : (hw >= 16 ? 8 : (hw >= 4 ? (int)hw / 2 : 1))) : 1;
        if (!video && nt > 4) nt = 4;                       // one sector in eight, and no checksum to compute
        std::vector<std::thread> th;
        const int per = (ns + nt - 1) / nt;
        for (int t = 1; t < nt; t++)
            if (t * per < ns) th.emplace_back(build, t * per, (t + 1) * per < ns ? (t + 1) * per : ns, video);
        build(0, per < ns ? per : ns, video);
        for (auto& x : th) x.join();
    };

    std::thread video([&]() {
        if (nf == 0) return;
        const int key[4] = {s->video_codec, s->video_width, s->video_height, pl.pub.max_frame_size};
        if (!c->mdec || memcmp(key, c->key, sizeof key) != 0) {
            psxhip_mdec_multi_destroy(c->mdec);
            c->mdec = nullptr;
            rc_video = psxhip_mdec_multi_create(&c->mdec, c->devices.data(), (int)c->devices.size(), s->video_codec, s->video_width,
                                                s->video_height, pl.pub.max_frame_size);
            if (rc_video == PSXHIP_OK) memcpy(c->key, key, sizeof key);
        }
        if (rc_video == PSXHIP_OK)
            rc_video = psxhip_mdec_multi_encode_frames_host(c->mdec, frames, nf, pl.budgets.data(), 0, bs, ostride, res.data(),
                                                            PSXHIP_SCHED_STATIC, 0, nullptr);
        if (rc_video) snprintf(err_video, sizeof err_video, "%s", psxhip_last_error());     // thread-local text
        else build_all(true);
    });

    // ---- audio: one XA stream, concurrently (on the list's first device: 3 ms of work next to the frames')
    const int ch = s->audio_channels;
    int na = 0;
    for (const Sector& sc : pl.sectors) na += sc.frame == -1;
    int rc_audio = PSXHIP_OK;
    if (na > 0 && s->format == FORMAT_STRSPU) {
        // STRSPU: every channel is one SPU chain over its samples fitted to 28 U (cut, or completed with silence), all channels in one
        // batched call; the host only places the blocks
        const StrspuLayout sx = strspu_layout(ch, s->audio_frequency, s->str_cd_speed);
        const int64_t fit = pl.audio_samples;                      // 28 U, an int's worth (make_plan)
        const int64_t have = pcm_samples_per_channel < fit ? pcm_samples_per_channel : fit;
        std::vector<int16_t> planar((size_t)fit * ch, 0);
        for (int k = 0; k < ch; k++)
            for (int64_t i = 0; i < have; i++) planar[(size_t)k * fit + i] = pcm[(size_t)i * ch + k];
        std::vector<uint8_t> blocks((size_t)(fit / 28) * 16 * ch);
        psxhip_adpcm_state_t st[2] = {{0, 0}, {0, 0}};
        rc_audio = psxhip_spu_encode_streams_host(device, planar.data(), ch, fit, 1, (int)fit, st, blocks.data(), fit / 28 * 16);
        if (rc_audio >= 0) {
            xa_out.resize((size_t)na * ssz);
            strspu_place_host(sx, s->audio_frequency, (uint32_t)s->strspu_options, na, blocks.data(), xa_out.data());
            rc_audio = PSXHIP_OK;
        }
    } else if (na > 0) {
        // The XA encoder is handed pl.audio_samples per channel (the sum of the sector loop's samples_length, filefmt.c:476-479).
        // A short last sector is completed from zeros: what lies past the end of the PCM data is zero in the reference's
        // decoder buffer too (decoding.c:395-398,521-527), which is what its stereo tail over-reads.  The complete
        // mode fills every audio slot, with silence once the PCM has run out.
        const int64_t need = pl.audio_samples;
        std::vector<int16_t> padded;
        const int16_t* src = pcm;
        if (pcm_samples_per_channel < need) {
            padded.assign((size_t)need * ch, 0);
            if (pcm_samples_per_channel) memcpy(padded.data(), pcm, (size_t)pcm_samples_per_channel * ch * sizeof(int16_t));
            src = padded.data();
        }
        std::vector<uint8_t> eof((size_t)na, 0);
        for (const Sector& sc : pl.sectors)
            if (sc.frame == -1) eof[(size_t)sc.at] = sc.eof;
        xa_out.resize((size_t)na * ssz);
        psxhip_adpcm_state_t st[2] = {{0, 0}, {0, 0}};
        const int32_t lba0 = 0;
        const int fmt = s->format == FORMAT_STRCD ? 1 : 0;
        rc_audio = psxhip_xa_encode_streams_host_flags(device, fmt, ch == 2, s->audio_frequency, s->audio_bit_depth,
                                                       s->audio_xa_file, s->audio_xa_channel, src, 1, need * ch, (int)need,
                                                       &lba0, st, xa_out.data(), (int64_t)xa_out.size(), 0, eof.data());
        if (rc_audio > 0) rc_audio = rc_audio == (int)(na * ssz) ? PSXHIP_OK : PSXHIP_EINVAL;
    }
    if (rc_audio == PSXHIP_OK) build_all(false);
    video.join();
    if (rc_video) {
        psxhip_set_error("psxhip_str_encode_host: video: %s", err_video);
        return rc_video;
    }
    if (rc_audio) return rc_audio;

    long long qsum = 0;
    for (int f = 0; f < nf; f++) qsum += res[(size_t)f].quant_scale;
    pl.pub.quant_scale_sum = qsum;
    if (plan_out) *plan_out = pl.pub;
    return PSXHIP_OK;
}


// ---------------------------------------------------------------------------------------------------------------------------
// Device-resident: frames and PCM in HBM -> muxed sectors in HBM.  n_streams independent streams of the same
// settings and lengths in one call: the frames of all streams are ONE batched MDEC launch (per-frame budgets from the plan),
// their XA tracks are chains of ONE speculate-and-verify session -- S x 2 chains share the verify passes' latency, which is what
// bounds a single stream (its one tonal XA track is re-encoded serially for ~3 ms while the frames take 0.2) -- the video sectors
// are built by a scatter kernel (sector header, subheaders, chunk header, 2016-byte slice, form-1 EDC) and the audio sectors are
// assembled straight into their slots of the stream.  No PCIe, no host interleave.
extern "C" int psxhip_str_encode_device(psxhip_str_ctx_t* c, const psxhip_str_settings_t* s, int n_streams, const uint8_t* d_frames,
                                        size_t frames_stream_stride, int n_frames, const int16_t* d_pcm, int64_t pcm_stream_stride,
                                        int64_t pcm_samples_per_channel, uint8_t* d_out, size_t out_stream_stride,
                                        psxhip_str_plan_t* plan_out, void* stream) {
    if (!c || n_streams < 1 || n_streams > 4096) {
        psxhip_set_error("psxhip_str_encode_device: NULL handle or bad stream count");
        return PSXHIP_EINVAL;
    }
    if (plan_out) memset(plan_out, 0, sizeof *plan_out);
    // (what the header promises the kernels: 4-byte aligned pointers and strides; a chain's sample limit is an int)
    if (pcm_samples_per_channel < 0 || pcm_samples_per_channel > 0x7FFFFFFFll || ((uintptr_t)d_pcm & 3) || (n_streams > 1 && (pcm_stream_stride & 1)) ||
        ((uintptr_t)d_frames & 3) || ((uintptr_t)d_out & 3) || (frames_stream_stride & 3) || (out_stream_stride & 3)) {
        psxhip_set_error("psxhip_str_encode_device: pointers and strides must be 4-byte aligned, pcm_samples_per_channel within 0 .. 2^31 - 1");
        return PSXHIP_EINVAL;
    }
    std::lock_guard<std::mutex> call(c->mu);
    psxhip_str_ctx::Dev& d = c->dev;
    const int device = c->devices[0];
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    hipStream_t S = (hipStream_t)stream;
    // ---- the plan and its device tables: rebuilt when the shape of the job changes
    const bool same = d.n_frames == n_frames && d.pcm_samples == pcm_samples_per_channel && d.n_streams == n_streams && s &&
                      memcmp(&d.settings, s, sizeof *s) == 0;
    if (!same) {
        Plan pl;
        memset(&pl.pub, 0, sizeof pl.pub);
        int rc = make_plan(s, n_frames, pcm_samples_per_channel, &pl);
        if (rc) return rc;
        if (plan_out) *plan_out = pl.pub;
        // nothing of the old shape may still be running on the buffers that are about to go
        HIP_TRY(hipStreamSynchronize(S), PSXHIP_EDEVICE);
        if (d.astream) HIP_TRY(hipStreamSynchronize(d.astream), PSXHIP_EDEVICE);
        if (d.session) { psxhip_adpcm_session_destroy(d.session); d.session = nullptr; }
        d.buf = {};
        d.tab = {};
        if (d.h_res) { (void)hipHostFree(d.h_res); d.h_res = nullptr; }
        d.n_frames = -1;
        d.plan = pl;
        d.settings = *s;
        const int nf = pl.pub.n_frames_encoded, ns = pl.pub.n_sectors;
        std::vector<int32_t> vtab, adst;
        std::vector<uint8_t> eof;
        for (int n = 0; n < ns; n++) {
            const Sector& sc = pl.sectors[(size_t)n];
            if (sc.frame == -1) {
                adst.push_back(n);
                eof.push_back(sc.eof);
            } else {
                vtab.push_back(n);
                vtab.push_back(sc.frame >= 0 ? sc.frame : -2);
                vtab.push_back(sc.frame >= 0 ? sc.at : 0);
                vtab.push_back(sc.frame >= 0 ? pl.budgets[(size_t)sc.frame] : 0);
            }
        }
        d.n_vtab = (int)(vtab.size() / 4);
        d.na = (int)adst.size();
        d.nf = nf;
        const size_t ostride = ((size_t)pl.pub.max_frame_size + 3) & ~(size_t)3;
        std::vector<int32_t> budgets((size_t)nf * n_streams);
        for (int i = 0; i < n_streams; i++)
            for (int f = 0; f < nf; f++) budgets[(size_t)i * nf + f] = pl.budgets[(size_t)f];
        // (STRSPU: 126 SPU blocks per audio sector; the records are the smaller of the two kinds, so the size below covers them)
        const size_t units_per_stream = (size_t)d.na * (s->format == FORMAT_STRSPU ? 126 : xa_layout(s->format == FORMAT_STRCD, s->audio_channels == 2, s->audio_bit_depth).units_per_sector);
        auto up = [](DeviceBuffer& dst, const void* src, size_t bytes) -> int {
            const int rc = dst.reserve(bytes ? bytes : 4);
            if (rc) return rc;
            if (bytes) HIP_TRY(hipMemcpy(dst.p, src, bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
            return PSXHIP_OK;
        };
        const size_t bs_bytes = ostride * (size_t)nf * n_streams + 16;          // (never an empty allocation: a stream may hold no frame at all)
        const size_t res_bytes = sizeof(psxhip_mdec_result_t) * (size_t)(nf ? nf : 1) * n_streams;
        if ((rc = up(d.buf.vtab, vtab.data(), vtab.size() * 4)) || (rc = up(d.buf.budgets, budgets.data(), budgets.size() * 4)) ||
            (rc = up(d.buf.adst, adst.data(), adst.size() * 4)) || (rc = up(d.buf.eof, eof.data(), eof.size())) || (rc = d.buf.bs.reserve(bs_bytes)))
            return rc;
        HIP_TRY(hipMemset(d.buf.bs.p, 0, bs_bytes), PSXHIP_EDEVICE);      // (rows wider than a frame's own budget read as zero there)
        if ((rc = d.buf.res.reserve(res_bytes))) return rc;
        HIP_TRY(hipHostMalloc((void**)&d.h_res, res_bytes, hipHostMallocDefault), PSXHIP_ENOMEM);
        if ((rc = d.buf.units.reserve((units_per_stream ? units_per_stream : 1) * PSXHIP_ADPCM_RECORD_BYTES * n_streams))) return rc;
        if (!d.astream) HIP_TRY(hipStreamCreateWithFlags(&d.astream, hipStreamNonBlocking), PSXHIP_EDEVICE);
        if (!d.ev_in) HIP_TRY(hipEventCreateWithFlags(&d.ev_in, hipEventDisableTiming), PSXHIP_EDEVICE);
        if (!d.ev_audio) HIP_TRY(hipEventCreateWithFlags(&d.ev_audio, hipEventDisableTiming), PSXHIP_EDEVICE);
        d.n_frames = n_frames;
        d.pcm_samples = pcm_samples_per_channel;
        d.n_streams = n_streams;
        d.d_pcm = nullptr;           // (the ADPCM session is built below, over this call's PCM)
    }
    const Plan& pl = d.plan;
    if (plan_out) *plan_out = pl.pub;
    const int ns = pl.pub.n_sectors, nf = d.nf, na = d.na;
    if (ns == 0) return PSXHIP_OK;
    const size_t ssz = (size_t)pl.pub.sector_size;
    const size_t fsz = (size_t)s->video_width * s->video_height * 3 / 2;
    if ((nf && !d_frames) || !d_out || (na && !d_pcm) || out_stream_stride < ssz * (size_t)ns || (out_stream_stride & 3) ||
        ((uintptr_t)d_out & 3) || (nf && ((frames_stream_stride < fsz * (size_t)n_frames && n_streams > 1) || (frames_stream_stride & 3) || ((uintptr_t)d_frames & 3)))) {
        psxhip_set_error("psxhip_str_encode_device: NULL / misaligned argument, or a stream stride smaller than a stream");
        return PSXHIP_EINVAL;
    }
    const size_t ostride = ((size_t)pl.pub.max_frame_size + 3) & ~(size_t)3;

    // ---- video: one batched launch over the frames of all streams, then the sector kernel, both on the caller's stream
    psxhip_str_video_job_t vj;
    memset(&vj, 0, sizeof vj);
    vj.bs = d.buf.bs.as<const uint8_t>();
    vj.bs_stride = ostride;
    vj.bs_stream_stride = ostride * (size_t)nf;
    vj.res = d.buf.res.as<const psxhip_mdec_result_t>();
    vj.frames_per_stream = nf;
    vj.tab = d.buf.vtab.as<const int4>();
    vj.n_entries = d.n_vtab;
    vj.format = s->format;
    vj.sector_size = (int)ssz;
    vj.xa_file = s->audio_xa_file;
    vj.xa_channel = s->audio_xa_channel;
    vj.video_id = s->str_video_id;
    vj.width = s->video_width;
    vj.height = s->video_height;
    vj.out = d_out;
    vj.out_stream_stride = out_stream_stride;
    // (d_out, n_streams and the strides -- what comes from outside the library -- were checked above; the rest is this handle's own)
    auto video_sectors = [&]() -> int {
        if (vj.n_entries == 0) return PSXHIP_OK;
        const int rc = psxhip_sector_tables(device);
        if (rc) return rc;
        HIP_TRY(psxhip_str_video_sectors_launch(&vj, n_streams, S), PSXHIP_EDEVICE);
        return PSXHIP_OK;
    };
    if (nf) {
        const int key[4] = {s->video_codec, s->video_width, s->video_height, pl.pub.max_frame_size};
        if (!d.mdec || memcmp(key, d.mdec_key, sizeof key) != 0) {
            if (d.mdec) { psxhip_mdec_destroy(d.mdec); d.mdec = nullptr; }
            const int rc = psxhip_mdec_create(&d.mdec, device, s->video_codec, s->video_width, s->video_height, pl.pub.max_frame_size);
            if (rc) return rc;
            memcpy(d.mdec_key, key, sizeof key);
        }
        std::vector<psxhip_mdec_batch_t> batches;
        const bool contiguous = n_streams == 1 || (frames_stream_stride == fsz * (size_t)nf && nf == n_frames);
        for (int i = 0; i < (contiguous ? 1 : n_streams); i++) {
            psxhip_mdec_batch_t b;
            b.d_frames = d_frames + (size_t)i * frames_stream_stride;
            b.n_frames = contiguous ? nf * n_streams : nf;
            b.reserved = 0;
            b.d_frame_max_sizes = d.buf.budgets.as<const int32_t>() + (size_t)i * nf;
            b.d_out = d.buf.bs.as<uint8_t>() + (size_t)i * nf * ostride;
            b.d_results = d.buf.res.as<psxhip_mdec_result_t>() + (size_t)i * nf;
            batches.push_back(b);
        }
        const int rc = psxhip_mdec_encode_batches_device(d.mdec, batches.data(), (int)batches.size(), fsz, 0, ostride, S);
        if (rc) return rc;
    }
    // (no frame in the stream, but audio slots without samples: zero sectors -- nothing reads a bitstream)
    if (const int rc = video_sectors()) return rc;
    if (nf) HIP_TRY(hipMemcpyAsync(d.h_res, d.buf.res.p, sizeof(psxhip_mdec_result_t) * (size_t)nf * n_streams, hipMemcpyDeviceToHost, S), PSXHIP_EDEVICE);

    // ---- audio: the streams' XA tracks as chains of one session on the handle's own stream, behind the caller's inputs; the
    //      host drives the verify passes (the call is synchronous), the video leg above runs meanwhile
    if (na) {
        // STRSPU: one SPU chain per channel (5 filters, 4-bit), U = K B - d units each in a stream's K x 126 records of 16 bytes
        const bool spu = s->format == FORMAT_STRSPU;
        const int ch = s->audio_channels, bits = spu ? 4 : s->audio_bit_depth, filters = spu ? 5 : 4;
        const XaLayout xa = xa_layout(s->format == FORMAT_STRCD, ch == 2, bits);
        const int units_per_stream = na * (spu ? 126 : xa.units_per_sector);
        const int units_per_chain = units_per_stream / ch - (spu ? strspu_dummy_of((uint32_t)s->strspu_options) : 0);
        const int64_t need = pl.audio_samples;                                   // per channel, over the whole stream
        const int limit = (int)(pcm_samples_per_channel < need ? pcm_samples_per_channel : need);      // past it the encoder reads zeros (decoding.c:521-527)
        if (n_streams > 1 && pcm_stream_stride < (int64_t)limit * ch) {
            psxhip_set_error("psxhip_str_encode_device: pcm_stream_stride smaller than a stream's samples");
            return PSXHIP_EINVAL;
        }
        HIP_TRY(hipEventRecord(d.ev_in, S), PSXHIP_EDEVICE);
        HIP_TRY(hipStreamWaitEvent(d.astream, d.ev_in, 0), PSXHIP_EDEVICE);
        const int n_chains = n_streams * ch;
        const bool chunked = units_per_chain >= psxhip_adpcm_chunked_threshold(n_chains);      // (the rule of the host entry points)
        // an error from here on leaves nothing of this call in flight on the caller's buffers
        auto fail = [&](int code) { (void)hipStreamSynchronize(d.astream); (void)hipStreamSynchronize(S); return code; };
        if (d.d_pcm != d_pcm || d.pcm_stream_stride != pcm_stream_stride || d.chunked != chunked) {
            d.d_pcm = nullptr;          // (set again when the new session / tables stand: a failure below must not leave the old key on torn-down state)
            if (d.session) { psxhip_adpcm_session_destroy(d.session); d.session = nullptr; }
            std::vector<psxhip_adpcm_chain_t> chains((size_t)n_chains);
            std::vector<int32_t> base((size_t)n_chains);
            fill_interleaved_chains(chains.data(), base.data(), n_streams, ch, pcm_stream_stride, limit, units_per_stream);
            for (psxhip_adpcm_chain_t& chain : chains) chain.n_units = units_per_chain;
            if (chunked) {
                int chunk_units = 0, warmup_units = 0;
                psxhip_adpcm_pick_chunking((long long)units_per_chain * n_chains, 5, device, &chunk_units, &warmup_units);
                const int rc = psxhip_adpcm_session_create(&d.session, device, d_pcm, chains.data(), base.data(), nullptr, n_chains, filters, bits,
                                                           d.buf.units.as<uint8_t>(), chunk_units, warmup_units, d.astream);
                if (rc) return fail(rc);
            } else {
                d.tab = {};
                int rc;
                if ((rc = d.tab.chains.reserve(chains.size() * sizeof(chains[0]))) || (rc = d.tab.base.reserve(base.size() * 4)) ||
                    (rc = d.tab.states.reserve(chains.size() * sizeof(psxhip_adpcm_state_t))))
                    return fail(rc);
                if (hipMemcpy(d.tab.chains.p, chains.data(), chains.size() * sizeof(chains[0]), hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(d.tab.base.p, base.data(), base.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
                    psxhip_set_error("psxhip_str_encode_device: chain tables: %s", hipGetErrorString(hipGetLastError()));
                    return fail(PSXHIP_EDEVICE);
                }
            }
            d.d_pcm = d_pcm;
            d.pcm_stream_stride = pcm_stream_stride;
            d.chunked = chunked;
        }
        int rc;
        if (chunked) {
            std::vector<psxhip_adpcm_state_t> zero((size_t)n_chains);
            memset(zero.data(), 0, zero.size() * sizeof(zero[0]));
            psxhip_adpcm_session_reset(d.session);
            rc = psxhip_adpcm_session_run(d.session, zero.data(), nullptr, 0, nullptr, nullptr);
            if (rc < 0) return fail(rc);
        } else {
            HIP_TRY(hipMemsetAsync(d.tab.states.p, 0, (size_t)n_chains * sizeof(psxhip_adpcm_state_t), d.astream), PSXHIP_EDEVICE);
            rc = psxhip_adpcm_encode_chains_device(device, d_pcm, d.tab.chains.as<const psxhip_adpcm_chain_t>(), d.tab.base.as<const int32_t>(), n_chains, filters,
                                                   bits, d.tab.states.as<psxhip_adpcm_state_t>(), d.buf.units.as<uint8_t>(), d.astream);
            if (rc) return fail(rc);
        }
        if (spu)
            rc = psxhip_strspu_audio_sectors_device(device, d.buf.units.as<const uint8_t>(), na, ch, s->audio_frequency, (uint32_t)s->strspu_options, n_streams,
                                                    (size_t)units_per_stream * xa.record_bytes, d_out, d.buf.adst.as<const int32_t>(), out_stream_stride, d.astream);
        else
            rc = psxhip_xa_assemble_scatter(device, d.buf.units.as<const uint8_t>(), na, s->format == FORMAT_STRCD ? 1 : 0, ch == 2, s->audio_frequency, bits,
                                            s->audio_xa_file, s->audio_xa_channel, 0, d.buf.eof.as<const uint8_t>(), 0u, d_out, d.buf.adst.as<const int32_t>(),
                                            n_streams, (size_t)units_per_stream * xa.record_bytes, out_stream_stride, d.astream);
        if (rc) return fail(rc);
        HIP_TRY(hipEventRecord(d.ev_audio, d.astream), PSXHIP_EDEVICE);
        HIP_TRY(hipStreamWaitEvent(S, d.ev_audio, 0), PSXHIP_EDEVICE);
    }
    HIP_TRY(hipStreamSynchronize(S), PSXHIP_EDEVICE);
    if (nf) {
        // frames the split kernel's watchdog released (another process held the CUs): encoded again through the frame kernel, and
        // the video sectors built again over them
        std::vector<psxhip_mdec_batch_t> again;
        for (size_t i = 0; i < (size_t)nf * n_streams; i++)
            if (d.h_res[i].quant_scale == PSXHIP_MDEC_QS_RELEASED) {
                psxhip_mdec_batch_t b;
                b.d_frames = d_frames + (i / (size_t)nf) * frames_stream_stride + (i % (size_t)nf) * fsz;
                b.n_frames = 1;
                b.reserved = 0;
                b.d_frame_max_sizes = d.buf.budgets.as<const int32_t>() + i;
                b.d_out = d.buf.bs.as<uint8_t>() + i * ostride;
                b.d_results = d.buf.res.as<psxhip_mdec_result_t>() + i;
                again.push_back(b);
            }
        if (!again.empty()) {
            int rc = psxhip_mdec_encode_batches_frame_kernel(d.mdec, again.data(), (int)again.size(), fsz, 0, ostride, S);
            if (rc) return rc;
            rc = video_sectors();
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(d.h_res, d.buf.res.p, sizeof(psxhip_mdec_result_t) * (size_t)nf * n_streams, hipMemcpyDeviceToHost, S), PSXHIP_EDEVICE);
            HIP_TRY(hipStreamSynchronize(S), PSXHIP_EDEVICE);
        }
    }
    long long qsum = 0;
    for (size_t i = 0; i < (size_t)nf * n_streams; i++) {
        if (d.h_res[i].quant_scale >= 64) {
            psxhip_set_error("psxhip_str_encode_device: frame %zu of stream %zu does not fit its budget at any quant scale", i % (size_t)nf, i / (size_t)nf);
            return PSXHIP_ENOFIT;
        }
        qsum += d.h_res[i].quant_scale;
    }
    if (plan_out) plan_out->quant_scale_sum = qsum;
    return PSXHIP_OK;
}


// ---------------------------------------------------------------------------------------------------------------------------
// The STRSPU audio sector builder on its own: unit records in HBM -> audio sectors in their slots (strspu_kernels.hip)
extern "C" int psxhip_strspu_audio_sectors_device(int device, const uint8_t* d_units, int n_sectors, int channels, int frequency, uint32_t options,
                                                  int n_streams, size_t units_stream_stride, uint8_t* d_out, const int32_t* d_dst_sector,
                                                  size_t out_stream_stride, void* stream) {
    if (!d_units || !d_out || n_sectors < 0 || n_sectors > 0x7FFFFFFF / 126 || n_streams < 1 || n_streams > 65535 || (channels != 1 && channels != 2) ||
        frequency <= 0 || (options & ~kStrspuOptionBits) || ((uintptr_t)d_units & 15) || (units_stream_stride & 15) || ((uintptr_t)d_out & 3) ||
        (out_stream_stride & 3) || ((uintptr_t)d_dst_sector & 3)) {
        psxhip_set_error("psxhip_strspu_audio_sectors_device: bad argument (d_units and its stride 16-byte aligned, d_out and its stride 4-byte aligned, "
                         "1 or 2 channels, no unknown option bit)");
        return PSXHIP_EINVAL;
    }
    if (n_streams > 1 && (units_stream_stride < (size_t)n_sectors * 126 * PSXHIP_ADPCM_RECORD_BYTES_4BIT || (!d_dst_sector && out_stream_stride < (size_t)n_sectors * 2048))) {
        psxhip_set_error("psxhip_strspu_audio_sectors_device: a stream stride smaller than a stream");
        return PSXHIP_EINVAL;
    }
    const int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    if (n_sectors == 0) return PSXHIP_OK;
    psxhip_strspu_job_t job;
    memset(&job, 0, sizeof job);
    job.units = d_units;
    job.n_sectors = n_sectors;
    job.channels = channels;
    job.frequency = frequency;
    job.options = options;
    job.out = d_out;
    job.dst_sector = d_dst_sector;
    job.units_stream_stride = units_stream_stride;
    job.out_stream_stride = out_stream_stride;
    HIP_TRY(psxhip_strspu_audio_sectors_launch(&job, n_streams, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" const char* psxhip_strspu_kernel_rev(void) { return PSXHIP_STRSPU_KERNEL_REV; }
