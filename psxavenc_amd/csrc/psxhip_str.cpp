// psxhip_str.cpp -- batched STR / STRCD / STRV muxer (include/psxav_hip.h, psxhip_str_*).
//
// What psxavenc's encode_file_str does sector by sector (psxavenc/filefmt.c:391-520 with :73-91, around
// encode_sector_str, mdec.c:757-836, and psx_audio_xa_encode, adpcm.c:293-332), restated for inputs that are all
// there up front: the sector loop is first run dry (make_plan, str_plan.cpp: which frame slice / audio sector lands where,
// which frames are part of the stream at all, which audio sectors carry EOF -- incl. the reference's end-of-input model);
// the per-frame byte budgets are a closed-form function of the frame index (mdec.c:768-775), so every frame is encoded
// in ONE batched MDEC call sharded over the handle's devices; the audio is one XA stream encoded by the ADPCM kernels
// concurrently (its own host thread and stream); the host then cuts the finished frames into sectors and interleaves
// them with the finished audio sectors.  No encoding happens on the host.  No process-global state: everything kept
// between calls lives in a psxhip_str_ctx_t.
//
// Format 8 (STRSPU, "psxhip STRSPU v1") is the same muxer with another audio leg: the sector schedule is a
// rational share p / q of audio sectors (host_layout.h: strspu_layout), the audio is one SPU-ADPCM chain per channel (5 filters,
// 4-bit), and an audio sector is a chunk header and 126 SPU blocks placed as the SPUI writer places them (filefmt.c:323-371) --
// on the device by strspu_kernels.hip, on the host by strspu_place_host (str_plan.cpp).
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
#include "adpcm_plan.h"
#include "device_buffer.h"
#include "psxhip_adpcm_internal.h"
#include "psxhip_internal.h"
#include "str_plan.h"

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
        // what the plan and the settings give, derived once when the shape is built
        int n_vtab = 0, na = 0, nf = 0;     // entries of the video table; audio sectors that hold samples, frames -- per stream
        size_t fsz = 0, ostride = 0;        // bytes of a frame; between the frames' bitstreams in buf.bs
        int bits = 0, filters = 0;          // of the ADPCM chains (XA: 4 filters; STRSPU: 5 filters, 4-bit)
        int units_per_stream = 0;           // unit records a stream's audio sectors hold (STRSPU: 126 blocks per sector)
        int units_per_chain = 0;            // units a channel's chain encodes (STRSPU: less the leading dummy block)
        size_t units_stream_bytes = 0;      // between the streams' records in buf.units
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
typedef psxhip_str_ctx::Dev Dev;

// The cached shape goes: its session, tables and buffers (the caller has waited for what ran on them).  The encoder context, the
// audio stream and the events outlive a shape.
void drop_shape(Dev& d) {
    if (d.session) psxhip_adpcm_session_destroy(d.session);
    d.session = nullptr;
    d.buf = {};
    d.tab = {};
    if (d.h_res) (void)hipHostFree(d.h_res);
    d.h_res = nullptr;
    d.n_frames = -1;
    d.n_streams = 0;            // (no call's shape equals a dropped one)
}

void free_dev(psxhip_str_ctx* c) {
    Dev& d = c->dev;
    (void)hipSetDevice(c->devices[0]);
    if (d.astream) (void)hipStreamSynchronize(d.astream);
    drop_shape(d);
    if (d.mdec) psxhip_mdec_destroy(d.mdec);
    if (d.ev_in) (void)hipEventDestroy(d.ev_in);
    if (d.ev_audio) (void)hipEventDestroy(d.ev_audio);
    if (d.astream) (void)hipStreamDestroy(d.astream);
    d.ev_in = nullptr; d.ev_audio = nullptr; d.astream = nullptr; d.mdec = nullptr;
}

// Whether the MDEC context kept under `kept` (have: there is one) is the one this stream needs; `key` is what the caller keeps once
// the new context stands
bool same_mdec(bool have, const int kept[4], const psxhip_str_settings_t* s, const Plan& pl, int key[4]) {
    key[0] = s->video_codec; key[1] = s->video_width; key[2] = s->video_height; key[3] = pl.pub.max_frame_size;
    return have && memcmp(key, kept, 4 * sizeof(int)) == 0;
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
    if (sectors && cap > 0) memcpy(sectors, pl.sectors.data(), (size_t)(n < cap ? n : cap) * sizeof *sectors);
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
            const psxhip_str_sector_t& sc = pl.sectors[(size_t)n];
            if ((sc.kind == PSXHIP_STR_SECTOR_VIDEO) != video) continue;
            if (video) {
                const int frame = sc.frame;
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
                str_video_chunk_header(hd, s, frame, sc.index, pl.budgets[(size_t)frame], (uint32_t)res[(size_t)frame].bytes_used, fo);
                memcpy(hd + 0x20, fo + (size_t)sc.index * 2016, 2016);
                psx_cdrom_calculate_checksums((psx_cdrom_sector_t*)sector, PSX_CDROM_SECTOR_TYPE_MODE2_FORM1);
                memcpy(dst, sector, ssz);
            } else if (sc.kind == PSXHIP_STR_SECTOR_EMPTY) {
                // no samples left: psx_audio_xa_encode writes nothing (adpcm.c:310) and the reference puts out whatever its
                // stack buffer held; zero here
                memset(dst, 0, ssz);
            } else {
                memcpy(dst, xa_out.data() + (size_t)sc.index * ssz, ssz);
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
        int key[4];
        if (!same_mdec(c->mdec != nullptr, c->key, s, pl, key)) {
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
    const int ch = s->audio_channels, na = pl.n_audio;
    int rc_audio = PSXHIP_OK;
    if (na > 0 && s->format == FORMAT_STRSPU) {
        // STRSPU: every channel is one SPU chain over its samples fitted to 28 U (cut, or completed with silence), all channels in one
        // batched call; the host only places the blocks
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
            strspu_place_host(pl.rates.spu_layout, s->audio_frequency, (uint32_t)s->strspu_options, na, blocks.data(), xa_out.data());
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
        for (const psxhip_str_sector_t& sc : pl.sectors)
            if (sc.kind == PSXHIP_STR_SECTOR_AUDIO) eof[(size_t)sc.index] = (uint8_t)sc.eof;
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
namespace {

// what the caller of psxhip_str_encode_device hands over (the settings are the cached shape's once that stands)
struct DevCall {
    int device, n_streams, n_frames;
    const uint8_t* d_frames;
    size_t frames_stream_stride;
    const int16_t* d_pcm;
    int64_t pcm_stream_stride, pcm_samples;
    uint8_t* d_out;
    size_t out_stream_stride;
    hipStream_t S;
};

// The plan and its device tables, the buffers and what the audio leg needs to know: rebuilt when the shape of the job changes.
// A job no plan can be made for leaves the cached shape as it was.
int rebuild_shape(Dev& d, const DevCall& a, const psxhip_str_settings_t* s, psxhip_str_plan_t* plan_out) {
    Plan pl;
    int rc = make_plan(s, a.n_frames, a.pcm_samples, &pl);
    if (rc) return rc;
    if (plan_out) *plan_out = pl.pub;
    // nothing of the old shape may still be running on the buffers that are about to go
    HIP_TRY(hipStreamSynchronize(a.S), PSXHIP_EDEVICE);
    if (d.astream) HIP_TRY(hipStreamSynchronize(d.astream), PSXHIP_EDEVICE);
    drop_shape(d);
    d.settings = *s;
    const int nf = pl.pub.n_frames_encoded, n_streams = a.n_streams;
    std::vector<int32_t> vtab, adst;
    std::vector<uint8_t> eof;
    for (int n = 0; n < pl.pub.n_sectors; n++) {
        const psxhip_str_sector_t& sc = pl.sectors[(size_t)n];
        if (sc.kind == PSXHIP_STR_SECTOR_AUDIO) {
            adst.push_back(n);
            eof.push_back((uint8_t)sc.eof);
        } else {            // {sector, frame, byte offset, budget}; frame -2: an audio slot with no samples left, a zero sector
            const bool video = sc.kind == PSXHIP_STR_SECTOR_VIDEO;
            for (int32_t v : {n, video ? sc.frame : -2, video ? sc.index * 2016 : 0, video ? pl.budgets[(size_t)sc.frame] : 0}) vtab.push_back(v);
        }
    }
    d.n_vtab = (int)(vtab.size() / 4);
    d.na = pl.n_audio;
    d.nf = nf;
    d.fsz = (size_t)s->video_width * s->video_height * 3 / 2;
    d.ostride = ((size_t)pl.pub.max_frame_size + 3) & ~(size_t)3;
    // STRSPU: one SPU chain per channel (5 filters, 4-bit), U = K B - d units each in a stream's K x 126 records of 16 bytes
    const bool spu = pl.rates.spu;
    d.bits = spu ? 4 : s->audio_bit_depth;
    d.filters = spu ? 5 : 4;
    const XaLayout xa = xa_layout(s->format == FORMAT_STRCD, s->audio_channels == 2, d.bits);
    d.units_per_stream = d.na * (spu ? 126 : xa.units_per_sector);
    d.units_per_chain = d.na ? d.units_per_stream / s->audio_channels - (spu ? strspu_dummy_of((uint32_t)s->strspu_options) : 0) : 0;
    d.units_stream_bytes = (size_t)d.units_per_stream * xa.record_bytes;
    std::vector<int32_t> budgets((size_t)nf * n_streams);
    for (int i = 0; i < n_streams; i++)
        for (int f = 0; f < nf; f++) budgets[(size_t)i * nf + f] = pl.budgets[(size_t)f];
    auto up = [](DeviceBuffer& dst, const void* src, size_t bytes) -> int {
        const int rc = dst.reserve(bytes ? bytes : 4);
        if (rc) return rc;
        if (bytes) HIP_TRY(hipMemcpy(dst.p, src, bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
        return PSXHIP_OK;
    };
    const size_t bs_bytes = d.ostride * (size_t)nf * n_streams + 16;          // (never an empty allocation: a stream may hold no frame at all)
    const size_t res_bytes = sizeof(psxhip_mdec_result_t) * (size_t)(nf ? nf : 1) * n_streams;
    if ((rc = up(d.buf.vtab, vtab.data(), vtab.size() * 4)) || (rc = up(d.buf.budgets, budgets.data(), budgets.size() * 4)) ||
        (rc = up(d.buf.adst, adst.data(), adst.size() * 4)) || (rc = up(d.buf.eof, eof.data(), eof.size())) || (rc = d.buf.bs.reserve(bs_bytes)))
        return rc;
    HIP_TRY(hipMemset(d.buf.bs.p, 0, bs_bytes), PSXHIP_EDEVICE);      // (rows wider than a frame's own budget read as zero there)
    if ((rc = d.buf.res.reserve(res_bytes))) return rc;
    HIP_TRY(hipHostMalloc((void**)&d.h_res, res_bytes, hipHostMallocDefault), PSXHIP_ENOMEM);
    // (the records of either kind fit the larger record size)
    if ((rc = d.buf.units.reserve((size_t)(d.units_per_stream ? d.units_per_stream : 1) * PSXHIP_ADPCM_RECORD_BYTES * n_streams))) return rc;
    if (!d.astream) HIP_TRY(hipStreamCreateWithFlags(&d.astream, hipStreamNonBlocking), PSXHIP_EDEVICE);
    if (!d.ev_in) HIP_TRY(hipEventCreateWithFlags(&d.ev_in, hipEventDisableTiming), PSXHIP_EDEVICE);
    if (!d.ev_audio) HIP_TRY(hipEventCreateWithFlags(&d.ev_audio, hipEventDisableTiming), PSXHIP_EDEVICE);
    d.plan = std::move(pl);
    d.n_frames = a.n_frames;
    d.pcm_samples = a.pcm_samples;
    d.n_streams = n_streams;
    d.d_pcm = nullptr;           // (the ADPCM session is built by the audio leg, over this call's PCM)
    return PSXHIP_OK;
}

// what comes from outside the library, against the shape
int check_call(const Dev& d, const DevCall& a) {
    const size_t ssz = (size_t)d.plan.pub.sector_size, ns = (size_t)d.plan.pub.n_sectors;
    if ((d.nf && !a.d_frames) || !a.d_out || (d.na && !a.d_pcm) || a.out_stream_stride < ssz * ns || (a.out_stream_stride & 3) || ((uintptr_t)a.d_out & 3) ||
        (d.nf && ((a.frames_stream_stride < d.fsz * (size_t)a.n_frames && a.n_streams > 1) || (a.frames_stream_stride & 3) || ((uintptr_t)a.d_frames & 3)))) {
        psxhip_set_error("psxhip_str_encode_device: NULL / misaligned argument, or a stream stride smaller than a stream");
        return PSXHIP_EINVAL;
    }
    return PSXHIP_OK;
}

// frames first .. first + n - 1 of the call, counted through the streams: the caller's pictures, and this handle's budgets,
// bitstream rows and result records
psxhip_mdec_batch_t frames_batch(const Dev& d, const DevCall& a, size_t first, int n) {
    psxhip_mdec_batch_t b;
    b.d_frames = a.d_frames + first / (size_t)d.nf * a.frames_stream_stride + first % (size_t)d.nf * d.fsz;
    b.n_frames = n;
    b.reserved = 0;
    b.d_frame_max_sizes = d.buf.budgets.as<const int32_t>() + first;
    b.d_out = d.buf.bs.as<uint8_t>() + first * d.ostride;
    b.d_results = d.buf.res.as<psxhip_mdec_result_t>() + first;
    return b;
}

// The sector kernel over the bitstreams and results as they stand, then the results to the host: on the caller's stream.
// (No frame in the stream, but audio slots without samples: zero sectors -- nothing reads a bitstream.)
int video_sectors_and_results(Dev& d, const DevCall& a) {
    if (d.n_vtab) {
        const psxhip_str_settings_t& s = d.settings;
        psxhip_str_video_job_t vj;
        memset(&vj, 0, sizeof vj);
        vj.bs = d.buf.bs.as<const uint8_t>();
        vj.bs_stride = d.ostride;
        vj.bs_stream_stride = d.ostride * (size_t)d.nf;
        vj.res = d.buf.res.as<const psxhip_mdec_result_t>();
        vj.frames_per_stream = d.nf;
        vj.tab = d.buf.vtab.as<const int4>();
        vj.n_entries = d.n_vtab;
        vj.format = s.format;
        vj.sector_size = d.plan.pub.sector_size;
        vj.xa_file = s.audio_xa_file;
        vj.xa_channel = s.audio_xa_channel;
        vj.video_id = s.str_video_id;
        vj.width = s.video_width;
        vj.height = s.video_height;
        vj.out = a.d_out;
        vj.out_stream_stride = a.out_stream_stride;
        const int rc = psxhip_sector_tables(a.device);
        if (rc) return rc;
        HIP_TRY(psxhip_str_video_sectors_launch(&vj, a.n_streams, a.S), PSXHIP_EDEVICE);
    }
    if (d.nf) HIP_TRY(hipMemcpyAsync(d.h_res, d.buf.res.p, sizeof(psxhip_mdec_result_t) * (size_t)d.nf * a.n_streams, hipMemcpyDeviceToHost, a.S), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

// video: one batched launch over the frames of all streams, then the sector kernel, both on the caller's stream
int video_leg(Dev& d, const DevCall& a) {
    if (d.nf) {
        const psxhip_str_settings_t& s = d.settings;
        int key[4];
        if (!same_mdec(d.mdec != nullptr, d.mdec_key, &s, d.plan, key)) {
            if (d.mdec) { psxhip_mdec_destroy(d.mdec); d.mdec = nullptr; }
            const int rc = psxhip_mdec_create(&d.mdec, a.device, s.video_codec, s.video_width, s.video_height, d.plan.pub.max_frame_size);
            if (rc) return rc;
            memcpy(d.mdec_key, key, sizeof key);
        }
        std::vector<psxhip_mdec_batch_t> batches;
        if (a.n_streams == 1 || (a.frames_stream_stride == d.fsz * (size_t)d.nf && d.nf == a.n_frames))
            batches.push_back(frames_batch(d, a, 0, d.nf * a.n_streams));          // the streams' frames lie back to back
        else
            for (int i = 0; i < a.n_streams; i++) batches.push_back(frames_batch(d, a, (size_t)i * d.nf, d.nf));
        const int rc = psxhip_mdec_encode_batches_device(d.mdec, batches.data(), (int)batches.size(), d.fsz, 0, d.ostride, a.S);
        if (rc) return rc;
    }
    return video_sectors_and_results(d, a);
}

// audio: the streams' tracks as chains of one session on the handle's own stream, behind the caller's inputs; the host drives the
// verify passes (the call is synchronous), the video leg runs meanwhile.  The caller's stream waits for the audio sectors.
int audio_leg(Dev& d, const DevCall& a) {
    const psxhip_str_settings_t& s = d.settings;
    const int ch = s.audio_channels, n_chains = a.n_streams * ch;
    const int64_t need = d.plan.audio_samples;                               // per channel, over the whole stream
    const int limit = (int)(a.pcm_samples < need ? a.pcm_samples : need);      // past it the encoder reads zeros (decoding.c:521-527)
    if (a.n_streams > 1 && a.pcm_stream_stride < (int64_t)limit * ch) {
        psxhip_set_error("psxhip_str_encode_device: pcm_stream_stride smaller than a stream's samples");
        return PSXHIP_EINVAL;
    }
    HIP_TRY(hipEventRecord(d.ev_in, a.S), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamWaitEvent(d.astream, d.ev_in, 0), PSXHIP_EDEVICE);
    const bool chunked = adpcm_route_chunked(d.units_per_chain, n_chains);      // (the rule of the host entry points)
    // an error from here on leaves nothing of this call in flight on the caller's buffers
    auto fail = [&](int code) { (void)hipStreamSynchronize(d.astream); (void)hipStreamSynchronize(a.S); return code; };
    if (d.d_pcm != a.d_pcm || d.pcm_stream_stride != a.pcm_stream_stride || d.chunked != chunked) {
        d.d_pcm = nullptr;          // (set again when the new session / tables stand: a failure below must not leave the old key on torn-down state)
        if (d.session) { psxhip_adpcm_session_destroy(d.session); d.session = nullptr; }
        std::vector<psxhip_adpcm_chain_t> chains((size_t)n_chains);
        std::vector<int32_t> base((size_t)n_chains);
        fill_interleaved_chains(chains.data(), base.data(), a.n_streams, ch, a.pcm_stream_stride, limit, d.units_per_stream);
        for (psxhip_adpcm_chain_t& chain : chains) chain.n_units = d.units_per_chain;
        if (chunked) {
            int chunk_units = 0, warmup_units = 0;
            psxhip_adpcm_pick_chunking((long long)d.units_per_chain * n_chains, 5, a.device, &chunk_units, &warmup_units);
            const int rc = psxhip_adpcm_session_create(&d.session, a.device, a.d_pcm, chains.data(), base.data(), nullptr, n_chains, d.filters, d.bits,
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
        d.d_pcm = a.d_pcm;
        d.pcm_stream_stride = a.pcm_stream_stride;
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
        rc = psxhip_adpcm_encode_chains_device(a.device, a.d_pcm, d.tab.chains.as<const psxhip_adpcm_chain_t>(), d.tab.base.as<const int32_t>(), n_chains, d.filters,
                                               d.bits, d.tab.states.as<psxhip_adpcm_state_t>(), d.buf.units.as<uint8_t>(), d.astream);
        if (rc) return fail(rc);
    }
    if (d.plan.rates.spu)
        rc = psxhip_strspu_audio_sectors_device(a.device, d.buf.units.as<const uint8_t>(), d.na, ch, s.audio_frequency, (uint32_t)s.strspu_options, a.n_streams,
                                                d.units_stream_bytes, a.d_out, d.buf.adst.as<const int32_t>(), a.out_stream_stride, d.astream);
    else
        rc = psxhip_xa_assemble_scatter(a.device, d.buf.units.as<const uint8_t>(), d.na, s.format == FORMAT_STRCD ? 1 : 0, ch == 2, s.audio_frequency, d.bits,
                                        s.audio_xa_file, s.audio_xa_channel, 0, d.buf.eof.as<const uint8_t>(), 0u, a.d_out, d.buf.adst.as<const int32_t>(),
                                        a.n_streams, d.units_stream_bytes, a.out_stream_stride, d.astream);
    if (rc) return fail(rc);
    HIP_TRY(hipEventRecord(d.ev_audio, d.astream), PSXHIP_EDEVICE);
    HIP_TRY(hipStreamWaitEvent(a.S, d.ev_audio, 0), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

// Frames the split kernel's watchdog released (another process held the CUs) are encoded again through the frame kernel, and the
// video sectors built again over them.  The results are on the host when this is called, and again when it returns.
int reencode_released(Dev& d, const DevCall& a) {
    std::vector<psxhip_mdec_batch_t> again;
    for (size_t i = 0; i < (size_t)d.nf * a.n_streams; i++)
        if (d.h_res[i].quant_scale == PSXHIP_MDEC_QS_RELEASED) again.push_back(frames_batch(d, a, i, 1));
    if (again.empty()) return PSXHIP_OK;
    int rc = psxhip_mdec_encode_batches_frame_kernel(d.mdec, again.data(), (int)again.size(), d.fsz, 0, d.ostride, a.S);
    if (rc) return rc;
    if ((rc = video_sectors_and_results(d, a))) return rc;
    HIP_TRY(hipStreamSynchronize(a.S), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

}  // namespace

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
    Dev& d = c->dev;
    const DevCall a = {c->devices[0], n_streams, n_frames, d_frames, frames_stream_stride, d_pcm, pcm_stream_stride, pcm_samples_per_channel,
                       d_out, out_stream_stride, (hipStream_t)stream};
    HIP_TRY(hipSetDevice(a.device), PSXHIP_EDEVICE);
    int rc;
    const bool same = d.n_frames == n_frames && d.pcm_samples == pcm_samples_per_channel && d.n_streams == n_streams && s &&
                      memcmp(&d.settings, s, sizeof *s) == 0;
    if (!same && (rc = rebuild_shape(d, a, s, plan_out))) return rc;
    if (plan_out) *plan_out = d.plan.pub;
    if (d.plan.pub.n_sectors == 0) return PSXHIP_OK;
    if ((rc = check_call(d, a)) || (rc = video_leg(d, a)) || (d.na && (rc = audio_leg(d, a)))) return rc;
    HIP_TRY(hipStreamSynchronize(a.S), PSXHIP_EDEVICE);
    if ((rc = reencode_released(d, a))) return rc;
    long long qsum = 0;
    for (size_t i = 0; i < (size_t)d.nf * n_streams; i++) {
        if (d.h_res[i].quant_scale >= 64) {
            psxhip_set_error("psxhip_str_encode_device: frame %zu of stream %zu does not fit its budget at any quant scale", i % (size_t)d.nf, i / (size_t)d.nf);
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
