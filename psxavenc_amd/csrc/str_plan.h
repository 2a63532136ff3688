// str_plan.h -- what the STR muxer (psxhip_str.cpp) and the reader (psxhip_str_demux.cpp) derive from settings and lengths alone: the
// rates of a stream, the sector plan, and the two 32-byte chunk headers and the STRSPU block placement the host writes.  Arithmetic
// and bytes only (no HIP), like host_layout.h: str_plan.cpp builds with a host compiler alone and links against nothing but
// psxhip_set_error (tests/test_str_plan_cpu.py does so, under the host sanitizers).  Nothing here is part of the library's surface.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/psxav_hip.h"
#include "../../include/psxav_mdec.h"
#include "host_layout.h"

extern "C" void psxhip_set_error(const char* fmt, ...);          // (psxhip_api.cpp; psxhip_internal.h declares it beside HIP)

#pragma GCC visibility push(hidden)

constexpr uint32_t kStrspuOptionBits = PSXHIP_STRSPU_ID_MASK | PSXHIP_STRSPU_LOOP | PSXHIP_STRSPU_NO_LEADING_DUMMY;
static inline int strspu_dummy_of(uint32_t options) { return (options & PSXHIP_STRSPU_NO_LEADING_DUMMY) ? 0 : 1; }      // d: blocks the leading dummy takes

// What a stream's rates give (filefmt.c:399-403,428-432; format 8: DESIGN.md section 15)
struct StrRates {
    int64_t base, den;          // frame_block_base_overflow / frame_block_overflow_den: a frame gets base / den sectors (mdec.c:768-775)
    int interleave;             // sectors per block of 1 audio + vpb video; 1 without audio; STRSPU: q / p when that is whole, else 0
    int vpb;                    // video sectors per block (STRSPU, or no audio: 1)
    int samples_per_sector;     // per channel; 0 without audio
    int sector_size;
    bool spu;                   // format 8 with audio: the schedule is spu_layout's p / q (format 8 without audio is STRV in 2048-byte sectors)
    StrspuLayout spu_layout;
};

// of settings whose format, CD speed, frame rate and audio settings are already checked (settings_error, or the reader's own checks)
StrRates str_rates(const psxhip_str_settings_t* s);

struct Plan {
    psxhip_str_plan_t pub = {};                 // (all zero until make_plan has accepted the settings)
    StrRates rates = {};
    std::vector<int32_t> budgets;               // frame_max_size of every frame in the stream, mdec.c:768-775
    std::vector<psxhip_str_sector_t> sectors;   // the rows psxhip_str_plan_sectors hands out; a video sector's slice starts at byte index * 2016
    int n_audio = 0;                            // audio sectors that hold samples (pub.n_audio_sectors counts the empty slots too)
    int64_t audio_samples = 0;                  // per channel, handed to the audio encoder over the whole stream
};

// nullptr, or what is wrong with the settings
const char* settings_error(const psxhip_str_settings_t* s);
// The sector loop of encode_file_str run dry.  PSXHIP_OK, or PSXHIP_EINVAL with the error text set.
int make_plan(const psxhip_str_settings_t* s, int n_frames, int64_t pcm_samples_per_channel, Plan* pl);

// The 32-byte chunk header of chunk `chunk` of frame `frame` (from 0), encode_sector_str, mdec.c:782-820: `budget` is the frame's
// frame_max_size, frame_bs its bitstream (the first 8 bytes are quoted)
void str_video_chunk_header(uint8_t* hd, const psxhip_str_settings_t* s, int frame, int chunk, int budget, uint32_t bytes_used, const uint8_t* frame_bs);
// The 32-byte chunk header of STRSPU audio sector k of K
void strspu_chunk_header(uint8_t* hd, const StrspuLayout& x, int frequency, uint32_t options, int k, int K);
// The host path's block placement: K audio sectors from every channel's U = K B - d encoded blocks (blocks: channel c's at
// c * U * 16), as strspu_audio_sector_kernel builds them on the device
void strspu_place_host(const StrspuLayout& x, int frequency, uint32_t options, int K, const uint8_t* blocks, uint8_t* out);

#pragma GCC visibility pop
