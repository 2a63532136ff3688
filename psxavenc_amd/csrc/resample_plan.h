// resample_plan.h -- what the audio front-end's host layer (psxhip_resample.cpp) derives from a call's arguments alone: the filter
// design in double, how many outputs a stream position yields, the default mix matrices, what create and the two convert entries
// refuse (with which text, in which order), the launch's shape on a device (span, table in LDS or not, LDS bytes by afe_layout.h,
// persistent grid) and the cut of a call into launches.  Arithmetic and refusals only (no HIP), like adpcm_plan.h and mdec_plan.h:
// resample_plan.cpp builds with a host compiler alone and links against nothing but psxhip_set_error
// (tests/test_resample_plan_cpu.py does so, under the host sanitizers); the launch file only executes these plans.  The two entry
// points of the C ABI that need no device (psxhip_resampler_design, psxhip_resampler_output_count) are defined in resample_plan.cpp
// as they stand in include/psxav_hip.h; nothing else here is part of the library's surface.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/psxav_hip.h"
#include "afe_layout.h"

extern "C" void psxhip_set_error(const char* fmt, ...);          // (psxhip_api.cpp; psxhip_internal.h declares it beside HIP)

#pragma GCC visibility push(hidden)

// ---------------------------------------------------------------------------------------------- the design
constexpr int kFilterSize = 32;         // libswresample's defaults: filter_size, phase_shift (1 << 10 phases), cutoff, Kaiser beta
constexpr int kMaxPhases = 1 << 10;
constexpr double kCutoff = 0.97;
constexpr double kBeta = 9.0;
constexpr int64_t kLaunchMaxIn = 1 << 28;   // new samples per launch (longer calls are cut; the history carries across)

struct Design {
    int L, M, P, T, H;
    bool bypass;
    double factor;
};
// false: a rate outside 1 000 .. 384 000 Hz, or a ratio above 16x
bool design_params(int src, int dst, Design* d);
// the Q15 table, [P][T]; false when some half of some phase has sum |h| > 65535
bool design_table(const Design& d, std::vector<int16_t>* out);

// outputs per channel that exist after n samples without flush, and in all after a flush
int64_t avail(const Design& d, int64_t n);
int64_t total(const Design& d, int64_t n);
// ... and what a call of n_in samples adds to a stream that has consumed `consumed`
inline int64_t outputs_of(const Design& d, int64_t consumed, int64_t n_in, int flush) {
    return (flush ? total(d, consumed + n_in) : avail(d, consumed + n_in)) - avail(d, consumed);
}

// ---------------------------------------------------------------------------------------------- the handle's plan
struct ResamplerPlan {
    int fmt, sch, dch;
    Design d;
    int16_t mix[8][8];                  // [dst][src] Q14: the caller's, or the default of the channel pair
    std::vector<int16_t> table;         // empty when the rates are equal
};
// psxhip_resampler_create behind its handle pointer, in front of the device: formats, channels, rates; the matrix and its row sums;
// the table
int resampler_create_plan(int src_format, int src_channels, int src_rate, int dst_channels, int dst_rate, const int16_t* mix, ResamplerPlan* out);

inline int resampler_nsrc(int fmt, int sch) { return (fmt & 1) ? sch : 1; }                          // source pointers: planes, or one buffer
inline size_t resampler_frame_bytes(int fmt, int sch) { return (size_t)(fmt <= PSXHIP_PCM_S16P ? 2 : 4) * ((fmt & 1) ? 1 : sch); }   // per pointer

// The launch's shape on a device of lds_per_cu bytes of LDS and n_cu compute units.  span: the input span of a tile, the last
// output's offset from the first (at most (L - 1 + 255 M) / L samples) plus T, even.  coef_lds: the table sits in LDS when it is at
// most 48 KiB and the launch's LDS (afe_lds_bytes) then still fits.  grid_max: a persistent grid, as many 256-lane groups as the LDS
// lets a compute unit hold, at most 8 (32 wavefronts).  Equal rates: no span, no LDS beyond the header (lds_bytes 0: nothing to
// prepare), 8 groups per CU.  Refuses a span that does not fit a compute unit.
struct ResamplerShape {
    int span = 0, coef_lds = 0, grid_max = 1;
    size_t lds_bytes = 0;
};
int resampler_shape(const Design& d, int dch, size_t lds_per_cu, int n_cu, ResamplerShape* out);

// psxhip_resampler_convert_device (host false) and _host in front of their HIP calls, the two orders as they are: p the handle's plan
// or NULL; dst_cap the host entry's.  *count: the call's outputs; *go false: nothing to launch (the device entry, no samples and no flush).
// The host entry's refusals of NULL arguments leave the error text as it was.
int resampler_convert_check(bool host, const ResamplerPlan* p, bool flushed, int64_t consumed, const void* const* src, int64_t n_in, bool dst,
                            int64_t dst_cap, int flush, int64_t* count, bool* go);

// The next launch of a call that still has `left` samples to give (flush: the call's): at most kLaunchMaxIn of them, and only the
// call's last launch flushes.  i0, r0: where output 0 sits in the input, (avail(consumed) * M) divmod L, relative to the launch's first
// new sample.  work: tiles of PSXHIP_AFE_TILE outputs, + the history tile; grid 0: nothing to launch (equal rates, no outputs).
struct ResamplerLaunch {
    int64_t n;
    bool flush;
    int64_t i0;
    int r0;
    int64_t n_out, work;
    int grid;
};
ResamplerLaunch resampler_launch(const Design& d, int64_t consumed, int64_t left, int flush, int grid_max);

#pragma GCC visibility pop
