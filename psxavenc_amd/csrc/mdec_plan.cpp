// mdec_plan.cpp -- see mdec_plan.h: every decision of the MDEC encoder's host layer, stated once.
#include "mdec_plan.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mdec_layout.h"

extern "C" size_t psxhip_mdec_lds_bytes(int nmb, int out_words, int stg_words, int large) {
    return lds_bytes(nmb, out_words, stg_words, large ? kWavesLarge : kWavesSmall);
}
extern "C" int psxhip_mdec_threads_per_group(int large) { return (large ? kWavesLarge : kWavesSmall) * 64; }

bool mdec_args_ok(int codec, int width, int height, int max_frame_size) {
    return !(codec < 0 || codec > 2 || width <= 0 || height <= 0 || (width % 16) || (height % 16) || width > 1024 ||
             height > 1024 || max_frame_size < 8);
}

int mdec_geometry(int width, int height, int max_frame_size, size_t lds_cu, int* large, int* out_words, int* stg_words,
                  size_t* lds_bytes) {
    const int nmb = (width / 16) * (height / 16);
    const int image = (max_frame_size + 3) / 4;     // dwords of the frame image
    const int sw = image + nmb + 2;
    if (sw > 0xFFFF) return 0;                      // staging offsets are 16-bit
    // The frame image is assembled in LDS whole, or one tile of 8 / 4 / 2 KiB at a time (+2: tile slack; at most 16 tiles).
    // Whole is a little faster (one merge sweep); a smaller tile is taken when that is what lets two 12-wavefront groups
    // share a CU (17-21 % faster than one 16-wavefront group: 640x480 at 8 KiB budgets needs the 4 KiB tile for it), or
    // what makes the geometry fit at all.
    const int tiles[4] = {image, 2048, 1024, 512};
    int lg = 1, ow = 0;
    for (int shape = 0; shape < 2 && !ow; shape++) {             // 0: two small groups per CU, 1: one large group
        for (int i = 0; i < 4 && !ow; i++) {
            const int t = tiles[i] < image ? tiles[i] : image;
            if ((image + t - 1) / t > kMaxTiles) continue;
            if ((shape ? 1 : 2) * psxhip_mdec_lds_bytes(nmb, t + 2, sw, shape) <= lds_cu) {
                lg = shape;
                ow = t + 2;
            }
        }
    }
    const int fits = ow != 0;
    if (!fits) {                                                 // nothing fits: report what the smallest working set would need
        lg = 1;
        ow = (image < 512 ? image : 512) + 2;
    }
    const size_t need = psxhip_mdec_lds_bytes(nmb, ow, sw, lg);
    if (large) *large = lg;
    if (out_words) *out_words = ow;
    if (stg_words) *stg_words = sw;
    if (lds_bytes) *lds_bytes = need;
    // (not "need <= lds_cu": the 512-dword tile of the report can be small enough where the image would take more than kMaxTiles of
    //  them -- 320x1024 at 80 000 bytes on 160 KiB is 40 tiles in 159 232 bytes -- and the kernel keeps kMaxTiles + 1 tile marks)
    return fits;
}

int mdec_max_budget(int width, int height, size_t lds_cu) {
    // (the LDS need grows by 8 bytes per budget dword)
    int lo = 8, hi = 1 << 20;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (mdec_geometry(width, height, mid, lds_cu, nullptr, nullptr, nullptr, nullptr)) lo = mid;
        else hi = mid - 1;
    }
    return mdec_geometry(width, height, lo, lds_cu, nullptr, nullptr, nullptr, nullptr) ? lo : 0;
}

int mdec_trips(int width, int height, int large) {
    const int waves = large ? kWavesLarge : kWavesSmall;
    return ((width / 16) * (height / 16) + waves - 1) / waves;
}

// iteration visiting stride: coprime with `trips`, near 0.38 * trips, so that any prefix of a pass samples the frame evenly
int mdec_pick_it_step(int trips) {
    if (trips <= 2) return 1;
    const int want = (trips * 382 + 500) / 1000;
    for (int d = 0; d < trips; d++) {
        const int cand[2] = {want + d, want - d};
        for (int i = 0; i < 2; i++) {
            const int c = cand[i];
            if (c < 1 || c >= trips) continue;
            int x = c, y = trips;
            while (y) { const int t = x % y; x = y; y = t; }
            if (x == 1) return c;
        }
    }
    return 1;
}

// The order in which a pass's tickets visit the macroblocks: ticket t = (round r = t / waves, slot w = t % waves) visits
// raster index w + seq[r] * waves.  For the rounds of the first quarter -- what the checkpoint looks at -- seq[r] =
// (r * step) % trips with step coprime to trips and close to 0.382 trips: they are spread evenly over the frame.  Entries
// past the last macroblock (the final round may be partial) hold kNoMb.  Returns the number of tickets (trips * waves).
extern "C" int psxhip_mdec_pass_order(int width, int height, int large, uint32_t* out, int cap) {
    const int waves = large ? kWavesLarge : kWavesSmall;
    const int nx = width / 16, nmb = nx * (height / 16);
    const int trips = mdec_trips(width, height, large), step = mdec_pick_it_step(trips);
    const int n = trips * waves;
    if (!out) return n;
    // The rounds before the checkpoint's mark (trips / 4 of them) are spread evenly over the frame, the rest follow in raster
    // order: a round's twelve macroblocks read 192-byte pieces of pixel rows, memory is fetched in 128-byte granules, and with
    // EVERY round scattered the half-used granules at a round's ends were gone from L2 before the neighbouring round came
    // (fetch 141 MB per 1000 frames of 320x240 against 115 MB of pixels; 123 MB with three quarters of the rounds in raster order).  Scattering all rounds in runs
    // of 3 or 5 neighbours instead (NOTEBOOK round 4) saves as much but changes what the checkpoint samples -- three
    // adjacent macroblock rows are no sample of a picture -- and moved noisy content by -12 .. +14 %.
    std::vector<int> seq;                                     // ticket round -> raster round (a permutation)
    std::vector<char> used((size_t)trips, 0);
    const int spread = trips >= 8 ? trips >> 2 : trips;       // (the kernel's check_t: no checkpoint below 8 rounds)
    for (int r = 0; r < spread; r++) { seq.push_back((r * step) % trips); used[seq.back()] = 1; }
    for (int rr = 0; rr < trips; rr++) if (!used[rr]) seq.push_back(rr);
    for (int t = 0; t < n && t < cap; t++) {
        const int m = t % waves + seq[t / waves] * waves;
        out[t] = m < nmb ? (uint32_t)(m % nx) | (uint32_t)(m / nx) << 8 : kNoMb;
    }
    return n;
}

// ... and the same order as the kernel reads it: per ticket {fy * 8 W | valid << 31, fx * 16 | 4 * encode-order index << 16} (an entry
// without a macroblock is all zero), followed by one all-zero entry (cap > n).  Returns the number of tickets n.
extern "C" int psxhip_mdec_pass_table(int width, int height, int large, uint32_t* out /* [2 * (n + 1)] */, int cap) {
    const int n = psxhip_mdec_pass_order(width, height, large, nullptr, 0);
    if (!out) return n;
    if (cap > n) { out[2 * n] = 0u; out[2 * n + 1] = 0u; }        // the entry tickets past the end are clamped onto
    std::vector<uint32_t> o((size_t)n);
    (void)psxhip_mdec_pass_order(width, height, large, o.data(), n);
    const int ny = height / 16;
    for (int t = 0; t < n && t < cap; t++) {
        if (o[t] == kNoMb) { out[2 * t] = 0u; out[2 * t + 1] = 0u; continue; }
        const uint32_t fx = o[t] & 0xFFu, fy = o[t] >> 8;
        out[2 * t] = (fy * 8u * (uint32_t)width) | 0x80000000u;
        out[2 * t + 1] = (fx * 16u) | ((fx * (uint32_t)ny + fy) * 4u << 16);
    }
    return n;
}

extern "C" int psxhip_mdec_split_geometry(int codec, int width, int height, int max_frame_size, int n_frames, int n_cu, psxhip_mdec_split_geo_t* g) {
    const int nx = width / 16, ny = height / 16, nmb = nx * ny;
    memset(g, 0, sizeof *g);
    if (nmb <= 0 || n_frames <= 0 || n_cu <= 0) return 0;
    // M: every group of every frame resident at once when that can be had (segments x frames <= CUs), and never more segments
    // than CUs per frame -- a frame's groups wait for each other
    int M = 2;
    while (M < 16 && (long long)((nmb + M - 1) / M) * n_frames > n_cu) M *= 2;
    static const int forced_m = [] { const char* e = getenv("PSXHIP_MDEC_SPLIT_M"); return e ? atoi(e) : 0; }();     // experiments only; read once
    if (forced_m == 1 || forced_m == 2 || forced_m == 4 || forced_m == 8 || forced_m == 16) M = forced_m;
    const int segs = (nmb + M - 1) / M;
    if (segs > n_cu) return 0;                                      // (more than 16 x CUs macroblocks: the frame kernel takes it)
    g->seg_mbs = M;
    g->segs = segs;
    g->img_words = (max_frame_size + 3) / 4 + 2;
    // the workspace's layout depends on the context's constants only (frame size, largest budget), not on M: launches of one
    // context with different M share it
    size_t o = 64;
    g->ws_slots = o;    o += (size_t)kSplitRounds * nmb * kSplitRound * 8;
    g->ws_dcq = o;      o += ((size_t)nmb * 3 * 4 + 15) & ~(size_t)15;
    g->ws_img = o;      o += ((size_t)g->img_words * 4 + 15) & ~(size_t)15;     // (every part starts on a 16-byte boundary)
    g->ws_done = o;     o += ((size_t)nmb * 4 + 15) & ~(size_t)15;
    g->ws_stride = (o + 127) & ~(size_t)127;
    g->lds_bytes = split_lds_bytes(codec, M, nmb);
    return g->lds_bytes <= 64 * 1024 ? 1 : 0;
}

MdecLaunchPlan mdec_launch_policy(const MdecLaunchConsts& k, int n_batches, int n_frames, bool stats, bool no_split) {
    MdecLaunchPlan p;
    memset(&p, 0, sizeof p);
    // A launch of a few frames: every frame across many workgroups (the reference's own pattern, one frame per call, most of all:
    // one workgroup would encode it on ONE compute unit while 255 idle)
    p.split = n_batches == 1 && n_frames <= k.split_max && !stats && !no_split &&
              psxhip_mdec_split_geometry(k.codec, k.width, k.height, k.max_frame_size, n_frames, k.n_cu, &p.geo);
    if (p.split) return p;
    // A batch of at most one frame per CU gains nothing from the two-group shape (its point is two frames per CU): such
    // launches use the 16-wavefront shape, which finishes a lone frame sooner -- the drop-in one-frame-per-call pattern most
    // of all.  (Tried and dropped: sending the REMAINDER of a large batch -- the frames past the last full round of
    // groups_max, when they are at most one per CU -- through that shape as a second launch.  1250 frames of 640x480 are
    // 2.44 rounds and the mean group is resident 76 % of the launch, but the frame tickets already let early finishers
    // start the third round while others are in their second; a second launch puts a barrier there instead: 1.176 ms
    // against 1.144 ms.)
    p.small_batch = k.order_large && n_frames <= k.n_cu;
    p.large = k.large || p.small_batch;
    p.trips = mdec_trips(k.width, k.height, p.large);
    p.it_step = mdec_pick_it_step(p.trips);
    // frame tickets: one frame each.  Tickets of 2 or 4 consecutive frames were built and measured, and not kept (NOTEBOOK round 5):
    // on top of the trust policy they changed mixed content by -2 .. +5 % and cost uniform content 10 % with two launch lanes.
    // Never more groups than tickets: every group of the kernel starts with a ticket of its own
    p.grid = n_frames < k.groups_max ? n_frames : k.groups_max;
    // frames are handed on only when a group can hold more than one (else nobody is left to take them), the queue has a slot per
    // frame, and a group holds FEW: from about eight frames per group on the fresh-frame tickets level the groups by themselves,
    // and a frame restarted on another XCD is read from HBM again (10 000 x 640x480: -1 % time, +8 % traffic with the queue)
    p.queue = k.retry_cap > 0 && n_frames > p.grid && n_frames <= 8 * p.grid && n_frames < k.retry_cap;
    return p;
}

int mdec_host_call_check(int max_frame_size, int n_frames, const int32_t* frame_max_sizes, int uniform_max_size, size_t out_stride, int row_bytes,
                         MdecHostCall* out) {
    int max_size = uniform_max_size;
    if (frame_max_sizes) {
        max_size = 0;
        for (int i = 0; i < n_frames; i++) {
            if (frame_max_sizes[i] < 8 || frame_max_sizes[i] > max_frame_size) {
                psxhip_set_error("encode_frames_host: frame %d budget %d outside [8, %d]", i, frame_max_sizes[i], max_frame_size);
                return PSXHIP_EINVAL;
            }
            if (frame_max_sizes[i] > max_size) max_size = frame_max_sizes[i];
        }
    } else if (uniform_max_size < 8 || uniform_max_size > max_frame_size) {
        psxhip_set_error("encode_frames_host: frame_max_size %d outside [8, %d]", uniform_max_size, max_frame_size);
        return PSXHIP_EINVAL;
    }
    if (row_bytes > 0) {
        if (row_bytes < max_size || row_bytes > max_frame_size) {
            psxhip_set_error("encode_frames_host: row width %d outside [%d, %d]", row_bytes, max_size, max_frame_size);
            return PSXHIP_EINVAL;
        }
        max_size = row_bytes;
    }
    if ((size_t)max_size > out_stride) {
        psxhip_set_error("encode_frames_host: out_stride %zu smaller than the largest budget %d", out_stride, max_size);
        return PSXHIP_EINVAL;
    }
    out->max_size = max_size;
    out->dstride = ((size_t)max_size + 3) & ~(size_t)3;
    return PSXHIP_OK;
}

int mdec_refine_call_check(int max_frame_size, size_t frame_bytes, const MdecRefineCall& a) {
    if (!a.d_frames || !a.d_out || !a.d_results || a.n_frames < 0) {
        psxhip_set_error("refine_frames_device: NULL argument");
        return PSXHIP_EINVAL;
    }
    if (a.max_magnitude < 1 || a.max_magnitude > 3) {
        psxhip_set_error("refine_frames_device: max_magnitude %d outside [1, 3]", a.max_magnitude);
        return PSXHIP_EINVAL;
    }
    if (a.frame_stride < frame_bytes || (a.frame_stride & 3) || (a.out_stride & 3) || ((uintptr_t)a.d_frames & 3) || ((uintptr_t)a.d_out & 3)) {
        psxhip_set_error("refine_frames_device: strides / pointers must be 4-byte aligned and frame_stride >= w*h*3/2");
        return PSXHIP_EINVAL;
    }
    if (!a.per_frame_budgets && (a.uniform_max_size < 8 || a.uniform_max_size > max_frame_size || (size_t)a.uniform_max_size > a.out_stride)) {
        psxhip_set_error("refine_frames_device: frame_max_size %d outside [8, %d] or larger than out_stride", a.uniform_max_size, max_frame_size);
        return PSXHIP_EINVAL;
    }
    if (a.n_frames > 0xFFFFFF) {
        psxhip_set_error("refine_frames_device: more than 16 777 215 frames in one call");
        return PSXHIP_EINVAL;
    }
    return PSXHIP_OK;
}

MdecShedWs mdec_shed_workspace(int n_blocks) {
    MdecShedWs w;
    const size_t nb = (size_t)n_blocks;
    w.acc = 0;
    w.decision = 13 * 64 * sizeof(int64_t);            // kShedRows rows (mdec_shed_core.h; the kernels assert the number)
    w.zeroed = w.decision + 64;
    w.dc_level = w.zeroed;
    w.dc_code = (w.dc_level + nb * sizeof(int16_t) + 15) & ~(size_t)15;
    w.block_off = w.dc_code + nb * sizeof(uint32_t);
    w.stride = (w.block_off + (nb + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
    return w;
}

int mdec_shed_analyse_groups(int nmb) { return (nmb + kShedAnalyseMbs - 1) / kShedAnalyseMbs; }

int mdec_chunk_frames(int groups_max, size_t frame_bytes, int n_frames) {
    // chunk: most of a GPU-load of frames -- small enough that a 1000-frame call already pipelines staging, DMA and kernel
    // over three chunks (353 k frames/s against 269 k with 1024-frame chunks), large enough for launches to stay efficient
    // (NOTEBOOK section 7)
    int chunk = groups_max * 3 / 4;
    const size_t staging_cap = (size_t)96 << 20;                  // pinned bytes per staging buffer
    if ((size_t)chunk * frame_bytes > staging_cap) chunk = (int)(staging_cap / frame_bytes);
    if (chunk < 1) chunk = 1;
    return chunk > n_frames ? n_frames : chunk;
}

MdecWithhold mdec_parse_withhold(const char* spec) {
    // frame:segment[:launches[:residue]] -- segment: 0 .. segs - 1 (larger: the last), negative: from the end (-1: the
    // finisher's own), "mid": segs / 2
    MdecWithhold w;
    char seg[16] = {0};
    int fr = 0, launches = 1, residue = 0;
    const int n = sscanf(spec, "%d:%15[^:]:%d:%d", &fr, seg, &launches, &residue);
    if (n >= 2 && fr >= 0 && launches > 0) {
        w.frame = fr;
        w.seg = strcmp(seg, "mid") == 0 ? INT_MIN : atoi(seg);
        w.launches = launches;
        w.residue = residue != 0;
    }
    return w;
}

int mdec_withhold_segment(int seg, int segs) {
    return seg == INT_MIN ? segs / 2 : (seg < 0 ? (segs + seg >= 0 ? segs + seg : 0) : (seg < segs ? seg : segs - 1));
}
