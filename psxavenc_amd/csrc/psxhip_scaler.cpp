// psxhip_scaler.cpp -- the scaler's C ABI (include/psxav_hip.h, psxhip_scaler_*): filter-bank design, the
// choice of the tile, the handle and its device tables.  The kernel is frontend_kernels.hip; no pixel is touched on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "device_buffer.h"
#include "psxhip_internal.h"

namespace {

// ---- filter bank, host side: the specification's integer arithmetic (see the header of oracle/frontend_oracle.c for the
//      same text as prose; the two are written independently and compared tap by tap in tests/test_gpu_frontend.py)
int64_t floor_div64(int64_t a, int64_t b) {
    int64_t q = a / b;
    if ((a % b != 0) && ((a < 0) != (b < 0))) q--;
    return q;
}
int64_t bicubic_weight(int64_t x) {          // x: |distance| / scale in 16.16; B = 0, C = 0.6, times 10 * 2^16
    const int64_t one = 65536;
    if (x < one) return ((14 * x * x * x) >> 32) - ((24 * x * x) >> 16) + 10 * one;
    if (x < 2 * one) return -((6 * x * x * x) >> 32) + ((30 * x * x) >> 16) - 48 * x + 24 * one;
    return 0;
}
struct HostBank {
    int taps = 0, taps4 = 0;
    std::vector<int32_t> left;
    std::vector<int16_t> coef;
    std::vector<uint32_t> digits;       // see Bank::digits
};
bool make_bank(int src, int dst, HostBank* b) {
    const int64_t xinc = (((int64_t)src << 16) + dst / 2) / dst;
    const int64_t scale = xinc > 65536 ? xinc : 65536;
    const int64_t R = 2 * scale;
    b->taps = (int)((2 * R + 65535) >> 16);
    if (b->taps > 64) return false;
    b->left.resize((size_t)dst);
    b->coef.resize((size_t)dst * b->taps);
    std::vector<int64_t> W((size_t)b->taps);
    for (int i = 0; i < dst; i++) {
        const int64_t c = (int64_t)i * xinc + ((xinc - 65536) >> 1);
        const int64_t l = floor_div64(c - R, 65536) + 1;
        int64_t sum = 0;
        int best = 0;
        for (int k = 0; k < b->taps; k++) {
            int64_t d = ((l + k) << 16) - c;
            if (d < 0) d = -d;
            W[(size_t)k] = bicubic_weight(d * 65536 / scale);
            sum += W[(size_t)k];
            if (W[(size_t)k] > W[(size_t)best]) best = k;
        }
        int64_t got = 0;
        for (int k = 0; k < b->taps; k++) {
            const int64_t q = W[(size_t)k] * 16384 / sum;
            b->coef[(size_t)i * b->taps + k] = (int16_t)q;
            got += q;
        }
        b->coef[(size_t)i * b->taps + best] = (int16_t)(b->coef[(size_t)i * b->taps + best] + (16384 - got));
        b->left[(size_t)i] = (int32_t)l;
    }
    // the taps as two balanced int8 digits, four to a dword (the horizontal pass's v_dot4_i32_i8 operands)
    b->taps4 = (b->taps + 3) / 4;
    b->digits.assign((size_t)dst * 2 * b->taps4, 0u);
    for (int i = 0; i < dst; i++)
        for (int k = 0; k < b->taps; k++) {
            const int c = b->coef[(size_t)i * b->taps + k];
            const int lo = ((c + 128) & 255) - 128, hi = (c - lo) >> 8;
            if (hi < -128 || hi > 127) return false;
            b->digits[((size_t)i * 2 + 0) * b->taps4 + k / 4] |= (uint32_t)(lo & 0xFF) << (8 * (k & 3));
            b->digits[((size_t)i * 2 + 1) * b->taps4 + k / 4] |= (uint32_t)(hi & 0xFF) << (8 * (k & 3));
        }
    return true;
}

}  // namespace

struct psxhip_scaler {
    int device, fmt, sw, sh, full_range, dw, dh;
    HostBank h[4];                 // lh, lv, ch, cv
    DeviceBuffer d_left[4], d_coef[4], d_digits[4];      // ... and their tables on the device
    psxhip_scaler_job_t job;
    size_t lds_bytes;
    size_t src_bytes;              // bytes of one source picture
    int n_cus;
};

extern "C" void psxhip_scaler_destroy(psxhip_scaler_t* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

extern "C" int psxhip_scaler_create(psxhip_scaler_t** out, int device, int src_format, int src_width, int src_height,
                                    int src_full_range, int dst_width, int dst_height) {
    if (!out) return PSXHIP_EINVAL;
    *out = nullptr;
    const bool yuv = src_format == PSXHIP_PIX_YUV420P;
    if ((src_format != PSXHIP_PIX_RGB24 && !yuv) || src_width < 2 || src_height < 2 || src_width > 16384 || src_height > 16384 ||
        dst_width < 16 || dst_height < 16 || (dst_width % 16) || (dst_height % 16) || dst_width > 1024 || dst_height > 1024 ||
        (yuv && ((src_width | src_height) & 1))) {
        psxhip_set_error("psxhip_scaler_create: bad geometry (%dx%d format %d -> %dx%d; the target must be a multiple of 16, YUV420P sources even)",
                         src_width, src_height, src_format, dst_width, dst_height);
        return PSXHIP_EINVAL;
    }
    int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    psxhip_scaler* s = new (std::nothrow) psxhip_scaler;
    if (!s) return PSXHIP_ENOMEM;
    struct Guard { psxhip_scaler* p; ~Guard() { if (p) psxhip_scaler_destroy(p); } } guard{s};
    s->device = device; s->fmt = src_format; s->sw = src_width; s->sh = src_height; s->full_range = src_full_range;
    s->dw = dst_width; s->dh = dst_height;
    const int csw = yuv ? src_width / 2 : src_width, csh = yuv ? src_height / 2 : src_height;
    {
        // lh, lv, ch, cv: RGB chroma is filtered from full resolution to half the target, so its banks shrink twice as much
        static const char* const names[4] = {"luma horizontal", "luma vertical", "chroma horizontal", "chroma vertical"};
        const int from[4] = {src_width, src_height, csw, csh}, to[4] = {dst_width, dst_height, dst_width / 2, dst_height / 2};
        for (int i = 0; i < 4; i++)
            if (!make_bank(from[i], to[i], &s->h[i])) {
                psxhip_set_error("psxhip_scaler_create: the %s filter (%d -> %d%s) shrinks by more than 16x, which is not supported",
                                 names[i], from[i], to[i], (i >= 2 && !yuv) ? ": RGB chroma is filtered from full resolution" : "");
                return PSXHIP_EINVAL;
            }
    }
    s->src_bytes = yuv ? (size_t)src_width * src_height * 3 / 2 : (size_t)src_width * src_height * 3;
    psxhip_scaler_job_t& j = s->job;
    memset(&j, 0, sizeof j);
    j.sw = src_width; j.sh = src_height; j.dw = dst_width; j.dh = dst_height;
    j.csw = csw; j.csh = csh;
    j.limited = yuv && !src_full_range;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device), PSXHIP_EDEVICE);
    s->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // tile: the largest of these whose LDS working set leaves room for at least two workgroups per CU
    // (PSXHIP_SCALER_TILE=k, tests: only shapes[k], taken if one workgroup fits a CU -- every shape can be run on purpose)
    const int shapes[4][2] = {{64, 16}, {32, 16}, {32, 8}, {16, 8}};
    int t_first = 0, t_last = 3;
    const char* forced = getenv("PSXHIP_SCALER_TILE");
    if (forced) {
        const int k = atoi(forced);
        if (k < 0 || k > 3) {
            psxhip_set_error("psxhip_scaler_create: PSXHIP_SCALER_TILE=%s is not a tile shape (0..3)", forced);
            return PSXHIP_EINVAL;
        }
        t_first = t_last = k;
    }
    size_t need = 0;
    bool ok = false;
    for (int t = t_first; t <= t_last && !ok; t++) {
        const int TW = shapes[t][0], TH = shapes[t][1];
        // the largest source reach of any tile, from the tables
        auto reach = [](const HostBank& b, int n, int tile) {
            int best = 0;
            for (int a = 0; a < n; a += tile) {
                const int e = (a + tile < n ? a + tile : n) - 1;
                const int sp = b.left[(size_t)e] + b.taps - b.left[(size_t)a];
                if (sp > best) best = sp;
            }
            return best;
        };
        int reg_rows, reg_cols, creg_rows, creg_cols;
        if (yuv) {
            // every plane's region starts and ends on a multiple of sixteen samples (a lane stages sixteen bytes)
            auto reach4 = [](const HostBank& b, int n, int tile) {
                int best = 0;
                for (int a = 0; a < n; a += tile) {
                    const int e = (a + tile < n ? a + tile : n) - 1;
                    const int lo = b.left[(size_t)a] & ~15, hi = (b.left[(size_t)e] + b.taps + 15) & ~15;
                    if (hi - lo > best) best = hi - lo;
                }
                return best;
            };
            reg_rows = reach(s->h[1], dst_height, TH); reg_cols = reach4(s->h[0], dst_width, TW);
            creg_rows = reach(s->h[3], dst_height / 2, TH / 2); creg_cols = reach4(s->h[2], dst_width / 2, TW / 2);
        } else {
            // the union of the luma and the chroma reach over the same full-resolution picture: bounded by the larger span plus
            // the offset between the two windows (at most the larger filter's half width); take the exact maximum over the tiles
            reg_rows = 0; reg_cols = 0;
            for (int a = 0; a < dst_width; a += TW) {
                const int e = (a + TW < dst_width ? a + TW : dst_width) - 1;
                const int lo = std::min(s->h[0].left[(size_t)a], s->h[2].left[(size_t)(a / 2)]) & ~3;       // whole groups of four pixels
                const int hi = (std::max(s->h[0].left[(size_t)e] + s->h[0].taps, s->h[2].left[(size_t)(e / 2)] + s->h[2].taps) + 3) & ~3;
                reg_cols = std::max(reg_cols, hi - lo);
            }
            for (int a = 0; a < dst_height; a += TH) {
                const int e = (a + TH < dst_height ? a + TH : dst_height) - 1;
                const int lo = std::min(s->h[1].left[(size_t)a], s->h[3].left[(size_t)(a / 2)]);
                const int hi = std::max(s->h[1].left[(size_t)e] + s->h[1].taps, s->h[3].left[(size_t)(e / 2)] + s->h[3].taps);
                reg_rows = std::max(reg_rows, hi - lo);
            }
            creg_rows = reg_rows; creg_cols = reg_cols;
        }
        // + 8: the horizontal pass reads a window as whole dwords, up to 7 bytes past the last tap (zero digits there)
        const size_t plane = ((size_t)reg_rows * reg_cols + 8 + 15) & ~(size_t)15;
        const size_t cplane = yuv ? (((size_t)creg_rows * creg_cols + 8 + 15) & ~(size_t)15) : plane;
        const size_t crows_cap = yuv ? (size_t)creg_rows : (size_t)reg_rows;
        const size_t v_words = (size_t)TH + TH / 2 + ((size_t)TH * s->h[1].taps + (size_t)(TH / 2) * s->h[3].taps + 1) / 2;      // one tile's vertical tables
        need = plane + 2 * cplane + 2 * ((size_t)reg_rows * TW + 2 * crows_cap * (TW / 2)) +
               8 * ((size_t)TW * s->h[0].taps4 + (size_t)(TW / 2) * s->h[2].taps4) + 4 * ((size_t)TW + TW / 2) + 4 * 2 * v_words + 16 * (((size_t)dst_height + TH - 1) / TH) + 16;
        if (need * 2 <= (size_t)prop.maxSharedMemoryPerMultiProcessor || ((t == 3 || forced) && need <= (size_t)prop.maxSharedMemoryPerMultiProcessor)) {
            ok = true;
            j.TW = TW; j.TH = TH;
            j.reg_rows = reg_rows; j.reg_cols = reg_cols; j.creg_rows = creg_rows; j.creg_cols = creg_cols;
        }
    }
    if (!ok && forced) {
        psxhip_set_error("psxhip_scaler_create: tile %dx%d (PSXHIP_SCALER_TILE=%d) needs %zu bytes of LDS, more than the %d of a compute unit",
                         shapes[t_first][0], shapes[t_first][1], t_first, need, (int)prop.maxSharedMemoryPerMultiProcessor);
        return PSXHIP_EINVAL;
    }
    if (!ok) {
        psxhip_set_error("psxhip_scaler_create: the filters' reach (%zu bytes of LDS per tile) does not fit a compute unit", need);
        return PSXHIP_EINVAL;
    }
    s->lds_bytes = need;
    j.tiles_x = (dst_width + j.TW - 1) / j.TW;
    j.tiles_y = (dst_height + j.TH - 1) / j.TH;
    psxhip_scaler_bank_t* banks[4] = {&j.lh, &j.lv, &j.ch, &j.cv};
    for (int i = 0; i < 4; i++) {
        const HostBank& h = s->h[i];
        const size_t left_bytes = h.left.size() * sizeof(int32_t), coef_bytes = h.coef.size() * sizeof(int16_t), digits_bytes = h.digits.size() * sizeof(uint32_t);
        if ((rc = s->d_left[i].reserve(left_bytes)) || (rc = s->d_coef[i].reserve(coef_bytes)) || (rc = s->d_digits[i].reserve(digits_bytes))) return rc;
        HIP_TRY(hipMemcpy(s->d_left[i].p, h.left.data(), left_bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
        HIP_TRY(hipMemcpy(s->d_coef[i].p, h.coef.data(), coef_bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
        HIP_TRY(hipMemcpy(s->d_digits[i].p, h.digits.data(), digits_bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
        banks[i]->left = s->d_left[i].as<int32_t>();
        banks[i]->coef = s->d_coef[i].as<int16_t>();
        banks[i]->digits = s->d_digits[i].as<uint32_t>();
        banks[i]->taps = h.taps;
        banks[i]->taps4 = h.taps4;
    }
    HIP_TRY(psxhip_scaler_prepare(yuv, (int)prop.maxSharedMemoryPerMultiProcessor), PSXHIP_EDEVICE);
    guard.p = nullptr;
    *out = s;
    return PSXHIP_OK;
}

extern "C" size_t psxhip_scaler_source_bytes(const psxhip_scaler_t* s) { return s ? s->src_bytes : 0; }

extern "C" int psxhip_scaler_filter(const psxhip_scaler_t* s, int which, int* taps, int32_t* left, int16_t* coef, int cap) {
    if (!s || which < 0 || which > 3) return PSXHIP_EINVAL;
    const HostBank& b = s->h[which];
    if (taps) *taps = b.taps;
    const int n = (int)b.left.size();
    if (left && coef) {
        if (cap < n * b.taps) return PSXHIP_EINVAL;
        memcpy(left, b.left.data(), (size_t)n * sizeof(int32_t));
        memcpy(coef, b.coef.data(), (size_t)n * b.taps * sizeof(int16_t));
    }
    return n;
}

extern "C" int psxhip_scaler_convert_device(psxhip_scaler_t* s, const uint8_t* d_src, size_t src_stride, int n_frames,
                                            uint8_t* d_frames, size_t frame_stride, void* stream) {
    if (!s || !d_src || !d_frames || n_frames < 0) {
        psxhip_set_error("psxhip_scaler_convert_device: NULL argument");
        return PSXHIP_EINVAL;
    }
    if (n_frames == 0) return PSXHIP_OK;
    if (src_stride < s->src_bytes || frame_stride < (size_t)s->dw * s->dh * 3 / 2 || (frame_stride & 3) || ((uintptr_t)d_frames & 3)) {
        psxhip_set_error("psxhip_scaler_convert_device: strides too small, or the output not 4-byte aligned");
        return PSXHIP_EINVAL;
    }
    HIP_TRY(hipSetDevice(s->device), PSXHIP_EDEVICE);
    psxhip_scaler_job_t j = s->job;
    j.src = d_src; j.src_stride = src_stride; j.out = d_frames; j.frame_stride = frame_stride;
    // a band walks the picture top to bottom; a small batch is cut into vertical segments until the chip has ~4 workgroups per CU
    // (each segment re-reads the rows its first tile reaches)
    const long long want = 4LL * s->n_cus;
    long long segs = (want + (long long)j.tiles_x * n_frames - 1) / ((long long)j.tiles_x * n_frames);
    if (segs < 1) segs = 1;
    if (segs > j.tiles_y) segs = j.tiles_y;
    if (const char* e = getenv("PSXHIP_SCALER_VSEGS")) { segs = atoi(e); if (segs < 1) segs = 1; if (segs > j.tiles_y) segs = j.tiles_y; }   // experiments
    j.vsegs = (int)segs;
    for (int f0 = 0; f0 < n_frames; f0 += 65535) {            // gridDim.y limit
        const int nf = n_frames - f0 < 65535 ? n_frames - f0 : 65535;
        j.src = d_src + (size_t)f0 * src_stride;
        j.out = d_frames + (size_t)f0 * frame_stride;
        HIP_TRY(psxhip_scaler_launch(&j, s->fmt == PSXHIP_PIX_YUV420P, nf, s->lds_bytes, stream), PSXHIP_EDEVICE);
    }
    return PSXHIP_OK;
}

extern "C" int psxhip_scaler_convert_host(psxhip_scaler_t* s, const uint8_t* src, int n_frames, uint8_t* frames) {
    if (!s || !src || !frames || n_frames < 0) return PSXHIP_EINVAL;
    if (n_frames == 0) return PSXHIP_OK;
    HIP_TRY(hipSetDevice(s->device), PSXHIP_EDEVICE);
    const size_t fsz = (size_t)s->dw * s->dh * 3 / 2;
    DeviceBuffer d_src, d_out;
    int rc;
    if ((rc = d_src.reserve(s->src_bytes * (size_t)n_frames)) || (rc = d_out.reserve(fsz * (size_t)n_frames))) return rc;
    HIP_TRY(hipMemcpy(d_src.p, src, s->src_bytes * (size_t)n_frames, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    rc = psxhip_scaler_convert_device(s, d_src.as<uint8_t>(), s->src_bytes, n_frames, d_out.as<uint8_t>(), fsz, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(frames, d_out.p, fsz * (size_t)n_frames, hipMemcpyDeviceToHost), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}
