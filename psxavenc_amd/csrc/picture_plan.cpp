// picture_plan.cpp -- the picture front ends' plans (picture_plan.h): the scaler's geometry rules, filter banks, tile, segments; the
// ingest's rules, matrix and planners; the display back-end's rules.  No HIP, no device: arithmetic and refusals.
#include "picture_plan.h"

#include <math.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "display_core.h"

static_assert(ING_SRC_YUV420P == PSXHIP_SRC_YUV420P && ING_SRC_YUV444P == PSXHIP_SRC_YUV444P && ING_SRC_NV21 == PSXHIP_SRC_NV21 &&
              ING_SRC_UYVY422 == PSXHIP_SRC_UYVY422 && ING_SRC_YUV444P10 == PSXHIP_SRC_YUV444P10 && ING_SRC_P010 == PSXHIP_SRC_P010 &&
              ING_SRC_GRAY8 == PSXHIP_SRC_GRAY8 && ING_SRC_RGB24 == PSXHIP_SRC_RGB24 && ING_SRC_BGRA32 == PSXHIP_SRC_BGRA32,
              "ingest_core.h restates the source formats");
static_assert(ING_OUT_RGB24 == PSXHIP_PIX_RGB24 && ING_OUT_YUV420P == PSXHIP_PIX_YUV420P && ING_CHROMA_BILINEAR == PSXHIP_INGEST_CHROMA_BILINEAR,
              "ingest_core.h restates the outputs and the options");
static_assert(DISP_RGB24 == PSXHIP_OUT_RGB24 && DISP_RGBX32 == PSXHIP_OUT_RGBX32 && DISP_RGB555 == PSXHIP_OUT_RGB555, "display_core.h restates the formats");
static_assert(DISP_CHROMA_BILINEAR == PSXHIP_DISPLAY_CHROMA_BILINEAR && DISP_DITHER == PSXHIP_DISPLAY_DITHER && DISP_MASK_BIT == PSXHIP_DISPLAY_MASK_BIT,
              "display_core.h restates the options");

int picture_bad(const char* who, const char* what) {
    psxhip_set_error("%s: %s", who, what);
    return PSXHIP_EINVAL;
}

// ================================================================================================ the scaler
int scaler_geometry_check(int src_format, int src_width, int src_height, int dst_width, int dst_height) {
    const bool yuv = src_format == PSXHIP_PIX_YUV420P;
    if ((src_format != PSXHIP_PIX_RGB24 && !yuv) || src_width < 2 || src_height < 2 || src_width > 16384 || src_height > 16384 ||
        dst_width < 16 || dst_height < 16 || (dst_width % 16) || (dst_height % 16) || dst_width > 1024 || dst_height > 1024 ||
        (yuv && ((src_width | src_height) & 1))) {
        psxhip_set_error("psxhip_scaler_create: bad geometry (%dx%d format %d -> %dx%d; the target must be a multiple of 16, YUV420P sources even)",
                         src_width, src_height, src_format, dst_width, dst_height);
        return PSXHIP_EINVAL;
    }
    return PSXHIP_OK;
}

namespace {

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

}  // namespace

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
            int64_t d = (l + k) * 65536 - c;          // (not << 16: l + k is negative at the picture's edge)
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

int scaler_design_banks(int src_format, int src_width, int src_height, int dst_width, int dst_height, HostBank h[4]) {
    const bool yuv = src_format == PSXHIP_PIX_YUV420P;
    const int csw = yuv ? src_width / 2 : src_width, csh = yuv ? src_height / 2 : src_height;
    // lh, lv, ch, cv: RGB chroma is filtered from full resolution to half the target, so its banks shrink twice as much
    static const char* const names[4] = {"luma horizontal", "luma vertical", "chroma horizontal", "chroma vertical"};
    const int from[4] = {src_width, src_height, csw, csh}, to[4] = {dst_width, dst_height, dst_width / 2, dst_height / 2};
    for (int i = 0; i < 4; i++)
        if (!make_bank(from[i], to[i], &h[i])) {
            psxhip_set_error("psxhip_scaler_create: the %s filter (%d -> %d%s) shrinks by more than 16x, which is not supported",
                             names[i], from[i], to[i], (i >= 2 && !yuv) ? ": RGB chroma is filtered from full resolution" : "");
            return PSXHIP_EINVAL;
        }
    return PSXHIP_OK;
}

namespace {

// The largest source reach of any tile of `tile` outputs out of n, from the tables: first source sample of the tile's first output
// to past the last tap of its last, both moved outward to multiples of `align` samples (a power of two: the granule a lane stages).
// With `c`, the union with the chroma bank's reach over the same source (RGB): its outputs are the luma's halved.
int reach(const HostBank& b, const HostBank* c, int n, int tile, int align) {
    int best = 0;
    for (int a = 0; a < n; a += tile) {
        const int e = (a + tile < n ? a + tile : n) - 1;
        int lo = b.left[(size_t)a], hi = b.left[(size_t)e] + b.taps;
        if (c) {
            lo = std::min(lo, c->left[(size_t)(a / 2)]);
            hi = std::max(hi, c->left[(size_t)(e / 2)] + c->taps);
        }
        best = std::max(best, ((hi + align - 1) & ~(align - 1)) - (lo & ~(align - 1)));
    }
    return best;
}

}  // namespace

int scaler_choose_tile(const HostBank h[4], bool yuv, int dst_width, int dst_height, size_t lds_per_cu, const char* forced,
                       psxhip_scaler_job_t* j, size_t* lds_bytes) {
    int t_first = 0, t_last = 3;
    if (forced) {
        const int k = atoi(forced);
        if (k < 0 || k > 3) {
            psxhip_set_error("psxhip_scaler_create: PSXHIP_SCALER_TILE=%s is not a tile shape (0..3)", forced);
            return PSXHIP_EINVAL;
        }
        t_first = t_last = k;
    }
    psxhip_scaler_bank_t* banks[4] = {&j->lh, &j->lv, &j->ch, &j->cv};
    for (int i = 0; i < 4; i++) { banks[i]->taps = h[i].taps; banks[i]->taps4 = h[i].taps4; }
    size_t need = 0;
    for (int t = t_first; t <= t_last; t++) {
        psxhip_scaler_job_t c = *j;
        const int TW = c.TW = kScalerShapes[t][0], TH = c.TH = kScalerShapes[t][1];
        c.tiles_x = (dst_width + TW - 1) / TW;
        c.tiles_y = (dst_height + TH - 1) / TH;
        if (yuv) {
            // every plane's region starts and ends on a multiple of sixteen samples (a lane stages sixteen bytes)
            c.reg_rows = reach(h[1], nullptr, dst_height, TH, 1); c.reg_cols = reach(h[0], nullptr, dst_width, TW, 16);
            c.creg_rows = reach(h[3], nullptr, dst_height / 2, TH / 2, 1); c.creg_cols = reach(h[2], nullptr, dst_width / 2, TW / 2, 16);
        } else {
            // the union of the luma and the chroma reach over the same full-resolution picture: bounded by the larger span plus
            // the offset between the two windows (at most the larger filter's half width); the exact maximum over the tiles, in
            // whole groups of four pixels across
            c.creg_rows = c.reg_rows = reach(h[1], &h[3], dst_height, TH, 1);
            c.creg_cols = c.reg_cols = reach(h[0], &h[2], dst_width, TW, 4);
        }
        need = (size_t)scaler_job_lds(c, yuv).total;
        if (need * 2 <= lds_per_cu || ((t == 3 || forced) && need <= lds_per_cu)) {
            *j = c;
            *lds_bytes = need;
            return PSXHIP_OK;
        }
    }
    if (forced)
        psxhip_set_error("psxhip_scaler_create: tile %dx%d (PSXHIP_SCALER_TILE=%d) needs %zu bytes of LDS, more than the %d of a compute unit",
                         kScalerShapes[t_first][0], kScalerShapes[t_first][1], t_first, need, (int)lds_per_cu);
    else
        psxhip_set_error("psxhip_scaler_create: the filters' reach (%zu bytes of LDS per tile) does not fit a compute unit", need);
    return PSXHIP_EINVAL;
}

int scaler_vsegs(int n_cus, int tiles_x, int tiles_y, int n_frames, const char* override_) {
    const long long want = 4LL * n_cus;
    long long segs = override_ ? atoi(override_) : (want + (long long)tiles_x * n_frames - 1) / ((long long)tiles_x * n_frames);
    if (segs < 1) segs = 1;
    if (segs > tiles_y) segs = tiles_y;
    return (int)segs;
}

int scaler_convert_check(const char* who, bool handle, uintptr_t src, uintptr_t dst, int n_frames, bool device_entry, size_t src_stride,
                         size_t frame_stride, size_t src_bytes, int dst_width, int dst_height, bool* go) {
    *go = false;
    if (!handle || !src || !dst || n_frames < 0) return picture_bad(who, "NULL argument");
    if (n_frames == 0) return PSXHIP_OK;
    if (device_entry && (src_stride < src_bytes || frame_stride < (size_t)dst_width * dst_height * 3 / 2 || (frame_stride & 3) || (dst & 3)))
        return picture_bad(who, "strides too small, or the output not 4-byte aligned");
    *go = true;
    return PSXHIP_OK;
}

// ================================================================================================ the picture ingest
namespace {

// Kr and Kb over 10000, by PSXHIP_MATRIX_*
const int kKr[5] = {2990, 2126, 2120, 3000, 2627}, kKb[5] = {1140, 722, 870, 1100, 593};

int64_t floor_div(int64_t a, int64_t b) {      // b > 0
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
// round-half-up of 65536 num / den, den > 0: floor(65536 num / den + 1 / 2)
int32_t fixed16(int64_t num, int64_t den) { return (int32_t)floor_div(2 * 65536 * num + den, 2 * den); }

// the seven numbers of the matrix, in int64 throughout; d: the bit depth
void make_matrix(int matrix, bool full_range, int depth, IngestDesc* o) {
    const int64_t s = (int64_t)1 << (depth - 8), top = ((int64_t)1 << depth) - 1;
    const int64_t yn = 255, yd = full_range ? top : 219 * s;          // luma gain
    const int64_t cn = 255, cd = full_range ? top : 224 * s;          // chroma gain
    const int64_t kr = kKr[matrix], kb = kKb[matrix], kg = 10000 - kr - kb, one = 10000;
    o->cy = fixed16(yn, yd);
    o->rv = fixed16(2 * (one - kr) * cn, one * cd);
    o->bu = fixed16(2 * (one - kb) * cn, one * cd);
    o->gu = fixed16(-2 * kb * (one - kb) * cn, one * kg * cd);
    o->gv = fixed16(-2 * kr * (one - kr) * cn, one * kg * cd);
    o->yoff = full_range ? 0 : (int)(16 * s);
    o->coff = 1 << (depth - 1);
}

bool yuv_or_grey(const IngestFormat& f) { return f.layout >= 0 && f.layout != ING_RGB; }
bool may_be_yuv420p(const IngestFormat& f, int matrix, int w, int h) {
    return yuv_or_grey(f) && matrix == PSXHIP_MATRIX_BT601 && !((w | h) & 1);
}

}  // namespace

int ingest_create_plan(int src_format, int width, int height, const psxhip_ingest_plane_t* planes, int n_planes, int matrix, int full_range,
                       int out_format, uint32_t options, IngestPlan* out) {
    const char* who = "psxhip_ingest_create";
    if (!planes) return picture_bad(who, "NULL argument");
    IngestDesc d = {};
    d.f = ingest_format(src_format);
    if (d.f.layout < 0) return picture_bad(who, "unknown source format");
    if (n_planes != d.f.planes) {
        psxhip_set_error("%s: source format %d has %d planes, %d given", who, src_format, d.f.planes, n_planes);
        return PSXHIP_EINVAL;
    }
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return picture_bad(who, "width and height are 1 .. 16384");
    if (d.f.layout == ING_PACKED422 && (width & 1)) return picture_bad(who, "a packed 4:2:2 source has an even width");
    if (options & ~(uint32_t)PSXHIP_INGEST_CHROMA_BILINEAR) return picture_bad(who, "unknown option bit");
    const bool yuv = yuv_or_grey(d.f);
    if (yuv && (matrix < 0 || matrix > PSXHIP_MATRIX_BT2020_NCL)) return picture_bad(who, "unknown matrix");
    if (out_format != PSXHIP_PIX_RGB24 && out_format != PSXHIP_PIX_YUV420P) return picture_bad(who, "out_format is PSXHIP_PIX_RGB24 or PSXHIP_PIX_YUV420P");
    if (out_format == PSXHIP_PIX_YUV420P) {
        if (!yuv) return picture_bad(who, "PSXHIP_PIX_YUV420P output takes a YUV or grey source, not packed RGB");
        if (matrix != PSXHIP_MATRIX_BT601) return picture_bad(who, "PSXHIP_PIX_YUV420P output copies the samples, which the scaler reads as BT.601: another matrix needs PSXHIP_PIX_RGB24");
        if ((width | height) & 1) return picture_bad(who, "PSXHIP_PIX_YUV420P output needs an even width and height");
    }
    d.w = width; d.h = height;
    d.bilinear = (options & PSXHIP_INGEST_CHROMA_BILINEAR) ? 1 : 0;
    size_t begin[3], end[3], extent = 0;
    for (int p = 0; p < n_planes; p++) {
        const size_t row = ing_row_bytes(d, p), rows = (size_t)ing_plane_rows(d, p);
        if (planes[p].offset > 0x7fffffffu || planes[p].pitch > 0x7fffffffu || planes[p].pitch < row) {
            psxhip_set_error("%s: plane %d: pitch %zu is below its row's %zu bytes, or offset / pitch above 2^31 - 1", who, p, planes[p].pitch, row);
            return PSXHIP_EINVAL;
        }
        if (d.f.bytes == 2 && ((planes[p].offset | planes[p].pitch) & 1)) {
            psxhip_set_error("%s: plane %d: a 16-bit format needs an even offset and pitch", who, p);
            return PSXHIP_EINVAL;
        }
        d.off[p] = (uint32_t)planes[p].offset;
        d.pitch[p] = (uint32_t)planes[p].pitch;
        begin[p] = planes[p].offset;
        end[p] = planes[p].offset + (rows - 1) * planes[p].pitch + row;
        if (end[p] > extent) extent = end[p];
        for (int q = 0; q < p; q++)
            if (begin[p] < end[q] && begin[q] < end[p]) {
                psxhip_set_error("%s: planes %d and %d overlap", who, q, p);
                return PSXHIP_EINVAL;
            }
    }
    if (yuv) make_matrix(matrix, full_range != 0, d.f.bytes == 2 ? 10 : 8, &d);
    out->d = d;
    out->out_format = out_format;
    out->src_bytes = extent;
    out->out_bytes = out_format == PSXHIP_PIX_RGB24 ? (size_t)width * height * 3 : (size_t)width * height * 3 / 2;
    return PSXHIP_OK;
}

int ingest_check(const char* who, const IngestPlan* p, uintptr_t src, size_t src_stride, int n_src, int n_out, uintptr_t dst, size_t out_stride,
                 bool device_pointers, bool* go) {
    *go = false;
    if (!p) return picture_bad(who, "NULL argument");
    if (n_src < 0 || n_out < 0) return picture_bad(who, "negative picture count");
    if (n_out == 0) return PSXHIP_OK;
    if (!src || !dst || n_src == 0) return picture_bad(who, "NULL argument, or output pictures without source pictures");
    if (src_stride < p->src_bytes || out_stride < p->out_bytes) {
        psxhip_set_error("%s: strides too small: src_stride %zu below the picture's %zu bytes, or out_stride %zu below %zu", who, src_stride,
                         p->src_bytes, out_stride, p->out_bytes);
        return PSXHIP_EINVAL;
    }
    if (p->d.f.bytes == 2 && ((src_stride & 1) || (device_pointers && (src & 1)))) return picture_bad(who, "a 16-bit format needs an even source address and src_stride");
    if (device_pointers) {
        const uintptr_t s = src, s_end = s + (size_t)(n_src - 1) * src_stride + p->src_bytes;
        const uintptr_t o = dst, o_end = o + (size_t)(n_out - 1) * out_stride + p->out_bytes;
        if (s < o_end && o < s_end) return picture_bad(who, "d_out overlaps d_src");
    }
    *go = true;
    return PSXHIP_OK;
}

// ---- the planners: no device

extern "C" int psxhip_ingest_recommend(int src_format, int matrix, int width, int height) {
    const IngestFormat f = ingest_format(src_format);
    if (f.layout < 0 || width < 1 || height < 1) return picture_bad("psxhip_ingest_recommend", "unknown source format, or an empty picture");
    return may_be_yuv420p(f, matrix, width, height) ? PSXHIP_PIX_YUV420P : PSXHIP_PIX_RGB24;
}

// psxavenc/decoding.c:275-285, in its own double-precision expressions
extern "C" int psxhip_ingest_fit(int src_w, int src_h, int max_w, int max_h, int ignore_aspect, int* dst_w, int* dst_h) {
    const char* who = "psxhip_ingest_fit";
    if (!dst_w || !dst_h) return picture_bad(who, "NULL argument");
    if (src_w < 1 || src_h < 1 || max_w < 16 || max_h < 16 || max_w > 1024 || max_h > 1024 || (max_w & 15) || (max_h & 15))
        return picture_bad(who, "the source is empty, or the maximum is not a multiple of 16 in 16 .. 1024");
    int w = max_w, h = max_h;
    if (!ignore_aspect) {
        const double src_ratio = (double)src_w / (double)src_h;
        const double dst_ratio = (double)max_w / (double)max_h;
        if (src_ratio < dst_ratio) {
            const double v = round((double)h * src_ratio);
            w = v >= 0 && v < 1e9 ? ((int)v + 15) & ~15 : 0;
        } else {
            const double v = round((double)w / src_ratio);
            h = v >= 0 && v < 1e9 ? ((int)v + 15) & ~15 : 0;
        }
    }
    if (w < 1 || h < 1 || w > max_w || h > max_h) {
        psxhip_set_error("%s: %dx%d fitted into %dx%d comes out %dx%d: a side is 0 or above its maximum", who, src_w, src_h, max_w, max_h, w, h);
        return PSXHIP_EINVAL;
    }
    *dst_w = w;
    *dst_h = h;
    return PSXHIP_OK;
}

// psxavenc/decoding.c:412-461: which decoded picture each output frame is made of
extern "C" int psxhip_ingest_pace(const int64_t* pts, int n, int tb_num, int tb_den, int fps_num, int fps_den, int32_t* out_index, int cap) {
    const char* who = "psxhip_ingest_pace";
    if (n < 0 || (n > 0 && !pts) || tb_num < 1 || tb_den < 1 || fps_num < 1 || fps_den < 1 || cap < 0 || (cap > 0 && !out_index))
        return picture_bad(who, "NULL argument, a negative count, or a time base or frame rate that is not positive");
    const double step = (double)fps_den / (double)fps_num;
    double next = 0.0;
    int64_t count = 0;
    int32_t last = -1;
    for (int i = 0; i < n; i++) {
        const double p = (double)pts[i] * (double)tb_num / (double)tb_den;
        if (count >= 1 && p < next) continue;                    // ahead of the clock: dropped
        if (count < 1) next = p;
        else next += step;
        const double gap = ceil((p - next) / step);
        if (gap > 1e9) return picture_bad(who, "a gap of more than 10^9 frames");
        for (int dupes = gap > 0 ? (int)gap : 0; dupes; dupes--) {
            if (count < cap) out_index[count] = last;
            count++;
            next += step;
        }
        if (count < cap) out_index[count] = i;
        count++;
        last = i;
        if (count > 0x7fffffff) return picture_bad(who, "more than 2^31 - 1 output frames");
    }
    return (int)count;
}

// ================================================================================================ the display back-end
extern "C" size_t psxhip_display_row_bytes(int out_format, int width) {
    return width > 0 ? (size_t)disp_row_bytes(out_format, width) : 0;
}

int psxhip_display_check(const char* who, const psxhip_display_job_t* j, bool device_pointers) {
    if (j->n_frames < 0 || (j->n_frames > 0 && (!j->d_frames || !j->d_dst))) {
        psxhip_set_error("%s: NULL argument or negative frame count", who);
        return PSXHIP_EINVAL;
    }
    if (j->width < 16 || j->height < 16 || j->width > 1024 || j->height > 1024 || (j->width & 15) || (j->height & 15)) {
        psxhip_set_error("%s: %dx%d is not a multiple of 16 in 16 .. 1024", who, j->width, j->height);
        return PSXHIP_EINVAL;
    }
    const size_t row = psxhip_display_row_bytes(j->out_format, j->width);
    if (!row) {
        psxhip_set_error("%s: unknown out_format %d", who, j->out_format);
        return PSXHIP_EINVAL;
    }
    const uint32_t known = PSXHIP_DISPLAY_CHROMA_BILINEAR | PSXHIP_DISPLAY_DITHER | PSXHIP_DISPLAY_MASK_BIT;
    if ((j->options & ~known) ||
        (j->out_format != PSXHIP_OUT_RGB555 && (j->options & (PSXHIP_DISPLAY_DITHER | PSXHIP_DISPLAY_MASK_BIT)))) {
        psxhip_set_error("%s: options 0x%x: an unknown bit, or dither / mask bit with a format other than RGB555", who, (unsigned)j->options);
        return PSXHIP_EINVAL;
    }
    const size_t frame_bytes = (size_t)j->width * j->height * 3 / 2;
    if ((device_pointers && ((uintptr_t)j->d_frames & 3)) || (j->frame_stride & 3) || j->frame_stride < frame_bytes) {
        psxhip_set_error("%s: d_frames / frame_stride not 4-byte aligned, or frame_stride below %zu", who, frame_bytes);
        return PSXHIP_EINVAL;
    }
    const size_t picture = (size_t)(j->height - 1) * j->dst_pitch + row;
    if ((device_pointers && ((uintptr_t)j->d_dst & 3)) || (j->dst_pitch & 3) || (j->dst_stride & 3) || j->dst_pitch < row || j->dst_stride < picture) {
        psxhip_set_error("%s: d_dst / dst_pitch / dst_stride not 4-byte aligned, dst_pitch below %zu or dst_stride below %zu", who, row, picture);
        return PSXHIP_EINVAL;
    }
    if (device_pointers && j->n_frames > 0) {
        const uintptr_t src = (uintptr_t)j->d_frames, src_end = src + (size_t)(j->n_frames - 1) * j->frame_stride + frame_bytes;
        const uintptr_t dst = (uintptr_t)j->d_dst, dst_end = dst + (size_t)(j->n_frames - 1) * j->dst_stride + picture;
        if (src < dst_end && dst < src_end) {
            psxhip_set_error("%s: d_dst overlaps d_frames", who);
            return PSXHIP_EINVAL;
        }
    }
    return PSXHIP_OK;
}
