// psxhip_ingest.cpp -- host side of the picture ingest (psxhip_ingest_*; include/psxav_hip.h): the source's
// rules, the matrix in exact integers, the entry points' staging and launches (ingest_kernels.hip), and the two planners that restate
// psxavenc/decoding.c's aspect fit and frame pacing.  No pixel is touched on the host.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <new>

#include "device_buffer.h"
#include "ingest_core.h"
#include "psxhip_ingest_internal.h"
#include "psxhip_internal.h"

static_assert(ING_SRC_YUV420P == PSXHIP_SRC_YUV420P && ING_SRC_YUV444P == PSXHIP_SRC_YUV444P && ING_SRC_NV21 == PSXHIP_SRC_NV21 &&
              ING_SRC_UYVY422 == PSXHIP_SRC_UYVY422 && ING_SRC_YUV444P10 == PSXHIP_SRC_YUV444P10 && ING_SRC_P010 == PSXHIP_SRC_P010 &&
              ING_SRC_GRAY8 == PSXHIP_SRC_GRAY8 && ING_SRC_RGB24 == PSXHIP_SRC_RGB24 && ING_SRC_BGRA32 == PSXHIP_SRC_BGRA32,
              "ingest_core.h restates the source formats");
static_assert(ING_OUT_RGB24 == PSXHIP_PIX_RGB24 && ING_OUT_YUV420P == PSXHIP_PIX_YUV420P && ING_CHROMA_BILINEAR == PSXHIP_INGEST_CHROMA_BILINEAR,
              "ingest_core.h restates the outputs and the options");

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

int bad(const char* who, const char* what) {
    psxhip_set_error("%s: %s", who, what);
    return PSXHIP_EINVAL;
}

}  // namespace

struct psxhip_ingest {
    int device, out_format;
    IngestDesc d;
    size_t src_bytes;       // from the picture's first byte to the end of its last plane
    size_t out_bytes;
};

extern "C" const char* psxhip_ingest_kernel_rev(void) { return PSXHIP_INGEST_KERNEL_REV; }

extern "C" void psxhip_ingest_destroy(psxhip_ingest_t* g) { delete g; }

extern "C" int psxhip_ingest_create(psxhip_ingest_t** out, int device, int src_format, int width, int height,
                                    const psxhip_ingest_plane_t* planes, int n_planes, int matrix, int full_range, int out_format,
                                    uint32_t options) {
    const char* who = "psxhip_ingest_create";
    if (!out) return bad(who, "NULL argument");
    *out = nullptr;
    if (!planes) return bad(who, "NULL argument");
    IngestDesc d = {};
    d.f = ingest_format(src_format);
    if (d.f.layout < 0) return bad(who, "unknown source format");
    if (n_planes != d.f.planes) {
        psxhip_set_error("%s: source format %d has %d planes, %d given", who, src_format, d.f.planes, n_planes);
        return PSXHIP_EINVAL;
    }
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return bad(who, "width and height are 1 .. 16384");
    if (d.f.layout == ING_PACKED422 && (width & 1)) return bad(who, "a packed 4:2:2 source has an even width");
    if (options & ~(uint32_t)PSXHIP_INGEST_CHROMA_BILINEAR) return bad(who, "unknown option bit");
    const bool yuv = yuv_or_grey(d.f);
    if (yuv && (matrix < 0 || matrix > PSXHIP_MATRIX_BT2020_NCL)) return bad(who, "unknown matrix");
    if (out_format != PSXHIP_PIX_RGB24 && out_format != PSXHIP_PIX_YUV420P) return bad(who, "out_format is PSXHIP_PIX_RGB24 or PSXHIP_PIX_YUV420P");
    if (out_format == PSXHIP_PIX_YUV420P) {
        if (!yuv) return bad(who, "PSXHIP_PIX_YUV420P output takes a YUV or grey source, not packed RGB");
        if (matrix != PSXHIP_MATRIX_BT601) return bad(who, "PSXHIP_PIX_YUV420P output copies the samples, which the scaler reads as BT.601: another matrix needs PSXHIP_PIX_RGB24");
        if ((width | height) & 1) return bad(who, "PSXHIP_PIX_YUV420P output needs an even width and height");
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
    psxhip_ingest* g = new (std::nothrow) psxhip_ingest;
    if (!g) return PSXHIP_ENOMEM;
    g->device = device; g->out_format = out_format; g->d = d; g->src_bytes = extent;
    g->out_bytes = out_format == PSXHIP_PIX_RGB24 ? (size_t)width * height * 3 : (size_t)width * height * 3 / 2;
    *out = g;
    return PSXHIP_OK;
}

extern "C" size_t psxhip_ingest_output_bytes(const psxhip_ingest_t* g) { return g ? g->out_bytes : 0; }
extern "C" size_t psxhip_ingest_source_bytes(const psxhip_ingest_t* g) { return g ? g->src_bytes : 0; }

extern "C" int psxhip_ingest_matrix(const psxhip_ingest_t* g, int32_t out[7]) {
    if (!g || !out) return bad("psxhip_ingest_matrix", "NULL argument");
    const IngestDesc& d = g->d;
    const int32_t m[7] = {d.cy, d.rv, d.gu, d.gv, d.bu, d.yoff, d.coff};
    for (int i = 0; i < 7; i++) out[i] = m[i];
    return PSXHIP_OK;
}

// the argument rules of a conversion, which need no device; *go: there is something to do
static int ingest_check(const char* who, const psxhip_ingest_t* g, const uint8_t* src, size_t src_stride, int n_src, int n_out,
                        const uint8_t* dst, size_t out_stride, bool device_pointers, bool* go) {
    *go = false;
    if (!g) return bad(who, "NULL argument");
    if (n_src < 0 || n_out < 0) return bad(who, "negative picture count");
    if (n_out == 0) return PSXHIP_OK;
    if (!src || !dst || n_src == 0) return bad(who, "NULL argument, or output pictures without source pictures");
    if (src_stride < g->src_bytes || out_stride < g->out_bytes) {
        psxhip_set_error("%s: strides too small: src_stride %zu below the picture's %zu bytes, or out_stride %zu below %zu", who, src_stride,
                         g->src_bytes, out_stride, g->out_bytes);
        return PSXHIP_EINVAL;
    }
    if (g->d.f.bytes == 2 && ((src_stride & 1) || (device_pointers && ((uintptr_t)src & 1)))) return bad(who, "a 16-bit format needs an even source address and src_stride");
    if (device_pointers) {
        const uintptr_t s = (uintptr_t)src, s_end = s + (size_t)(n_src - 1) * src_stride + g->src_bytes;
        const uintptr_t o = (uintptr_t)dst, o_end = o + (size_t)(n_out - 1) * out_stride + g->out_bytes;
        if (s < o_end && o < s_end) return bad(who, "d_out overlaps d_src");
    }
    *go = true;
    return PSXHIP_OK;
}

static psxhip_ingest_job_t job_of(const psxhip_ingest_t* g, const uint8_t* d_src, size_t src_stride, int n_src, const int32_t* d_src_index,
                                  int n_out, uint8_t* d_out, size_t out_stride) {
    psxhip_ingest_job_t j;
    j.d = g->d; j.d_src = d_src; j.src_stride = src_stride; j.n_src = n_src; j.d_src_index = d_src_index; j.first = 0; j.n_out = n_out;
    j.d_out = d_out; j.out_stride = out_stride; j.out_format = g->out_format;
    return j;
}

// (no temporary memory: the kernel reads the caller's pictures and index and writes the caller's output)
extern "C" int psxhip_ingest_convert_device(psxhip_ingest_t* g, const uint8_t* d_src, size_t src_stride, int n_src, const int32_t* d_src_index,
                                            int n_out, uint8_t* d_out, size_t out_stride, void* stream) {
    bool go;
    int rc = ingest_check("psxhip_ingest_convert_device", g, d_src, src_stride, n_src, n_out, d_out, out_stride, true, &go);
    if (rc || !go) return rc;
    if ((rc = psxhip_ensure_device(g->device))) return rc;
    HIP_TRY(hipSetDevice(g->device), PSXHIP_EDEVICE);
    const psxhip_ingest_job_t j = job_of(g, d_src, src_stride, n_src, d_src_index, n_out, d_out, out_stride);
    HIP_TRY(psxhip_ingest_launch(&j, stream), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_ingest_convert_host(psxhip_ingest_t* g, const uint8_t* src, size_t src_stride, int n_src, const int32_t* src_index,
                                          int n_out, uint8_t* out, size_t out_stride) {
    bool go;
    int rc = ingest_check("psxhip_ingest_convert_host", g, src, src_stride, n_src, n_out, out, out_stride, false, &go);
    if (rc || !go) return rc;
    if ((rc = psxhip_ensure_device(g->device))) return rc;
    HIP_TRY(hipSetDevice(g->device), PSXHIP_EDEVICE);
    const size_t src_bytes = (size_t)(n_src - 1) * src_stride + g->src_bytes, out_bytes = (size_t)(n_out - 1) * out_stride + g->out_bytes;
    DeviceBuffer d_src, d_out, d_index;                  // a call's temporaries
    if ((rc = d_src.reserve(src_bytes)) || (rc = d_out.reserve(out_bytes)) || (src_index && (rc = d_index.reserve((size_t)n_out * sizeof(int32_t))))) return rc;
    HIP_TRY(hipMemcpy(d_src.p, src, src_bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    // the output goes up as well: what the kernel does not write (between pictures, pictures of negative indices) comes back as it was
    HIP_TRY(hipMemcpy(d_out.p, out, out_bytes, hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    if (src_index) HIP_TRY(hipMemcpy(d_index.p, src_index, (size_t)n_out * sizeof(int32_t), hipMemcpyHostToDevice), PSXHIP_EDEVICE);
    const psxhip_ingest_job_t j = job_of(g, d_src.as<uint8_t>(), src_stride, n_src, src_index ? d_index.as<int32_t>() : nullptr, n_out,
                                         d_out.as<uint8_t>(), out_stride);
    HIP_TRY(psxhip_ingest_launch(&j, nullptr), PSXHIP_EDEVICE);
    HIP_TRY(hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost), PSXHIP_EDEVICE);
    HIP_TRY(hipDeviceSynchronize(), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

// ---- the planners: no device

extern "C" int psxhip_ingest_recommend(int src_format, int matrix, int width, int height) {
    const IngestFormat f = ingest_format(src_format);
    if (f.layout < 0 || width < 1 || height < 1) return bad("psxhip_ingest_recommend", "unknown source format, or an empty picture");
    return may_be_yuv420p(f, matrix, width, height) ? PSXHIP_PIX_YUV420P : PSXHIP_PIX_RGB24;
}

// psxavenc/decoding.c:275-285, in its own double-precision expressions
extern "C" int psxhip_ingest_fit(int src_w, int src_h, int max_w, int max_h, int ignore_aspect, int* dst_w, int* dst_h) {
    const char* who = "psxhip_ingest_fit";
    if (!dst_w || !dst_h) return bad(who, "NULL argument");
    if (src_w < 1 || src_h < 1 || max_w < 16 || max_h < 16 || max_w > 1024 || max_h > 1024 || (max_w & 15) || (max_h & 15))
        return bad(who, "the source is empty, or the maximum is not a multiple of 16 in 16 .. 1024");
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
        return bad(who, "NULL argument, a negative count, or a time base or frame rate that is not positive");
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
        if (gap > 1e9) return bad(who, "a gap of more than 10^9 frames");
        for (int dupes = gap > 0 ? (int)gap : 0; dupes; dupes--) {
            if (count < cap) out_index[count] = last;
            count++;
            next += step;
        }
        if (count < cap) out_index[count] = i;
        count++;
        last = i;
        if (count > 0x7fffffff) return bad(who, "more than 2^31 - 1 output frames");
    }
    return (int)count;
}
