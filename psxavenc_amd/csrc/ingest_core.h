// ingest_core.h -- "psxhip ingest v1" for one sample: a decoder's picture -> the scaler's RGB24 or YUV420P.
// Plain C++ for host and device, and it includes nothing but <stdint.h>: the kernels (ingest_kernels.hip) call these functions on
// samples they have loaded, and the CPU program of tests/test_ingest_core_cpu.py (tests/cpu/ingest_sim.cpp) runs ingest_pixel(),
// which computes one output sample from a picture in memory without any sharing.  The statement both are held to is
// tests/ingest_ref.py, written independently.  Integers only; >> is arithmetic.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ING_FN __host__ __device__ inline __attribute__((always_inline))      /* (__forceinline__, spelt out: hip_runtime.h need not be included first) */
#else
#define ING_FN static inline
#endif

// src_format, out_format and options of include/psxav_hip.h, restated so that this file includes nothing
enum {
    ING_SRC_YUV420P = 0, ING_SRC_YUV422P, ING_SRC_YUV444P, ING_SRC_NV12, ING_SRC_NV21, ING_SRC_YUYV422, ING_SRC_UYVY422,
    ING_SRC_YUV420P10, ING_SRC_YUV422P10, ING_SRC_YUV444P10, ING_SRC_P010, ING_SRC_GRAY8,
    ING_SRC_RGB24, ING_SRC_BGR24, ING_SRC_RGBA32, ING_SRC_BGRA32, ING_SRC_COUNT
};
enum { ING_OUT_RGB24 = 0, ING_OUT_YUV420P = 1 };
enum { ING_CHROMA_BILINEAR = 1 };
// how the samples lie in memory: three planes; a luma plane and one of Cb Cr pairs; one plane of Y Cb Y Cr; luma alone; R G B (X)
enum { ING_PLANAR = 0, ING_SEMI = 1, ING_PACKED422 = 2, ING_GRAY = 3, ING_RGB = 4 };

struct IngestFormat {
    int layout;        // ING_PLANAR ..
    int bytes;         // of a sample: 1, or 2 (a little-endian word, the value (word >> shift) & 1023)
    int subx, suby;    // 1: chroma has half the columns / rows (rounded up)
    int shift;
    int swap;          // semi-planar: Cr first; packed 4:2:2: chroma first (UYVY); RGB: B first
    int px_bytes;      // ING_RGB: 3 or 4
    int planes;
};
ING_FN IngestFormat ingest_format(int f) {
    IngestFormat o = {-1, 1, 0, 0, 0, 0, 0, 0};
    switch (f) {
    case ING_SRC_YUV420P: o.layout = ING_PLANAR; o.subx = 1; o.suby = 1; o.planes = 3; break;
    case ING_SRC_YUV422P: o.layout = ING_PLANAR; o.subx = 1; o.planes = 3; break;
    case ING_SRC_YUV444P: o.layout = ING_PLANAR; o.planes = 3; break;
    case ING_SRC_NV12: o.layout = ING_SEMI; o.subx = 1; o.suby = 1; o.planes = 2; break;
    case ING_SRC_NV21: o.layout = ING_SEMI; o.subx = 1; o.suby = 1; o.swap = 1; o.planes = 2; break;
    case ING_SRC_YUYV422: o.layout = ING_PACKED422; o.subx = 1; o.planes = 1; break;
    case ING_SRC_UYVY422: o.layout = ING_PACKED422; o.subx = 1; o.swap = 1; o.planes = 1; break;
    case ING_SRC_YUV420P10: o.layout = ING_PLANAR; o.bytes = 2; o.subx = 1; o.suby = 1; o.planes = 3; break;
    case ING_SRC_YUV422P10: o.layout = ING_PLANAR; o.bytes = 2; o.subx = 1; o.planes = 3; break;
    case ING_SRC_YUV444P10: o.layout = ING_PLANAR; o.bytes = 2; o.planes = 3; break;
    case ING_SRC_P010: o.layout = ING_SEMI; o.bytes = 2; o.subx = 1; o.suby = 1; o.shift = 6; o.planes = 2; break;
    case ING_SRC_GRAY8: o.layout = ING_GRAY; o.planes = 1; break;
    case ING_SRC_RGB24: o.layout = ING_RGB; o.px_bytes = 3; o.planes = 1; break;
    case ING_SRC_BGR24: o.layout = ING_RGB; o.px_bytes = 3; o.swap = 1; o.planes = 1; break;
    case ING_SRC_RGBA32: o.layout = ING_RGB; o.px_bytes = 4; o.planes = 1; break;
    case ING_SRC_BGRA32: o.layout = ING_RGB; o.px_bytes = 4; o.swap = 1; o.planes = 1; break;
    default: break;
    }
    return o;
}

// a checked source and its conversion: what psxhip_ingest_create keeps and the kernels take by value
struct IngestDesc {
    IngestFormat f;
    int w, h;
    uint32_t off[3], pitch[3];             // of each plane, in bytes
    int cy, rv, gu, gv, bu, yoff, coff;    // the matrix (psxhip_ingest_matrix's seven numbers)
    int bilinear;
};

ING_FN int ing_clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
ING_FN int ing_chroma_cols(const IngestDesc& d) { return d.f.subx ? (d.w + 1) >> 1 : d.w; }
ING_FN int ing_chroma_rows(const IngestDesc& d) { return d.f.suby ? (d.h + 1) >> 1 : d.h; }
// bytes a row of plane p holds
ING_FN uint32_t ing_row_bytes(const IngestDesc& d, int p) {
    const uint32_t w = (uint32_t)d.w, cw = (uint32_t)ing_chroma_cols(d);
    switch (d.f.layout) {
    case ING_PLANAR: return (p == 0 ? w : cw) * (uint32_t)d.f.bytes;
    case ING_SEMI: return (p == 0 ? w : 2 * cw) * (uint32_t)d.f.bytes;
    case ING_PACKED422: return 2 * w;
    case ING_GRAY: return w;
    default: return w * (uint32_t)d.f.px_bytes;
    }
}
ING_FN int ing_plane_rows(const IngestDesc& d, int p) { return p == 0 ? d.h : ing_chroma_rows(d); }

// ---- sample fetch by format.  value_of(): a sample from its 8 or 16 bits
ING_FN int ing_value(int raw, int shift) { return (raw >> shift) & 1023; }
ING_FN int ing_sample(const uint8_t* p, const IngestFormat& f) {
    return f.bytes == 1 ? (int)p[0] : ing_value((int)p[0] | ((int)p[1] << 8), f.shift);
}
ING_FN int ingest_luma(const IngestDesc& d, const uint8_t* pic, int x, int y) {
    const uint8_t* row = pic + d.off[0] + (size_t)y * d.pitch[0];
    if (d.f.layout == ING_PACKED422) return row[2 * x + d.f.swap];
    return ing_sample(row + (size_t)x * d.f.bytes, d.f);
}
// c: 0 Cb, 1 Cr; (cx, cy) on the chroma grid
ING_FN int ingest_chroma(const IngestDesc& d, const uint8_t* pic, int c, int cx, int cy) {
    if (d.f.layout == ING_PLANAR) return ing_sample(pic + d.off[1 + c] + (size_t)cy * d.pitch[1 + c] + (size_t)cx * d.f.bytes, d.f);
    if (d.f.layout == ING_SEMI) return ing_sample(pic + d.off[1] + (size_t)cy * d.pitch[1] + (size_t)(2 * cx + (c ^ d.f.swap)) * d.f.bytes, d.f);
    return (pic + d.off[0] + (size_t)cy * d.pitch[0])[4 * cx + 2 * c + 1 - d.f.swap];        // Y Cb Y Cr, or Cb Y Cr Y
}

// ---- chroma to the luma grid.  The far sample's index along one axis: the neighbour on the pixel's own side, clamped to the plane
ING_FN int ing_far(int p, int n_samples) {
    const int k = p >> 1, f = (p & 1) ? k + 1 : k - 1;
    return f < 0 ? 0 : (f > n_samples - 1 ? n_samples - 1 : f);
}
// 4:2:0: (9 near + 3 far_x + 3 far_y + far_xy + 8) >> 4 as 3 (3 k + f) + (3 k' + f'), rounded once; 4:2:2: (3 near + far + 2) >> 2
ING_FN int ing_hmix(int near, int far) { return 3 * near + far; }
ING_FN int ing_vsum(int near_row, int far_row) { return 3 * near_row + far_row; }
ING_FN int ing_vround(int sum) { return (sum + 8) >> 4; }
ING_FN int ing_vmix(int near_row, int far_row) { return ing_vround(ing_vsum(near_row, far_row)); }
ING_FN int ing_hmix422(int near, int far) { return (3 * near + far + 2) >> 2; }
ING_FN int ingest_chroma_at(const IngestDesc& d, const uint8_t* pic, int c, int x, int y) {
    const int kx = d.f.subx ? x >> 1 : x, ky = d.f.suby ? y >> 1 : y;
    if (!d.bilinear || !d.f.subx) return ingest_chroma(d, pic, c, kx, ky);
    const int fx = ing_far(x, ing_chroma_cols(d));
    if (!d.f.suby) return ing_hmix422(ingest_chroma(d, pic, c, kx, ky), ingest_chroma(d, pic, c, fx, ky));
    const int fy = ing_far(y, ing_chroma_rows(d));
    return ing_vmix(ing_hmix(ingest_chroma(d, pic, c, kx, ky), ingest_chroma(d, pic, c, fx, ky)),
                    ing_hmix(ingest_chroma(d, pic, c, kx, fy), ingest_chroma(d, pic, c, fx, fy)));
}

// ---- matrix to bytes: out = clamp((cy (Y - yoff) + cu (Cb - coff) + cv (Cr - coff) + 32768) >> 16, 0, 255); |sum| < 2^26
struct IngRgb {
    int r, g, b;
};
ING_FN IngRgb ing_matrix(const IngestDesc& d, int y, int cb, int cr) {
    const int base = d.cy * (y - d.yoff) + 32768, u = cb - d.coff, v = cr - d.coff;
    IngRgb o;
    o.r = ing_clamp255((base + d.rv * v) >> 16);
    o.g = ing_clamp255((base + d.gu * u + d.gv * v) >> 16);
    o.b = ing_clamp255((base + d.bu * u) >> 16);
    return o;
}
ING_FN int ing_grey(const IngestDesc& d, int y) { return ing_clamp255((d.cy * (y - d.yoff) + 32768) >> 16); }

// ---- the YUV420P output: depth reduction and the box average in one rounding.  sum of 1 << log2n samples of `bytes` bytes
ING_FN int ing_box(int sum, int log2n, int bytes) {
    const int s = log2n + (bytes == 2 ? 2 : 0);
    const int v = s ? (sum + (1 << (s - 1))) >> s : sum;
    return v > 255 ? 255 : v;
}

// ---- one pixel / one sample of a picture in memory, by the steps above
ING_FN IngRgb ingest_rgb(const IngestDesc& d, const uint8_t* pic, int x, int y) {
    IngRgb o;
    if (d.f.layout == ING_RGB) {
        const uint8_t* p = pic + d.off[0] + (size_t)y * d.pitch[0] + (size_t)x * d.f.px_bytes;
        o.r = p[d.f.swap ? 2 : 0]; o.g = p[1]; o.b = p[d.f.swap ? 0 : 2];
        return o;
    }
    const int l = ingest_luma(d, pic, x, y);
    if (d.f.layout == ING_GRAY) {
        o.r = o.g = o.b = ing_grey(d, l);
        return o;
    }
    return ing_matrix(d, l, ingest_chroma_at(d, pic, 0, x, y), ingest_chroma_at(d, pic, 1, x, y));
}
// plane: 0 Y at (x, y) of w x h; 1 Cb, 2 Cr at (x, y) of w / 2 x h / 2
ING_FN int ingest_yuv(const IngestDesc& d, const uint8_t* pic, int plane, int x, int y) {
    if (plane == 0) return ing_box(ingest_luma(d, pic, x, y), 0, d.f.bytes);
    if (d.f.layout == ING_GRAY) return 128;
    const int nx = d.f.subx ? 1 : 2, ny = d.f.suby ? 1 : 2;
    int sum = 0;
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) sum += ingest_chroma(d, pic, plane - 1, nx * x + i, ny * y + j);
    return ing_box(sum, (nx >> 1) + (ny >> 1), d.f.bytes);
}
// comp: the channel (0 R, 1 G, 2 B) of pixel (x, y), or the plane of sample (x, y)
ING_FN int ingest_pixel(const IngestDesc& d, const uint8_t* pic, int out_format, int comp, int x, int y) {
    if (out_format == ING_OUT_YUV420P) return ingest_yuv(d, pic, comp, x, y);
    const IngRgb c = ingest_rgb(d, pic, x, y);
    return comp == 0 ? c.r : (comp == 1 ? c.g : c.b);
}
