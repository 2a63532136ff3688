// ingest_kernels.hip -- the picture ingest's kernel for gfx950: a decoder's pictures -> the scaler's RGB24 or YUV420P ("psxhip ingest
// v1"; the arithmetic of one sample is ingest_core.h, the text the CPU test runs).
//
// The conversion streams: 1 .. 4 bytes read and 1.5 or 3 written per pixel, a handful of integer operations in between, so the kernel
// is shaped by its memory accesses.  A lane owns a run of 8 x 2 pixels: eight horizontally adjacent pixels of two rows, which share
// their chroma samples in every subsampled format, so each source byte is loaded once.  Of every plane it fetches the run's bytes of
// a row in one access -- 4 bytes of 8-bit 4:2:0 chroma, 8 of 8-bit luma, 16 of a 10-bit or packed row, 24 or 32 of RGB -- as whole
// dwords when the address is 4-byte aligned and the run lies inside the row, else byte by byte (unaligned plane offsets and pitches,
// the ragged right edge).  It stores the same way: six dwords a row of RGB24; two a row of luma and one of each chroma plane for
// YUV420P; bytes where a packed row of an odd-sized picture starts off a dword or ends inside one.  Consecutive lanes take consecutive
// addresses along a row, so a wavefront's accesses are contiguous runs.  Bilinear chroma needs the chroma rows above and below and
// one sample left and right of the run: extra loads of cache lines the lane's neighbours fetch anyway (no cross-lane exchange: a
// neighbour in x may sit in another wavefront, and the plane's edges clamp).
//
// The kernel is a template on the layout class (planar 4:4:4 / 4:2:2 / 4:2:0, semi-planar, packed 4:2:2, grey, packed RGB), the sample
// depth (for packed RGB: the pixel's bytes) and the output mode (RGB24 with replicated chroma, RGB24 with bilinear chroma, YUV420P):
// 29 instantiations, not one per format; the order of a pair (NV12 / NV21, YUYV / UYVY, RGB / BGR), the shift of a 16-bit word and
// the matrix are kernel arguments, the same in every lane.  No branch depends on a pixel.  No LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ingest_core.h"
#include "psxhip_ingest_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxPicturesPerLaunch = 65535;                   // gridDim.y
constexpr int kRun = 8;                                        // pixels of a row a lane owns
enum { SUB444 = 0, SUB422 = 1, SUB420 = 2 };
enum { MODE_RGB = 0, MODE_RGB_BILINEAR = 1, MODE_YUV = 2 };

template <int NB>
struct Run {                                                   // NB bytes of a row (alignment 4: a row starts on a dword, not more)
    uint32_t v[NB / 4];
};

// NB bytes from p on, of which the first `valid` exist: whole dwords where p allows it, else bytes (those that do not exist read 0)
template <int NB>
__device__ __forceinline__ Run<NB> fetch(const uint8_t* p, int valid) {
    Run<NB> r;
    if (valid >= NB && !((uintptr_t)p & 3)) {
        r = *(const Run<NB>*)p;
    } else {
#pragma unroll
        for (int i = 0; i < NB / 4; i++) {
            uint32_t w = 0;
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (4 * i + b < valid) w |= (uint32_t)p[4 * i + b] << (8 * b);
            r.v[i] = w;
        }
    }
    return r;
}
// the first `valid` of 4 ND bytes to p on: whole dwords where p allows it, else bytes
template <int ND>
__device__ __forceinline__ void store(uint8_t* p, const Run<4 * ND>& r, int valid) {
    if (valid >= 4 * ND && !((uintptr_t)p & 3)) {
        *(Run<4 * ND>*)p = r;
    } else {
#pragma unroll
        for (int k = 0; k < 4 * ND; k++)
            if (k < valid) p[k] = (uint8_t)(r.v[k >> 2] >> (8 * (k & 3)));
    }
}

// sample i (a constant once unrolled) of a fetched run
template <int BPS, int NB>
__device__ __forceinline__ int sample_at(const Run<NB>& r, int i, int shift) {
    if (BPS == 1) return (int)((r.v[i >> 2] >> (8 * (i & 3))) & 255u);
    return ing_value((int)((r.v[i >> 1] >> (16 * (i & 1))) & 0xffffu), shift);
}

// b0 | b1 << 8 | b2 << 16 | b3 << 24 of four values in 0 .. 255, by two byte permutes and an or, as display_kernels.hip packs them
// and for its reason: shifts and ors of clamped values become one v_ashr_pk_u8_i32, whose upper half an MI355X leaves dirty
// (tests/test_ingest_resources.py keeps the instruction out of this file's code).
__device__ __forceinline__ uint32_t pack4(int b0, int b1, int b2, int b3) {
    const uint32_t lo = __builtin_amdgcn_perm((uint32_t)b1, (uint32_t)b0, 0x0c0c0400u);      // bytes b0, b1, 0, 0
    const uint32_t hi = __builtin_amdgcn_perm((uint32_t)b3, (uint32_t)b2, 0x04000c0cu);      // bytes 0, 0, b2, b3
    return lo | hi;
}

// the run's eight luma samples of row y
template <int LAYOUT, int BPS>
__device__ __forceinline__ void load_luma(const IngestDesc& d, const uint8_t* pic, int x0, int y, int npx, int (&Y)[kRun]) {
    const uint8_t* row = pic + d.off[0] + (size_t)y * d.pitch[0];
    if (LAYOUT == ING_PACKED422) {
        const Run<2 * kRun> r = fetch<2 * kRun>(row + 2 * x0, 2 * npx);
#pragma unroll
        for (int i = 0; i < kRun / 2; i++) {
            const uint32_t w = d.f.swap ? r.v[i] >> 8 : r.v[i];            // Y . Y .
            Y[2 * i] = (int)(w & 255u);
            Y[2 * i + 1] = (int)((w >> 16) & 255u);
        }
    } else {
        const Run<BPS * kRun> r = fetch<BPS * kRun>(row + (size_t)x0 * BPS, BPS * npx);
#pragma unroll
        for (int i = 0; i < kRun; i++) Y[i] = sample_at<BPS>(r, i, d.f.shift);
    }
}

// NCS chroma samples of both channels from column cx0 of chroma row cy on, of which the first n exist.  EDGE: those that do not
// exist repeat the last one that does (the bilinear mix's clamp to the plane)
template <int LAYOUT, int BPS, int NCS, bool EDGE>
__device__ __forceinline__ void load_chroma(const IngestDesc& d, const uint8_t* pic, int cx0, int cy, int n, int (&cb)[NCS], int (&cr)[NCS]) {
    if (LAYOUT == ING_PLANAR) {
        const Run<BPS * NCS> a = fetch<BPS * NCS>(pic + d.off[1] + (size_t)cy * d.pitch[1] + (size_t)cx0 * BPS, BPS * n);
        const Run<BPS * NCS> b = fetch<BPS * NCS>(pic + d.off[2] + (size_t)cy * d.pitch[2] + (size_t)cx0 * BPS, BPS * n);
#pragma unroll
        for (int i = 0; i < NCS; i++) {
            cb[i] = sample_at<BPS>(a, i, d.f.shift);
            cr[i] = sample_at<BPS>(b, i, d.f.shift);
        }
    } else if (LAYOUT == ING_SEMI) {
        const Run<2 * BPS * NCS> a = fetch<2 * BPS * NCS>(pic + d.off[1] + (size_t)cy * d.pitch[1] + (size_t)cx0 * (2 * BPS), 2 * BPS * n);
#pragma unroll
        for (int i = 0; i < NCS; i++) {
            const int first = sample_at<BPS>(a, 2 * i, d.f.shift), second = sample_at<BPS>(a, 2 * i + 1, d.f.shift);
            cb[i] = d.f.swap ? second : first;
            cr[i] = d.f.swap ? first : second;
        }
    } else {                                                               // ING_PACKED422: a dword is Y Cb Y Cr or Cb Y Cr Y
        const Run<4 * NCS> a = fetch<4 * NCS>(pic + d.off[0] + (size_t)cy * d.pitch[0] + (size_t)cx0 * 4, 4 * n);
#pragma unroll
        for (int i = 0; i < NCS; i++) {
            const uint32_t w = d.f.swap ? a.v[i] : a.v[i] >> 8;            // Cb . Cr .
            cb[i] = (int)(w & 255u);
            cr[i] = (int)((w >> 16) & 255u);
        }
    }
    if (EDGE) {
#pragma unroll
        for (int i = 1; i < NCS; i++)
            if (i >= n) {
                cb[i] = cb[i - 1];
                cr[i] = cr[i - 1];
            }
    }
}

// one chroma sample (c: 0 Cb, 1 Cr) at (cx, cy) of the chroma grid: ingest_chroma() with the layout known (through its switch on
// the layout at run time the bilinear kernels took 66 .. 74 registers instead of 50 .. 54)
template <int LAYOUT, int BPS>
__device__ __forceinline__ int chroma_sample(const IngestDesc& d, const uint8_t* pic, int c, int cx, int cy) {
    const uint8_t* p;
    if (LAYOUT == ING_PLANAR) p = pic + d.off[1 + c] + (size_t)cy * d.pitch[1 + c] + (size_t)cx * BPS;
    else if (LAYOUT == ING_SEMI) p = pic + d.off[1] + (size_t)cy * d.pitch[1] + (size_t)(2 * cx + (c ^ d.f.swap)) * BPS;
    else return (pic + d.off[0] + (size_t)cy * d.pitch[0])[4 * cx + 2 * c + 1 - d.f.swap];
    return BPS == 1 ? (int)p[0] : ing_value((int)*(const uint16_t*)p, d.f.shift);
}

// the near and the far sample of pixel i of the run (4 samples, and the ones left and right of them)
__device__ __forceinline__ int near_of(const int (&c)[kRun / 2], int i) { return c[i >> 1]; }
__device__ __forceinline__ int far_of(const int (&c)[kRun / 2], int left, int right, int i) {
    const int k = i >> 1;
    return (i & 1) ? (k == kRun / 2 - 1 ? right : c[k + 1 < kRun / 2 ? k + 1 : k]) : (k == 0 ? left : c[k > 0 ? k - 1 : 0]);
}
// ing_hmix() of chroma row cy for the run's eight pixels, Cb in the low and Cr in the high half of a register: a mix of 10-bit samples
// stays below 2^16 (3 * 1023 + 1023, and ing_vsum() of two of them 16 * 1023), so one multiply-add serves both channels and the
// sixteen mixes of a row take eight registers
template <int LAYOUT, int BPS>
__device__ __forceinline__ void chroma_hmix(const IngestDesc& d, const uint8_t* pic, int cx0, int cy, int n, int (&h)[kRun]) {
    int cb[kRun / 2], cr[kRun / 2], c[kRun / 2];
    load_chroma<LAYOUT, BPS, kRun / 2, true>(d, pic, cx0, cy, n, cb, cr);
    const int cw = ing_chroma_cols(d), lx = cx0 > 0 ? cx0 - 1 : 0, rx = cx0 + kRun / 2 < cw ? cx0 + kRun / 2 : cw - 1;
    const int left = chroma_sample<LAYOUT, BPS>(d, pic, 0, lx, cy) | (chroma_sample<LAYOUT, BPS>(d, pic, 1, lx, cy) << 16);
    const int right = chroma_sample<LAYOUT, BPS>(d, pic, 0, rx, cy) | (chroma_sample<LAYOUT, BPS>(d, pic, 1, rx, cy) << 16);
#pragma unroll
    for (int i = 0; i < kRun / 2; i++) c[i] = cb[i] | (cr[i] << 16);
#pragma unroll
    for (int i = 0; i < kRun; i++) h[i] = ing_hmix(near_of(c, i), far_of(c, left, right, i));
}

// eight RGB pixels to row y of the output picture
__device__ __forceinline__ void store_rgb(const IngestDesc& d, uint8_t* out, int x0, int y, int npx, const IngRgb (&p)[kRun]) {
    Run<3 * kRun> r;
#pragma unroll
    for (int q = 0; q < kRun / 4; q++) {                                   // four pixels are three dwords
        const IngRgb *a = &p[4 * q];
        r.v[3 * q] = pack4(a[0].r, a[0].g, a[0].b, a[1].r);
        r.v[3 * q + 1] = pack4(a[1].g, a[1].b, a[2].r, a[2].g);
        r.v[3 * q + 2] = pack4(a[2].b, a[3].r, a[3].g, a[3].b);
    }
    store<3 * kRun / 4>(out + ((size_t)y * d.w + x0) * 3, r, 3 * npx);
}

template <int LAYOUT, int SUB, int BPS, int MODE>
__global__ __launch_bounds__(kThreads) void ingest_convert_kernel(const psxhip_ingest_job_t j) {
    constexpr bool SUBX = SUB != SUB444, SUBY = SUB == SUB420;
    constexpr int NCS = SUBX ? kRun / 2 : kRun;                           // chroma samples under the run
    const IngestDesc& d = j.d;
    const int i = j.first + (int)blockIdx.y;
    const int idx = j.d_src_index ? j.d_src_index[i] : i;
    if (idx < 0 || idx >= j.n_src) return;                                // the output picture keeps its contents
    const int uw = (d.w + kRun - 1) / kRun, uh = (d.h + 1) >> 1;
    const int u = (int)(blockIdx.x * (unsigned)kThreads + threadIdx.x);
    if (u >= uw * uh) return;
    const int uy = u / uw, ux = u - uy * uw;
    const int x0 = ux * kRun, y0 = 2 * uy, npx = d.w - x0 < kRun ? d.w - x0 : kRun;
    const bool two_rows = y0 + 1 < d.h;                                   // (an odd height: RGB24 output only)
    const int y1 = two_rows ? y0 + 1 : y0;
    const uint8_t* pic = j.d_src + (size_t)idx * j.src_stride;
    uint8_t* out = j.d_out + (size_t)i * j.out_stride;

    if (LAYOUT == ING_RGB) {                                              // BPS: the bytes of a pixel
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int y = r ? y1 : y0;
            const Run<BPS * kRun> s = fetch<BPS * kRun>(pic + d.off[0] + (size_t)y * d.pitch[0] + (size_t)x0 * BPS, BPS * npx);
            IngRgb p[kRun];
#pragma unroll
            for (int k = 0; k < kRun; k++) {
                const int a = sample_at<1>(s, BPS * k, 0), c = sample_at<1>(s, BPS * k + 2, 0);
                p[k].r = d.f.swap ? c : a;
                p[k].g = sample_at<1>(s, BPS * k + 1, 0);
                p[k].b = d.f.swap ? a : c;
            }
            if (r == 0 || two_rows) store_rgb(d, out, x0, y, npx, p);
        }
        return;
    }

    int Y[kRun];                                                          // of the row at hand
    const int cx0 = SUBX ? x0 >> 1 : x0, ncs = SUBX ? (npx + 1) >> 1 : npx;

    if (MODE == MODE_YUV) {                                               // width and height are even
        const size_t w = (size_t)d.w, plane = w * (size_t)d.h;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            Run<kRun> l;
            load_luma<LAYOUT, BPS>(d, pic, x0, y0 + r, npx, Y);
#pragma unroll
            for (int q = 0; q < kRun / 4; q++)
                l.v[q] = pack4(ing_box(Y[4 * q], 0, BPS), ing_box(Y[4 * q + 1], 0, BPS), ing_box(Y[4 * q + 2], 0, BPS), ing_box(Y[4 * q + 3], 0, BPS));
            store<kRun / 4>(out + (size_t)(y0 + r) * w + x0, l, npx);
        }
        Run<4> cu, cv;
        if (LAYOUT == ING_GRAY) {
            cu.v[0] = cv.v[0] = 0x80808080u;
        } else {
            int sb[NCS], sr[NCS];                                         // the column sums of the one or two chroma rows
            load_chroma<LAYOUT, BPS, NCS, false>(d, pic, cx0, SUBY ? uy : y0, ncs, sb, sr);
            if (!SUBY) {
                int tb[NCS], tr[NCS];
                load_chroma<LAYOUT, BPS, NCS, false>(d, pic, cx0, y1, ncs, tb, tr);
#pragma unroll
                for (int k = 0; k < NCS; k++) {
                    sb[k] += tb[k];
                    sr[k] += tr[k];
                }
            }
            constexpr int NX = SUBX ? 1 : 2, LOG2N = (SUBX ? 0 : 1) + (SUBY ? 0 : 1);
            int ob[kRun / 2], orr[kRun / 2];
#pragma unroll
            for (int k = 0; k < kRun / 2; k++) {
                ob[k] = ing_box(NX == 1 ? sb[k] : sb[(2 * k) % NCS] + sb[(2 * k + 1) % NCS], LOG2N, BPS);
                orr[k] = ing_box(NX == 1 ? sr[k] : sr[(2 * k) % NCS] + sr[(2 * k + 1) % NCS], LOG2N, BPS);
            }
            cu.v[0] = pack4(ob[0], ob[1], ob[2], ob[3]);
            cv.v[0] = pack4(orr[0], orr[1], orr[2], orr[3]);
        }
        uint8_t* pu = out + plane + (size_t)uy * (w >> 1) + (x0 >> 1);
        store<1>(pu, cu, npx >> 1);
        store<1>(pu + (plane >> 2), cv, npx >> 1);
        return;
    }

    IngRgb p[kRun];
    if (LAYOUT == ING_GRAY) {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            load_luma<LAYOUT, BPS>(d, pic, x0, r ? y1 : y0, npx, Y);
#pragma unroll
            for (int k = 0; k < kRun; k++) p[k].r = p[k].g = p[k].b = ing_grey(d, Y[k]);
            if (r == 0 || two_rows) store_rgb(d, out, x0, r ? y1 : y0, npx, p);
        }
    } else if (MODE == MODE_RGB) {                                        // replicated chroma
        int cb[NCS], cr[NCS];
#pragma unroll
        for (int r = 0; r < 2; r++) {
            if (r == 0 || !SUBY) load_chroma<LAYOUT, BPS, NCS, false>(d, pic, cx0, SUBY ? uy : (r ? y1 : y0), ncs, cb, cr);
            load_luma<LAYOUT, BPS>(d, pic, x0, r ? y1 : y0, npx, Y);
#pragma unroll
            for (int k = 0; k < kRun; k++) p[k] = ing_matrix(d, Y[k], cb[SUBX ? k >> 1 : k], cr[SUBX ? k >> 1 : k]);
            if (r == 0 || two_rows) store_rgb(d, out, x0, r ? y1 : y0, npx, p);
        }
    } else if (SUBY) {                                                    // bilinear, 4:2:0: the row above for y0, the one below for y1
        const int ch = ing_chroma_rows(d);
        int m[kRun], f[kRun];                                             // Cb | Cr << 16
        chroma_hmix<LAYOUT, BPS>(d, pic, cx0, uy, ncs, m);
#pragma unroll
        for (int r = 0; r < 2; r++) {
            chroma_hmix<LAYOUT, BPS>(d, pic, cx0, r ? (uy < ch - 1 ? uy + 1 : ch - 1) : (uy > 0 ? uy - 1 : 0), ncs, f);
            load_luma<LAYOUT, BPS>(d, pic, x0, r ? y1 : y0, npx, Y);
#pragma unroll
            for (int k = 0; k < kRun; k++) {
                const int s = ing_vsum(m[k], f[k]);
                p[k] = ing_matrix(d, Y[k], ing_vround(s & 0xffff), ing_vround(s >> 16));
            }
            if (r == 0 || two_rows) store_rgb(d, out, x0, r ? y1 : y0, npx, p);
        }
    } else {                                                              // bilinear, 4:2:2: along the row only
        const int cw = ing_chroma_cols(d), lx = cx0 > 0 ? cx0 - 1 : 0, rx = cx0 + kRun / 2 < cw ? cx0 + kRun / 2 : cw - 1;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int y = r ? y1 : y0;
            int cb[kRun / 2], cr[kRun / 2];
            load_chroma<LAYOUT, BPS, kRun / 2, true>(d, pic, cx0, y, ncs, cb, cr);
            const int lb = chroma_sample<LAYOUT, BPS>(d, pic, 0, lx, y), rb = chroma_sample<LAYOUT, BPS>(d, pic, 0, rx, y);
            const int lr = chroma_sample<LAYOUT, BPS>(d, pic, 1, lx, y), rr = chroma_sample<LAYOUT, BPS>(d, pic, 1, rx, y);
            load_luma<LAYOUT, BPS>(d, pic, x0, y, npx, Y);
#pragma unroll
            for (int k = 0; k < kRun; k++)
                p[k] = ing_matrix(d, Y[k], ing_hmix422(near_of(cb, k), far_of(cb, lb, rb, k)), ing_hmix422(near_of(cr, k), far_of(cr, lr, rr, k)));
            if (r == 0 || two_rows) store_rgb(d, out, x0, y, npx, p);
        }
    }
}

template <int LAYOUT, int SUB, int BPS, int MODE>
void launch(const psxhip_ingest_job_t& j, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((ingest_convert_kernel<LAYOUT, SUB, BPS, MODE>), grid, dim3(kThreads), 0, stream, j);
}
// the three output modes of a YUV source with subsampled chroma
template <int LAYOUT, int SUB, int BPS>
void launch_mode(const psxhip_ingest_job_t& j, int mode, dim3 grid, hipStream_t stream) {
    if (mode == MODE_YUV) launch<LAYOUT, SUB, BPS, MODE_YUV>(j, grid, stream);
    else if (mode == MODE_RGB_BILINEAR) launch<LAYOUT, SUB, BPS, MODE_RGB_BILINEAR>(j, grid, stream);
    else launch<LAYOUT, SUB, BPS, MODE_RGB>(j, grid, stream);
}
// ... and the two of a source whose chroma needs no mix
template <int LAYOUT, int BPS>
void launch_unmixed(const psxhip_ingest_job_t& j, int mode, dim3 grid, hipStream_t stream) {
    if (mode == MODE_YUV) launch<LAYOUT, SUB444, BPS, MODE_YUV>(j, grid, stream);
    else launch<LAYOUT, SUB444, BPS, MODE_RGB>(j, grid, stream);
}
template <int LAYOUT, int SUB>
void launch_depth(const psxhip_ingest_job_t& j, int mode, dim3 grid, hipStream_t stream) {
    if (j.d.f.bytes == 2) launch_mode<LAYOUT, SUB, 2>(j, mode, grid, stream);
    else launch_mode<LAYOUT, SUB, 1>(j, mode, grid, stream);
}

}  // namespace

extern "C" hipError_t psxhip_ingest_launch(const psxhip_ingest_job_t* job, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const IngestFormat& f = job->d.f;
    const int units = ((job->d.w + kRun - 1) / kRun) * ((job->d.h + 1) / 2);
    const int mode = job->out_format == PSXHIP_PIX_YUV420P ? MODE_YUV : ((job->d.bilinear && f.subx) ? MODE_RGB_BILINEAR : MODE_RGB);
    for (int first = 0; first < job->n_out; first += kMaxPicturesPerLaunch) {
        psxhip_ingest_job_t j = *job;
        j.first = first;
        j.n_out = job->n_out - first < kMaxPicturesPerLaunch ? job->n_out - first : kMaxPicturesPerLaunch;
        const dim3 grid((unsigned)((units + kThreads - 1) / kThreads), (unsigned)j.n_out);
        switch (f.layout) {
        case ING_PLANAR:
            if (f.suby) launch_depth<ING_PLANAR, SUB420>(j, mode, grid, stream);
            else if (f.subx) launch_depth<ING_PLANAR, SUB422>(j, mode, grid, stream);
            else if (f.bytes == 2) launch_unmixed<ING_PLANAR, 2>(j, mode, grid, stream);
            else launch_unmixed<ING_PLANAR, 1>(j, mode, grid, stream);
            break;
        case ING_SEMI: launch_depth<ING_SEMI, SUB420>(j, mode, grid, stream); break;
        case ING_PACKED422: launch_mode<ING_PACKED422, SUB422, 1>(j, mode, grid, stream); break;
        case ING_GRAY: launch_unmixed<ING_GRAY, 1>(j, mode, grid, stream); break;
        default:
            if (f.px_bytes == 4) launch<ING_RGB, SUB444, 4, MODE_RGB>(j, grid, stream);
            else launch<ING_RGB, SUB444, 3, MODE_RGB>(j, grid, stream);
            break;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
