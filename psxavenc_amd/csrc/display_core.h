// display_core.h -- "psxhip display v1" for one pixel: NV21 -> RGB24 / RGBX32 / RGB555.  Plain C++ for host and
// device: the kernels (display_kernels.hip) and the CPU program of tests/test_display_core_cpu.py (tests/cpu/display_sim.cpp) run
// this text; the statement it is held to is tests/display_ref.py, written independently.  Integers only; >> is arithmetic.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DISP_FN __host__ __device__ inline __attribute__((always_inline))      /* (__forceinline__, spelt out: hip_runtime.h need not be included first) */
#else
#define DISP_FN static inline
#endif

// out_format and options of include/psxav_hip.h, restated so that this file includes nothing
enum { DISP_RGB24 = 0, DISP_RGBX32 = 1, DISP_RGB555 = 2 };
enum { DISP_CHROMA_BILINEAR = 1, DISP_DITHER = 2, DISP_MASK_BIT = 4 };

DISP_FN int disp_clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

DISP_FN int disp_row_bytes(int out_format, int width) {
    return out_format == DISP_RGB24 ? 3 * width : out_format == DISP_RGBX32 ? 4 * width : out_format == DISP_RGB555 ? 2 * width : 0;
}

// ---- step 1, bilinear: v = (9 c[ky][kx] + 3 c[ky][fx] + 3 c[fy][kx] + c[fy][fx] + 8) >> 4, taken as 3 (3 k + f) + (3 k' + f'): the
// horizontal mix of a chroma row is shared by the pixels above and below it, and nothing is rounded before the one shift
DISP_FN int disp_hmix(int near, int far) { return 3 * near + far; }
DISP_FN int disp_vmix(int near_row, int far_row) { return (3 * near_row + far_row + 8) >> 4; }
// the far sample's index along one axis: the neighbour on the pixel's own side of its chroma sample, clamped to the plane
DISP_FN int disp_far(int p, int n_samples) {
    const int k = p >> 1, f = (p & 1) ? k + 1 : k - 1;
    return f < 0 ? 0 : (f > n_samples - 1 ? n_samples - 1 : f);
}

// ---- step 2: BT.601 full range, the inverse of the front-end's matrix; y, cr, cb are the bytes (0 .. 255).  |sum| <= 31 609 088
struct DispRgb {
    int r, g, b;
};
DISP_FN DispRgb disp_matrix(int y, int cr_byte, int cb_byte) {
    const int cr = cr_byte - 128, cb = cb_byte - 128, base = 65536 * y + 32768;
    DispRgb o;
    o.r = disp_clamp255((base + 91881 * cr) >> 16);
    o.g = disp_clamp255((base - 22553 * cb - 46802 * cr) >> 16);
    o.b = disp_clamp255((base + 116130 * cb) >> 16);
    return o;
}

// ---- step 3: the PlayStation GPU's 4x4 ordered dither, D[y & 3][x & 3] + 4 as sixteen nibbles (entry 0 the lowest)
//   D = {-4, 0, -3, 1}, {2, -2, 3, -1}, {-3, 1, -4, 0}, {3, -1, 2, -2}
DISP_FN int disp_dither(int x, int y) {
    const uint64_t packed = 0x2637'4051'3726'5140ull;
    return (int)((packed >> (4 * (4 * (y & 3) + (x & 3)))) & 15u) - 4;
}
// d: the pixel's dither offset, or 0; mask: 0 or 1
DISP_FN uint32_t disp_pack555(DispRgb c, int d, int mask) {
    const int r = disp_clamp255(c.r + d) >> 3, g = disp_clamp255(c.g + d) >> 3, b = disp_clamp255(c.b + d) >> 3;
    return (uint32_t)(r | (g << 5) | (b << 10) | (mask << 15));
}

// ---- one pixel of a frame in memory, by the steps above: what the kernel computes for (x, y), without its sharing of loads
DISP_FN DispRgb disp_pixel(const uint8_t* frame, int w, int h, int x, int y, bool bilinear) {
    const uint8_t* c = frame + (size_t)w * h;
    const int kx = x >> 1, ky = y >> 1;
    int cr = c[(size_t)ky * w + 2 * kx], cb = c[(size_t)ky * w + 2 * kx + 1];
    if (bilinear) {
        const int fx = disp_far(x, w / 2), fy = disp_far(y, h / 2);
        const uint8_t *rk = c + (size_t)ky * w, *rf = c + (size_t)fy * w;
        cr = disp_vmix(disp_hmix(rk[2 * kx], rk[2 * fx]), disp_hmix(rf[2 * kx], rf[2 * fx]));
        cb = disp_vmix(disp_hmix(rk[2 * kx + 1], rk[2 * fx + 1]), disp_hmix(rf[2 * kx + 1], rf[2 * fx + 1]));
    }
    return disp_matrix(frame[(size_t)y * w + x], cr, cb);
}
