// frontend_kernels.hip -- colour conversion + scaling front-end for MI355X (gfx950): RGB24 / YUV420P pictures of any size
// -> NV21 frames of the encoder's size, BT.601 full range, written straight into the buffer the MDEC kernel reads
// (include/psxav_hip.h, psxhip_scaler_*).
//
// The reference hands this step to FFmpeg's libswscale (psxavenc/decoding.c:287-311: sws_getContext(... AV_PIX_FMT_NV21,
// SWS_BICUBIC ...) + sws_setColorspaceDetails(dst = ITU-R BT.601, full range); :463-475: sws_scale into the frame buffer).
// libswscale is not part of the reference tree and not installed here, so there is nothing to be bit-exact TO: the
// arithmetic below is this library's own ("psxhip front-end v1", specified in DESIGN.md section 9 and restated
// independently in oracle/frontend_oracle.c, which the tests hold this kernel to bit for bit).  It follows libswscale's
// structure -- bicubic B = 0 / C = 0.6, taps widened when shrinking, 14-bit coefficients, a horizontal pass into 15-bit
// intermediates, range expansion on the intermediates, a vertical pass -- so results agree with it to within the rounding
// of those formats, but PARITY WITH THE REFERENCE'S SCALER IS UNPINNED and stays so until someone runs both side by side.
//
// Why it exists: the frame encoder consumes 750 GB/s of NV21 at its headline rate, a PCIe link delivers 50 GB/s.  Pictures
// that are decoded on the device (or uploaded once at source size) have to become encoder input without leaving HBM.
//
// Mapping: HBM-bound streaming work, no matrix shape in it.  One workgroup = one BAND of the output -- 64 luma columns (+ the
// 32 chroma pairs under them) -- of one frame, walked top to bottom in tiles of 16 rows; grid = bands x frames x vertical
// segments (>> 256 workgroups for any batch; a lone picture is cut into segments so that the chip still fills).  Per tile, the
// source rows its filters reach AND THE PREVIOUS TILE DID NOT are read, coalesced, converted (RGB -> Y, Cb, Cr) and parked in
// LDS as bytes; the horizontal pass runs LDS -> LDS into a RING of int16 rows that outlives the tile (a source row is
// converted and filtered once per band, not once per tile whose vertical taps touch it: at 2:1 that was 1.5x the rows), the
// vertical pass ring -> registers, and the tile leaves as dword stores (four luma bytes, or two interleaved Cr,Cb pairs, per
// lane).  The band's horizontal taps sit in LDS for the whole walk, the tile's vertical taps are reloaded per tile.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "psxhip_internal.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// out8(): (acc >> 21) clamped to 0..255.  The value passes through an empty asm statement on purpose: hipcc 7.2 (LLVM 22git)
// fuses "shift right, saturate to u8, pack two" into gfx950's v_ashr_pk_u8_i32 and then ORs the other two bytes of the dword
// into the same register -- but the instruction leaves the destination's upper 16 bits as they were (the old accumulator), so
// bytes 2 and 3 of every packed store came out as (right value | leftover bits).  Found by tests/test_gpu_frontend.py (first
// on an enlarging geometry where only three rows per tile hit it, then on all rows once register allocation shifted).  No other
// kernel of the library contains the instruction.
__device__ __forceinline__ uint32_t out8(int acc) {
    int v = acc >> 21;
    asm volatile("" : "+v"(v));
    return (uint32_t)clampi(v, 0, 255);
}

// (q, r) = divmod(start + k * step, d) for k = 0, 1, 2, ...: one division when the walk starts, a compare per step after that
// (every loop of the kernel walks item = tid, tid + 256, ... over a rows x columns grid whose width is a run-time value;
// a division per item cost more than the item's own work)
struct DivWalk {
    int q, r, dq, dr, d;
    __device__ __forceinline__ DivWalk(int start, int step, int d_) : d(d_) {
        q = start / d_; r = start - q * d_;
        dq = step / d_; dr = step - dq * d_;
    }
    __device__ __forceinline__ void next() {
        q += dq; r += dr;
        if (r >= d) { r -= d; q++; }
    }
};

template <int FMT>      // 0 = RGB24, 1 = YUV420P
__global__ __launch_bounds__(256) void scaler_kernel(const psxhip_scaler_job_t job) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = (int)threadIdx.x;
    const int tx = (int)blockIdx.x;
    const uint8_t* src = job.src + (size_t)blockIdx.y * job.src_stride;
    uint8_t* out = job.out + (size_t)blockIdx.y * job.frame_stride;
    const int TW = job.TW, TH = job.TH, CW = TW >> 1, CH = TH >> 1;
    // this segment's tiles
    const int per_seg = (job.tiles_y + job.vsegs - 1) / job.vsegs;
    const int ty0 = (int)blockIdx.z * per_seg, ty1 = min(job.tiles_y, ty0 + per_seg);
    if (ty0 >= ty1) return;

    // ---- the band's output columns and the source columns their taps reach
    const int X0 = tx * TW, X1 = min(job.dw, X0 + TW);
    const int tw = X1 - X0, cw = tw >> 1;
    const int cX0 = X0 >> 1;
    const int lxa = job.lh.left[X0], lxb = job.lh.left[X1 - 1] + job.lh.taps;
    const int cxa = job.ch.left[cX0], cxb = job.ch.left[cX0 + cw - 1] + job.ch.taps;

    // ---- LDS: three byte planes (the rows a tile adds), the two rings of intermediates, the taps.  scaler_layout.h's scaler_lds()
    //      states this carve region by region, and the host sizes the launch by its total: a region added or resized here is added
    //      there.  (The kernel keeps its own pointer chain: placed by scaler_lds()'s offsets it compiled to another instruction stream.)
    static_assert(kScalerPlanePad == 8 && kScalerTileRowBytes == 4 * sizeof(int32_t), "scaler_layout.h: the planes' padding, t_rows' four dwords per tile");
    const int plane_bytes = (job.reg_rows * job.reg_cols + 8 + 15) & ~15;
    const int cplane_bytes = FMT == 0 ? plane_bytes : ((job.creg_rows * job.creg_cols + 8 + 15) & ~15);
    uint8_t* p0 = (uint8_t*)smem;
    uint8_t* p1 = p0 + plane_bytes;
    uint8_t* p2 = p1 + cplane_bytes;
    const int ringL = job.reg_rows, ringC = FMT == 0 ? job.reg_rows : job.creg_rows;      // rows the rings hold
    int16_t* tmpL = (int16_t*)(p2 + cplane_bytes);                               // [ringL][TW]
    int16_t* tmpC = tmpL + (size_t)ringL * TW;                                    // [2][ringC][CW]
    uint32_t* g_lh = (uint32_t*)(tmpC + (size_t)2 * ringC * CW);                 // [TW][2 * taps4] digit dwords (l.., h..)
    uint32_t* g_ch = g_lh + TW * 2 * job.lh.taps4;                                // [CW][2 * taps4]
    int32_t* l_lh = (int32_t*)(g_ch + CW * 2 * job.ch.taps4);                     // [TW]
    int32_t* l_ch = l_lh + TW;                                                    // [CW]
    // the vertical tables of a tile, two copies taken in turn (a tile's are loaded while the previous tile's are still read)
    int32_t* v_tab = l_ch + CW;
    const int v_words = TH + CH + (TH * job.lv.taps + CH * job.cv.taps + 1) / 2;
    // the source rows every tile of this segment reaches (first and past-the-last row of its luma / chroma taps): looked up once
    // for the walk -- as four scalar loads at the top of every tile they stalled the whole workgroup for a memory round trip
    int32_t* t_rows = v_tab + 2 * v_words;                                       // [tiles of the segment][4]

    // (transposed on the way in: dword q of output column i at [q][i], so that the lanes of a wavefront -- consecutive columns --
    //  read consecutive dwords; column-major rows of 4 dwords put every eighth lane on the same LDS bank)
    {
        const int nl = 2 * job.lh.taps4, nc = 2 * job.ch.taps4;
        for (int e = tid; e < tw * nl; e += 256) { const int i = e / nl, q = e - i * nl; g_lh[q * TW + i] = job.lh.digits[(size_t)X0 * nl + e]; }
        for (int e = tid; e < cw * nc; e += 256) { const int i = e / nc, q = e - i * nc; g_ch[q * CW + i] = job.ch.digits[(size_t)cX0 * nc + e]; }
    }
    if (tid < tw) l_lh[tid] = job.lh.left[X0 + tid];
    if (tid < cw) l_ch[tid] = job.ch.left[cX0 + tid];
    for (int t = tid; t < ty1 - ty0; t += 256) {
        const int Y0 = (ty0 + t) * TH, Y1 = min(job.dh, Y0 + TH), cY0 = Y0 >> 1, chh = (Y1 - Y0) >> 1;
        t_rows[4 * t + 0] = job.lv.left[Y0];
        t_rows[4 * t + 1] = job.lv.left[Y1 - 1] + job.lv.taps;
        t_rows[4 * t + 2] = job.cv.left[cY0];
        t_rows[4 * t + 3] = job.cv.left[cY0 + chh - 1] + job.cv.taps;
    }
    __syncthreads();

    // the staged columns (whole groups of four samples: a lane moves dwords)
    int xa, xb, rcols, crcols, cxa4 = 0;
    if (FMT == 0) {
        xa = min(lxa, cxa) & ~3; xb = (max(lxb, cxb) + 3) & ~3;
        rcols = xb - xa; crcols = rcols;
    } else {
        // (YUV planes are staged sixteen bytes to a lane: regions start and end on multiples of sixteen samples)
        xa = lxa & ~15; xb = (lxb + 15) & ~15;
        rcols = xb - xa;
        cxa4 = cxa & ~15;
        crcols = ((cxb + 15) & ~15) - cxa4;
    }
    // ring position of source row r (r may be negative: edge replication reaches above the picture)
    const int offL = ringL * 128, offC = ringC * 128;

    // ---- horizontal pass of one output column over FOUR consecutive rows: four taps at a time; a window's bytes are fetched as
    //      aligned dwords and shifted into place (v_alignbit), biased to int8 (xor 0x80), and multiplied by the taps' two int8 digits
    //      with v_dot4_i32_i8: sum c s = 256 * sum h (s - 128) + sum l (s - 128) + 128 * 16384 (every row of taps sums to 16384).
    //      Exact.  The column's digits are read once for the four rows (the planes' pitch is a multiple of four bytes, so the
    //      rows' windows also share their alignment).
    //      `fixed` carries the number of tap dwords when it is one of the common ones (1: no scaling, 2: 2x down, 3, 4: 4x down):
    //      the loop is then unrolled -- window dwords at immediate offsets, no rotation of the current dword through registers,
    //      no pointer arithmetic (the rolled loop spent 22 of its 38 instructions per four rows and tap dword on those).
    auto hpass4 = [&](auto fixed, const uint8_t* plane, int pitch, int row, int col, const uint32_t* g, int gstride, int taps4, int (&res)[4]) {
        constexpr int T = decltype(fixed)::value;                           // 0: any number of tap dwords (rolled loop)
        const uint32_t at = (uint32_t)(__mul24(row, pitch) + col);          // byte offset of the first row's window in the plane
        const uint32_t* w = (const uint32_t*)(plane + (at & ~3u));
        const uint32_t sh = (at & 3u) * 8u;
        const int pw = pitch >> 2;
        const uint32_t* w1 = w + pw;
        const uint32_t* w2 = w1 + pw;
        const uint32_t* w3 = w2 + pw;
        int acc_l[4] = {128 << 14, 128 << 14, 128 << 14, 128 << 14}, acc_h[4] = {0, 0, 0, 0};
        if constexpr (T > 0) {
            uint32_t win[4][T + 1];
#pragma unroll
            for (int q = 0; q <= T; q++) { win[0][q] = w[q]; win[1][q] = w1[q]; win[2][q] = w2[q]; win[3][q] = w3[q]; }
#pragma unroll
            for (int q = 0; q < T; q++) {
                const int dl = (int)g[q * gstride], dh = (int)g[(T + q) * gstride];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const uint32_t sv = __builtin_amdgcn_alignbit(win[r][q + 1], win[r][q], sh) ^ 0x80808080u;
                    acc_l[r] = __builtin_amdgcn_sdot4(dl, (int)sv, acc_l[r], false);
                    acc_h[r] = __builtin_amdgcn_sdot4(dh, (int)sv, acc_h[r], false);
                }
            }
        } else {
            const uint32_t* gl = g;
            const uint32_t* gh = g + __mul24(taps4, gstride);
            uint32_t cur[4] = {w[0], w1[0], w2[0], w3[0]};
            for (int q = 0; q < taps4; q++) {
                const int dl = (int)*gl, dh = (int)*gh;
                gl += gstride; gh += gstride;
                const uint32_t nxt[4] = {w[q + 1], w1[q + 1], w2[q + 1], w3[q + 1]};
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const uint32_t sv = __builtin_amdgcn_alignbit(nxt[r], cur[r], sh) ^ 0x80808080u;
                    acc_l[r] = __builtin_amdgcn_sdot4(dl, (int)sv, acc_l[r], false);
                    acc_h[r] = __builtin_amdgcn_sdot4(dh, (int)sv, acc_h[r], false);
                    cur[r] = nxt[r];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) res[r] = (acc_h[r] << 8) + acc_l[r];
    };
    // calls `body` with the number of tap dwords as a compile-time constant when it is a common one
    auto with_taps = [&](int taps4, auto body) {
        switch (taps4) {
            case 1: body(std::integral_constant<int, 1>{}); break;
            case 2: body(std::integral_constant<int, 2>{}); break;
            case 3: body(std::integral_constant<int, 3>{}); break;
            case 4: body(std::integral_constant<int, 4>{}); break;
            default: body(std::integral_constant<int, 0>{}); break;
        }
    };

    int have_l = -(1 << 30), have_c = -(1 << 30);          // source rows below these are in the rings (luma / chroma stream)
    for (int ty = ty0; ty < ty1; ty++) {
        const int Y0 = ty * TH, Y1 = min(job.dh, Y0 + TH);
        const int th = Y1 - Y0, chh = th >> 1, cY0 = Y0 >> 1;
        const int lya = t_rows[4 * (ty - ty0) + 0], lyb = t_rows[4 * (ty - ty0) + 1];
        const int cya = t_rows[4 * (ty - ty0) + 2], cyb = t_rows[4 * (ty - ty0) + 3];
        int32_t* vt = v_tab + ((ty - ty0) & 1) * v_words;
        int32_t* l_lv = vt;                                   // [TH] ring position of the first tap's row
        int32_t* l_cv = l_lv + TH;                            // [CH]
        int16_t* f_lv = (int16_t*)(l_cv + CH);                // [TH][taps]
        int16_t* f_cv = f_lv + TH * job.lv.taps;              // [CH][ctaps]
        for (int i = tid; i < th * job.lv.taps; i += 256) f_lv[i] = job.lv.coef[(size_t)Y0 * job.lv.taps + i];
        for (int i = tid; i < chh * job.cv.taps; i += 256) f_cv[i] = job.cv.coef[(size_t)cY0 * job.cv.taps + i];
        if (tid < th) l_lv[tid] = (job.lv.left[Y0 + tid] + offL) % ringL;
        if (tid < chh) l_cv[tid] = (job.cv.left[cY0 + tid] + offC) % ringC;

        // ---- stage the source rows this tile adds: every byte once (edge replication = clamped coordinates)
        int n0, n1, cn0, cn1;          // new rows of the luma stream (RGB: of all three components) / of the chroma stream (YUV)
        if (FMT == 0) {
            // a lane converts four pixels = three dwords of the picture (12 bytes, aligned because a row is 3 * sw bytes and sw a
            // multiple of 4) into one dword of each LDS plane
            n0 = max(min(lya, cya), have_l); n1 = max(lyb, cyb);
            cn0 = n0; cn1 = n1;
            const int rows = n1 - n0, groups = rcols >> 2;
            const bool aligned = (job.sw & 3) == 0 && (((uintptr_t)src) & 3) == 0;
            auto convert = [](int R, int G, int B, uint32_t& y, uint32_t& cb, uint32_t& cr) {
                y = (uint32_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
                cb = (uint32_t)clampi(((-11059 * R - 21709 * G + 32768 * B + 32768) >> 16) + 128, 0, 255);
                cr = (uint32_t)clampi(((32768 * R - 27439 * G - 5329 * B + 32768) >> 16) + 128, 0, 255);
            };
            // kU groups per trip, all their loads issued before the first conversion: a lane that loads, converts and stores one
            // group at a time spends a memory round trip per group (the first version: 27 of them per tile, 55 % of the kernel's
            // wave-cycles waiting)
            constexpr int kU = 4;
            const int n_items = rows * groups;
            DivWalk at(tid, 256, groups);
            for (int base = tid; base < n_items; base += 256 * kU) {
                uint32_t d[kU][3];
                bool fast[kU];
                int sy[kU], x0[kU];
#pragma unroll
                for (int u = 0; u < kU; u++) {
                    const int item = base + u * 256;
                    if (item - tid >= n_items) break;             // (uniform: no lane has an item in this slot or the ones after)
                    const int r = at.q, g = at.r;
                    at.next();
                    sy[u] = clampi(n0 + r, 0, job.sh - 1);
                    x0[u] = xa + 4 * g;
                    fast[u] = item < n_items && aligned && x0[u] >= 0 && x0[u] + 3 < job.sw;
                    // every lane loads, the others from the picture's first bytes: a load under a branch is waited for before the
                    // next one is issued (the compiler closes each divergent block with s_waitcnt vmcnt(0))
                    const uint32_t off = (__umul24((uint32_t)sy[u], (uint32_t)job.sw) + (uint32_t)x0[u]) * 3u;     // < 2^31: pictures are at most 16384 x 16384
                    __builtin_memcpy(d[u], src + (fast[u] ? off : 0u), 12);
                }
#pragma unroll
                for (int u = 0; u < kU; u++) {
                    const int item = base + u * 256;
                    if (item - tid >= n_items) break;
                    if (item >= n_items) continue;
                    uint32_t Y = 0, CB = 0, CR = 0;
                    if (fast[u]) {
                        // The same three forms on v_dot4_u32_u8: a pixel's bytes (R, G, B, one byte of its neighbour against a zero
                        // coefficient) times the coefficients' two base-256 digits.  Negative coefficients are applied to the
                        // complemented byte (-c p = c (255 - p) - 255 c): with R, G complemented Cb's coefficients are 11059, 21709,
                        // 32768, with G, B complemented Cr's are 32768, 27439, 5329, and either constant comes to
                        // 32768 + (128 << 16) - 32768 * 255 = 65536.  The sums are >= 65536, so the lower clamp never acts; the upper
                        // one is a min on the 24-bit sum.  The answer is byte 2 of each sum.
                        const uint32_t d0 = d[u][0], d1 = d[u][1], d2 = d[u][2];
                        uint32_t px[4] = {d0, __builtin_amdgcn_alignbit(d1, d0, 24), __builtin_amdgcn_alignbit(d2, d1, 16), d2 >> 8};
                        uint32_t ty[4], tb[4], tr[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const uint32_t p = px[k], pb = p ^ 0x0000FFFFu, pr = p ^ 0x00FFFF00u;
                            ty[k] = (__builtin_amdgcn_udot4(p, 76u | 150u << 8 | 29u << 16, 0u, false) << 8) +
                                    __builtin_amdgcn_udot4(p, 139u | 70u << 8 | 47u << 16, 32768u, false);
                            tb[k] = min((__builtin_amdgcn_udot4(pb, 43u | 84u << 8 | 128u << 16, 0u, false) << 8) +
                                        __builtin_amdgcn_udot4(pb, 51u | 205u << 8, 65536u, false), 0xFFFFFFu);
                            tr[k] = min((__builtin_amdgcn_udot4(pr, 128u | 107u << 8 | 20u << 16, 0u, false) << 8) +
                                        __builtin_amdgcn_udot4(pr, 47u << 8 | 209u << 16, 65536u, false), 0xFFFFFFu);
                        }
                        Y = __builtin_amdgcn_perm(ty[1], ty[0], 0x0c0c0602u) | __builtin_amdgcn_perm(ty[3], ty[2], 0x06020c0cu);
                        CB = __builtin_amdgcn_perm(tb[1], tb[0], 0x0c0c0602u) | __builtin_amdgcn_perm(tb[3], tb[2], 0x06020c0cu);
                        CR = __builtin_amdgcn_perm(tr[1], tr[0], 0x0c0c0602u) | __builtin_amdgcn_perm(tr[3], tr[2], 0x06020c0cu);
                    } else {                              // the picture's edges (clamped coordinates), or an unaligned picture
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const uint8_t* px = src + (__umul24((uint32_t)sy[u], (uint32_t)job.sw) + (uint32_t)clampi(x0[u] + k, 0, job.sw - 1)) * 3u;
                            uint32_t y, cb, cr;
                            convert(px[0], px[1], px[2], y, cb, cr);
                            Y |= y << (8 * k); CB |= cb << (8 * k); CR |= cr << (8 * k);
                        }
                    }
                    ((uint32_t*)p0)[item] = Y;            // item = r * groups + g = dword index (rcols = 4 * groups)
                    ((uint32_t*)p1)[item] = CB;
                    ((uint32_t*)p2)[item] = CR;
                }
            }
        } else {
            n0 = max(lya, have_l); n1 = lyb;
            cn0 = max(cya, have_c); cn1 = cyb;
            const uint8_t* Y = src;
            const uint8_t* U = src + (size_t)job.sw * job.sh;
            const uint8_t* V = U + (size_t)job.csw * job.csh;
            // a lane moves sixteen samples: one 16-byte load (the picture's rows need not be 16-byte aligned; the loads are dword
            // aligned), one 16-byte LDS store (the planes' rows are).  The first version moved dwords: 25 instructions per dword
            // made this plain copy 38 % of the kernel.
            auto stage = [&](uint8_t* dst, const uint8_t* plane, int pw, int ph, int y0, int rows, int x0, int cols) {
                const int groups = cols >> 4, n_items = rows * groups;
                const bool aligned = (pw & 3) == 0 && (((uintptr_t)plane) & 3) == 0;
                constexpr int kU = 2;
                DivWalk at(tid, 256, groups);
                for (int base = tid; base < n_items; base += 256 * kU) {
                    uint4 v[kU];
#pragma unroll
                    for (int u = 0; u < kU; u++) {
                        const int item = base + u * 256;
                        const int r = at.q, g = at.r;
                        at.next();
                        const int sy = clampi(y0 + r, 0, ph - 1), x = x0 + 16 * g;
                        const uint32_t rowoff = __umul24((uint32_t)sy, (uint32_t)pw);      // (planes are at most 16384 x 16384)
                        v[u] = make_uint4(0u, 0u, 0u, 0u);
                        if (item < n_items) {
                            if (aligned && x >= 0 && x + 15 < pw) {
                                __builtin_memcpy(&v[u], plane + (rowoff + (uint32_t)x), 16);
                            } else {                          // the picture's edges: clamped coordinates, byte by byte
                                auto four = [&](int xk) {
                                    uint32_t d = 0u;
#pragma unroll
                                    for (int k = 0; k < 4; k++) d |= (uint32_t)plane[rowoff + (uint32_t)clampi(xk + k, 0, pw - 1)] << (8 * k);
                                    return d;
                                };
                                v[u] = make_uint4(four(x), four(x + 4), four(x + 8), four(x + 12));
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < kU; u++)
                        if (base + u * 256 < n_items) ((uint4*)dst)[base + u * 256] = v[u];
                }
            };
            stage(p0, Y, job.sw, job.sh, n0, n1 - n0, xa, rcols);
            stage(p1, U, job.csw, job.csh, cn0, cn1 - cn0, cxa4, crcols);      // Cb
            stage(p2, V, job.csw, job.csh, cn0, cn1 - cn0, cxa4, crcols);      // Cr
        }
        have_l = n1; have_c = cn1;
        __syncthreads();

        // ---- horizontal pass over the new rows, LDS -> the rings: 15-bit intermediates (+ the range expansion of limited-range input)
        //      (rows past the last new one in the last group of four read whatever follows in LDS and are not stored)
        {
            const int rows = n1 - n0, c_off = -xa, taps4 = job.lh.taps4;
            const int ring0 = (n0 + offL) % ringL;
            with_taps(taps4, [&](auto fixed) {
                DivWalk la(tid, 256, tw);
                for (int item = tid; item < ((rows + 3) >> 2) * tw; item += 256, la.next()) {
                    const int r4 = la.q * 4, i = la.r;
                    int acc[4];
                    hpass4(fixed, p0, rcols, r4, l_lh[i] + c_off, g_lh + i, TW, taps4, acc);
                    int rr = ring0 + r4;
                    if (rr >= ringL) rr -= ringL;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        int t = clampi(acc[r] >> 7, 0, 32767);
                        if (job.limited) t = (__mul24(min(t, 30189), 19077) - 39057361) >> 14;        // (at most 30189 * 19077 < 2^31)
                        if (r4 + r < rows) tmpL[__mul24(rr, TW) + i] = (int16_t)t;
                        rr = rr + 1 == ringL ? 0 : rr + 1;
                    }
                }
            });
            const int crows = cn1 - cn0, cc_off = FMT == 0 ? -xa : -cxa4, ctaps4 = job.ch.taps4;
            const int cring0 = (cn0 + offC) % ringC;
            const int cgroups = (crows + 3) >> 2;
            with_taps(ctaps4, [&](auto fixed) {
                DivWalk ca(tid, 256, cw);
                for (int item = tid; item < 2 * cgroups * cw; item += 256, ca.next()) {
                    const int comp = ca.q >= cgroups ? 1 : 0, r4 = (ca.q - comp * cgroups) * 4, i = ca.r;      // groups 0..cgroups-1: Cr, then Cb
                    int acc[4];
                    hpass4(fixed, comp ? p1 : p2, crcols, r4, l_ch[i] + cc_off, g_ch + i, CW, ctaps4, acc);      // comp 0 = Cr, 1 = Cb
                    int rr = cring0 + r4;
                    if (rr >= ringC) rr -= ringC;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        int t = clampi(acc[r] >> 7, 0, 32767);
                        if (job.limited) t = (__mul24(min(t, 30775), 4663) - 9289992) >> 12;
                        if (r4 + r < crows) tmpC[__mul24(__mul24(comp, ringC) + rr, CW) + i] = (int16_t)t;
                        rr = rr + 1 == ringC ? 0 : rr + 1;
                    }
                }
            });
        }
        __syncthreads();

        // ---- vertical pass, rings -> registers -> HBM: a lane makes four adjacent luma bytes / two adjacent Cr,Cb pairs
        {
            const int taps = job.lv.taps, q = tw >> 2;
            DivWalk va(tid, 256, q);
            for (int item = tid; item < th * q; item += 256, va.next()) {
                const int j = va.q, i4 = va.r * 4;
                const int16_t* f = f_lv + j * taps;
                int rr = l_lv[j];
                const int16_t* t = tmpL + __mul24(rr, TW) + i4;
                int a0 = 1 << 20, a1 = 1 << 20, a2 = 1 << 20, a3 = 1 << 20;
                for (int k = 0; k < taps; k++) {
                    const int c = (int)f[k];
                    const uint2 v4 = *(const uint2*)t;                       // four int16 (i4 and TW are multiples of 4)
                    a0 += c * (int)(int16_t)(v4.x & 0xFFFFu); a1 += c * ((int)v4.x >> 16);
                    a2 += c * (int)(int16_t)(v4.y & 0xFFFFu); a3 += c * ((int)v4.y >> 16);
                    rr++; t += TW;
                    if (rr == ringL) { rr = 0; t = tmpL + i4; }
                }
                const uint32_t v = out8(a0) | out8(a1) << 8 | out8(a2) << 16 | out8(a3) << 24;
                *(uint32_t*)(out + (size_t)(Y0 + j) * job.dw + X0 + i4) = v;
            }
            const int ctaps = job.cv.taps, cq = cw >> 1;
            uint8_t* cout = out + (size_t)job.dw * job.dh;
            DivWalk vc(tid, 256, cq);
            for (int item = tid; item < chh * cq; item += 256, vc.next()) {
                const int j = vc.q, i2 = vc.r * 2;
                const int16_t* f = f_cv + j * ctaps;
                int rr = l_cv[j];
                const int cb_off = __mul24(ringC, CW);
                const int16_t* cr = tmpC + __mul24(rr, CW) + i2;
                int r0 = 1 << 20, r1 = 1 << 20, b0 = 1 << 20, b1 = 1 << 20;
                for (int k = 0; k < ctaps; k++) {
                    const int c = (int)f[k];
                    const uint32_t vr = *(const uint32_t*)cr, vb = *(const uint32_t*)(cr + cb_off);      // two int16 each (i2, CW, ringC * CW even)
                    r0 += c * (int)(int16_t)(vr & 0xFFFFu); r1 += c * ((int)vr >> 16);
                    b0 += c * (int)(int16_t)(vb & 0xFFFFu); b1 += c * ((int)vb >> 16);
                    rr++; cr += CW;
                    if (rr == ringC) { rr = 0; cr = tmpC + i2; }
                }
                // NV21: Cr at even bytes, Cb at odd (mdec.c:627-628)
                const uint32_t v = out8(r0) | out8(b0) << 8 | out8(r1) << 16 | out8(b1) << 24;
                *(uint32_t*)(cout + (size_t)(cY0 + j) * job.dw + (size_t)(cX0 + i2) * 2) = v;
            }
        }
    }
}
}  // namespace

extern "C" hipError_t psxhip_scaler_prepare(int yuv, int max_lds) {
    return hipFuncSetAttribute(yuv ? (const void*)scaler_kernel<1> : (const void*)scaler_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
}

extern "C" hipError_t psxhip_scaler_launch(const psxhip_scaler_job_t* j, int yuv, int n_frames, size_t lds_bytes, void* stream) {
    const dim3 grid((unsigned)j->tiles_x, (unsigned)n_frames, (unsigned)j->vsegs);
    void* args[] = {(void*)j};
    return hipLaunchKernel(yuv ? (const void*)scaler_kernel<1> : (const void*)scaler_kernel<0>, grid, dim3(256), args, lds_bytes, (hipStream_t)stream);
}
