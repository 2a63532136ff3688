"""psxhip MDEC reconstruct v1 in numpy int64: levels -> NV21 pixels.  The device kernel
(csrc/mdec_decode_kernels.hip: mdec_reconstruct_kernel) is held to this bit for bit; this in turn is held to the oracle's float64
reconstruction within a bound derived below from its own constants and shifts (tests/test_mdec_recon_ref.py).

Per 8x8 block, levels lv[0..63] in zig-zag order, quant scale s (the header's 16-bit field), Q = the quant matrix in raster order:

  dequantise   F8[0]  = clamp(16 * lv[0],                 -SAT, SAT - 1)          DC x 2, with three fraction bits
               F8[ri] = clamp(lv[z] * Q[ri] * s,          -SAT, SAT - 1)          ri = raster position of scan position z >= 1
                        (level x Q x scale / 8 exactly, kept as eighths; SAT = 2^14: |coefficient| < 2048, twice what an 8x8
                        block of 8-bit pixels can produce, so saturation touches no stream an encoder made.  The saturating
                        range is exercised all the same, not only argued: tests/mdec_foreign_streams.py writes streams whose
                        coefficients saturate, and statement and kernel are held to a float64 IDCT of the clamped values there)
  rows         T[v][x] = (sum_u F8[v][u] * C[u][x] + 2^14) >> 15                   two fraction bits are kept
  columns      P[y][x] = (sum_v T[v][x]  * C[v][y] + 2^15) >> 16
  pixel        clamp(P + 128, 0, 255)

with C[u][x] = round(2^14 * c(u) * cos((2x + 1) u pi / 16)), c(0) = sqrt(1/8), c(u) = 1/2: the eight magnitudes IDCT_MAG below,
and >> an arithmetic shift (floor).  Blocks are placed as the encoder reads them: macroblocks column-major, blocks Cr, Cb, Y0..Y3.
"""
import numpy as np

SAT = 1 << 14
SHIFT1, SHIFT2 = 15, 16
CBITS = 14
# round(2^14 * cos(k pi / 16) / 2) for k = 0..7; c(0) cos(0) = sqrt(1/8) has the magnitude of k = 4
IDCT_MAG = (8192, 8035, 7568, 6811, 5793, 4551, 3135, 1598)
QUANT = np.array([
    2, 16, 19, 22, 26, 27, 29, 34,
    16, 16, 22, 24, 27, 29, 34, 37,
    19, 22, 26, 27, 29, 34, 34, 38,
    22, 22, 26, 27, 29, 34, 37, 40,
    22, 26, 27, 29, 32, 35, 40, 48,
    26, 27, 29, 32, 35, 40, 48, 58,
    26, 27, 29, 34, 38, 46, 56, 69,
    27, 29, 35, 38, 46, 56, 69, 83], np.int64)


def zagzig():
    """scan position -> raster position"""
    order = []
    for s in range(15):
        diag = [(y, s - y) for y in range(8) if 0 <= s - y < 8]
        if s % 2 == 0:
            diag.reverse()
        order += [y * 8 + x for (y, x) in diag]
    return np.array(order, np.int64)


def idct_matrix():
    """C[u][x], int64"""
    c = np.zeros((8, 8), np.int64)
    for u in range(8):
        for x in range(8):
            if u == 0:
                c[u, x] = IDCT_MAG[4]
                continue
            k = ((2 * x + 1) * u) % 32                   # cos(k pi / 16), folded into k = 0..8 with a sign
            sign = 1
            if k > 16:
                k = 32 - k
            if k > 8:
                k, sign = 16 - k, -1
            c[u, x] = 0 if k == 8 else sign * IDCT_MAG[k]
    return c


def real_matrix():
    """the exact basis the integers stand for: cs[u][x], float64"""
    u = np.arange(8)[:, None]
    x = np.arange(8)[None, :]
    return np.where(u == 0, np.sqrt(0.125), 0.5) * np.cos((2 * x + 1) * u * np.pi / 16.0)


def dequantise(levels, scale):
    """levels (blocks, 64) zig-zag -> F8 (blocks, 8, 8) raster, eighths"""
    lv = np.asarray(levels, np.int64).reshape(-1, 64)
    zz = zagzig()
    f = np.zeros_like(lv)
    f[:, zz] = lv * QUANT[zz] * int(scale)
    f[:, 0] = lv[:, 0] * 16
    return np.clip(f, -SAT, SAT - 1).reshape(-1, 8, 8)


def idct_blocks(f8):
    """F8 (blocks, 8, 8) -> pixels (blocks, 8, 8) uint8"""
    c = idct_matrix()
    t = (np.einsum("bvu,ux->bvx", f8, c) + (1 << (SHIFT1 - 1))) >> SHIFT1
    p = (np.einsum("bvx,vy->byx", t, c) + (1 << (SHIFT2 - 1))) >> SHIFT2
    return np.clip(p + 128, 0, 255).astype(np.uint8)


def place(w, h, px):
    """pixels (blocks, 8, 8) -> NV21 frame, the encoder's block order"""
    nx, ny = w // 16, h // 16
    px = px.reshape(nx, ny, 6, 8, 8)
    out = np.zeros(w * h * 3 // 2, np.uint8)
    luma = out[:w * h].reshape(ny, 2, 8, nx, 2, 8)        # [fy][by][y][fx][bx][x]
    luma[...] = px[:, :, 2:].reshape(nx, ny, 2, 2, 8, 8).transpose(1, 2, 4, 0, 3, 5)
    chroma = out[w * h:].reshape(ny, 8, nx, 8, 2)         # [fy][y][fx][x][Cr | Cb]
    chroma[..., 0] = px[:, :, 0].transpose(1, 2, 0, 3)
    chroma[..., 1] = px[:, :, 1].transpose(1, 2, 0, 3)
    return out


def reconstruct(w, h, levels, scale):
    return place(w, h, idct_blocks(dequantise(levels, scale)))


# ---------------------------------------------------------------- the ranges every intermediate can take
def worst_case():
    """largest magnitude of every intermediate over all levels (-512..511 from the syntax; a v3 DC without the wrap is any int16) and
    all scales (0..65535): what the 32-bit device arithmetic has to hold"""
    c = np.abs(idct_matrix())
    level, dc = 512, 32768
    out = {}
    # the device multiplies by min(scale, SAT): once scale >= SAT every non-zero product is beyond +-SAT anyway
    out["dequant product"] = level * int(QUANT.max()) * SAT
    out["dc product"] = dc * 16
    out["F8"] = SAT
    out["row sum"] = SAT * int(c.sum(axis=0).max()) + (1 << (SHIFT1 - 1))
    t = out["row sum"] >> SHIFT1
    out["T"] = t
    out["column sum"] = t * int(c.sum(axis=0).max()) + (1 << (SHIFT2 - 1))
    return out


# ---------------------------------------------------------------- distance to the real-valued IDCT
def error_bound(f8):
    """Per block: E with |P_exact - R| <= E, where R = the real IDCT of F8 / 8 and P_exact = the value the last shift rounds.
    Three parts, all from the constants above:
      the integer basis   |sum F8/8 (C C' / 2^28 - cs cs')| <= sum |F8|/8 * max-over-pixels |C[u][x] C[v][y] / 2^28 - cs[u][x] cs[v][y]|
      the row shift       each T is off by at most 1/2 (in quarter pixels after the 2^14 of the columns: / 2^SHIFT2), times sum_v |C[v][y]|
    The last shift's own rounding is the one lrint also makes: |round(a) - round(b)| <= floor(|a - b|) + 1 covers it."""
    c, cs = idct_matrix().astype(np.float64), real_matrix()
    k = np.abs(np.einsum("ux,vy->vuyx", c, c) / 2.0 ** (2 * CBITS) - np.einsum("ux,vy->vuyx", cs, cs)).max(axis=(2, 3))    # [v][u]
    basis = (np.abs(f8).astype(np.float64) / 8.0 * k[None]).sum(axis=(1, 2))
    rows = 0.5 * np.abs(c).sum(axis=0).max() / 2.0 ** SHIFT2
    return basis + rows


def pixel_bound(f8):
    """largest |device pixel - lrint(real pixel)| the statement allows, per block"""
    return np.floor(error_bound(f8)).astype(np.int64) + 1


def real_pixels(f8):
    """clip(rint(real IDCT of F8 / 8 + 128), 0, 255) in float64, (blocks, 8, 8) int64: what the integers stand for, F8 as dequantise()
    gives it, saturated coefficients included"""
    cs = real_matrix()
    return np.clip(np.rint(np.einsum("bvu,ux,vy->byx", np.asarray(f8, np.float64) / 8.0, cs, cs) + 128.0), 0, 255).astype(np.int64)


def saturating_blocks(levels, scale):
    """per block: a coefficient is clamped, i.e. dequantise() differs from the plain product"""
    lv = np.asarray(levels, np.int64).reshape(-1, 64)
    zz = zagzig()
    f = np.zeros_like(lv)
    f[:, zz] = lv * QUANT[zz] * int(scale)
    f[:, 0] = lv[:, 0] * 16
    return (f.reshape(-1, 8, 8) != dequantise(lv, scale)).any(axis=(1, 2))


# ---------------------------------------------------------------- SSE
def sse(w, h, a, b):
    """(n, 3) uint64: Y, Cb, Cr sums of squared differences of two (n, >= w*h*3/2) NV21 arrays"""
    a = np.asarray(a)[:, :w * h * 3 // 2].astype(np.int64)
    b = np.asarray(b)[:, :w * h * 3 // 2].astype(np.int64)
    d = (a - b) ** 2
    return np.stack([d[:, :w * h].sum(axis=1), d[:, w * h + 1::2].sum(axis=1), d[:, w * h::2].sum(axis=1)], axis=1).astype(np.uint64)
