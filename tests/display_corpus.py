"""The pictures the display back-end is shown, for the CPU program (tests/test_display_core_cpu.py) and the kernels
(tests/test_gpu_display.py), and the statement's answers for them, computed once per size and left unchanged.

  noise      uniform in all three planes: most of it lies outside the RGB gamut, so every clamp of the matrix is hit
  corners    the eight flat pictures with Y, Cb, Cr in {0, 255}
  checker    chroma checkerboards of period 1 and 2 samples, Cr and Cb in opposite phase, over noise luma
  single     one chroma sample that differs from its plane, at each corner and the middle of each edge: bilinear's clamped neighbours
  ramp       grey chroma, luma constant over each 4x4 dither tile and counting up from tile to tile (and on into the next frame) until
             every value 0 .. 255 has met every dither cell: R = G = B = Y there, so every 5-bit boundary is crossed in every cell

Test infrastructure only."""
import functools

import numpy as np

import display_ref as R

SIZES = [(16, 16), (32, 16), (16, 32), (48, 32), (320, 240)]


def _frame(w, h, y, cr, cb):
    f = np.empty(w * h * 3 // 2, np.uint8)
    f[:w * h] = np.asarray(y, np.uint8).reshape(-1)
    c = f[w * h:].reshape(h // 2, w // 2, 2)
    c[..., 0], c[..., 1] = cr, cb
    return f


@functools.lru_cache(maxsize=None)
def frames(w, h):
    """(n, w h 3 / 2) uint8, read-only, and the kind of every frame"""
    rng = np.random.default_rng(1000 * w + h)
    cw, ch = w // 2, h // 2
    out, kinds = [], []

    def add(kind, f):
        out.append(f)
        kinds.append(kind)
    for _ in range(2):
        add("noise", rng.integers(0, 256, w * h * 3 // 2).astype(np.uint8))
    for y in (0, 255):
        for cb in (0, 255):
            for cr in (0, 255):
                add("corners", _frame(w, h, np.full((h, w), y), cr, cb))
    yy, xx = np.mgrid[0:ch, 0:cw]
    for period in (1, 2):
        phase = ((xx // period) + (yy // period)) & 1
        add("checker", _frame(w, h, rng.integers(0, 256, (h, w)), 255 * phase, 255 * (1 - phase)))
    for sx, sy in [(0, 0), (cw - 1, 0), (0, ch - 1), (cw - 1, ch - 1), (cw // 2, 0), (cw // 2, ch - 1), (0, ch // 2), (cw - 1, ch // 2)]:
        cr, cb = np.full((ch, cw), 100), np.full((ch, cw), 150)
        cr[sy, sx], cb[sy, sx] = 255, 0
        add("single", _frame(w, h, rng.integers(0, 256, (h, w)), cr, cb))
    tiles = (w // 4) * (h // 4)
    ys, xs = np.mgrid[0:h, 0:w]
    tile = (xs >> 2) + (w // 4) * (ys >> 2)
    n_ramp = -(-256 // tiles)
    for k in range(n_ramp):
        add("ramp", _frame(w, h, (tile + tiles * k) & 255, 128, 128))
    all_frames = np.stack(out)
    # every luma value meets every dither cell on the ramps
    ramp = all_frames[[k == "ramp" for k in kinds], :w * h].reshape(n_ramp, h, w)
    for cy in range(4):
        for cx in range(4):
            assert np.unique(ramp[:, cy::4, cx::4]).size == 256
    all_frames.setflags(write=False)
    return all_frames, tuple(kinds)


@functools.lru_cache(maxsize=None)
def colours(w, h, bilinear):
    c = R.rgb(frames(w, h)[0], w, h, bilinear)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(w, h, out_format, options):
    """the statement's pictures of frames(w, h): (n, h, row bytes) uint8, read-only"""
    p = R.pack(colours(w, h, bool(options & R.CHROMA_BILINEAR)), out_format, options)
    p.setflags(write=False)
    return p
