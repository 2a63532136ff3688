"""What the picture ingest is shown: source pictures of every format as bytes in memory, and the list of conversions.  Shared by the
CPU program's test (tests/test_ingest_core_cpu.py) and the kernels' (tests/test_gpu_ingest.py), so that the kernels see nothing the
arithmetic of one sample has not passed on the CPU first.

Test infrastructure only."""
import numpy as np

import ingest_ref as R

# the sizes at which the kernel can go wrong: a run of eight pixels and two rows per lane (a picture has ceil(w / 8) ceil(h / 2)
# lanes), so 1 .. 7 pixels left over at the right edge, one lane, more than one lane; 2 mod 4 widths start every other packed output
# row off a dword.  All of these stay inside one wavefront of 64 lanes: the largest are 127x5 (48 lanes), 66x10 (45), 130x4 (34) and
# 258x2 (33)
EVEN_SIZES = [(2, 2), (6, 4), (18, 2), (34, 6), (66, 10), (130, 4), (258, 2)]
ODD_SIZES = [(1, 1), (3, 3), (5, 7), (33, 1), (65, 3), (127, 5)]          # RGB24 output only
# ... and sizes whose rows are whole runs on dwords, which the sizes above never are: the kernel's dword loads and stores
WHOLE_SIZES = [(8, 2), (16, 4), (24, 6), (64, 4)]
# ... and sizes of more than one wavefront and more than one workgroup of 256 lanes, shown on their own (wide_sizes_for): 130x10 is
# 85 lanes, two wavefronts whose bilinear rows meet across the seam; 512x6 is 192, whole dwords and a wavefront per row; 522x10 is
# 330, two workgroups, rows that start off a dword and a tail of 74 lanes; 2050x2 is 257, a second workgroup of one lane; 517x5 is
# 195 and odd (RGB24 output only, not for packed formats)
WIDE_SIZES = [(130, 10), (512, 6), (522, 10), (2050, 2), (517, 5)]
MATRICES = (R.BT601, R.BT709, R.BT2020)
PADS = (1, 3, 13)
OFFSETS = (0, 1, 2, 3)


def sizes_for(fmt, out_format):
    sizes = EVEN_SIZES + WHOLE_SIZES + (ODD_SIZES if out_format == R.OUT_RGB24 else [])
    return [s for s in sizes if not (fmt in R.PACKED and s[0] % 2)]


def wide_sizes_for(fmt, out_format):
    return [s for s in WIDE_SIZES if not ((s[0] | s[1]) & 1 and (out_format != R.OUT_RGB24 or fmt in R.PACKED))]


def lanes_of(w, h):
    return ((w + 7) // 8) * ((h + 1) // 2)


def settings_for(fmt):
    """every (matrix, full_range, out_format, options) a format is shown with: both outputs where allowed, both chroma modes, three
    matrices, both ranges"""
    if fmt in R.RGBS:
        return [(R.BT601, True, R.OUT_RGB24, 0), (R.BT709, False, R.OUT_RGB24, R.CHROMA_BILINEAR)]      # (matrix, range and option are ignored)
    out = [(m, full, R.OUT_RGB24, opt) for m in MATRICES for full in (False, True) for opt in (0, R.CHROMA_BILINEAR)]
    return out + [(R.BT601, full, R.OUT_YUV420P, 0) for full in (False, True)]


def _put(pic, plane, rows, row, values):
    off, pitch = plane
    pic[off + np.arange(rows)[:, None] * pitch + np.arange(row)[None, :]] = values


def pack(fmt, w, h, planes, size, comps, rng, fill):
    """one picture of `size` bytes, every byte that is no sample `fill`: comps = (Y, Cb, Cr) sample values (chroma on the format's
    grid) or (R, G, B).  The unused bits of a 16-bit word are garbage from rng: the high 6 of a planar word, the low 6 of P010's"""
    pic = np.full(size, fill, np.uint8)
    a, b, c = [None if x is None else np.asarray(x, np.int64) for x in comps]
    sizes = R.plane_sizes(fmt, w, h)

    def words(v):
        g = rng.integers(0, 64, v.shape)
        v = (v << 6) | g if fmt == R.P010 else v | (g << 10)
        return np.stack([v & 255, v >> 8], axis=-1).reshape(v.shape[0], -1)

    if fmt in R.RGBS:
        first, last = (c, a) if fmt in (R.BGR24, R.BGRA32) else (a, c)
        parts = [first, b, last] + ([rng.integers(0, 256, a.shape)] if fmt in (R.RGBA32, R.BGRA32) else [])
        rows = [np.stack(parts, axis=-1).reshape(h, -1)]
    elif fmt == R.GRAY8:
        rows = [a]
    elif fmt in R.PACKED:
        ya = a.reshape(h, w // 2, 2)
        q = [ya[..., 0], b, ya[..., 1], c] if fmt == R.YUYV422 else [b, ya[..., 0], c, ya[..., 1]]
        rows = [np.stack(q, axis=-1).reshape(h, -1)]
    elif fmt in R.PLANAR:
        rows = [words(x) if fmt in R.TEN_BIT else x for x in (a, b, c)]
    else:
        pairs = np.stack([c, b] if fmt == R.NV21 else [b, c], axis=-1).reshape(b.shape[0], -1)
        rows = [words(a), words(pairs)] if fmt in R.TEN_BIT else [a, pairs]
    for plane, (n_rows, row), values in zip(planes, sizes, rows):
        assert values.shape == (n_rows, row), (fmt, values.shape, n_rows, row)
        _put(pic, plane, n_rows, row, values.astype(np.uint8))
    return pic


def pictures(fmt, w, h, planes, stride, seed, fill=0xA5):
    """(4, stride) uint8: two pictures of noise in every byte (pad bytes and the unused bits of 16-bit words included), and the two
    0 / max checkerboards of every component; (kinds)"""
    rng = np.random.default_rng([seed, fmt, w, h])
    top = 255 if fmt not in R.TEN_BIT else 1023
    cw, ch = R.chroma_size(fmt, w, h)
    out = [rng.integers(0, 256, stride).astype(np.uint8) for _ in range(2)]
    for phase in (0, 1):
        def board(rows, cols, flip):
            return (((np.arange(rows)[:, None] + np.arange(cols)[None, :] + phase + flip) & 1) * top).astype(np.int64)
        if fmt in R.RGBS:
            comps = (board(h, w, 0), board(h, w, 1), board(h, w, 0))
        elif fmt == R.GRAY8:
            comps = (board(h, w, 0), None, None)
        else:
            comps = (board(h, w, 0), board(ch, cw, 1), board(ch, cw, 0))
        out.append(pack(fmt, w, h, planes, stride, comps, rng, fill))
    return np.stack(out), ("noise", "noise", "checker", "checker")
