"""The statement of "psxhip ingest v1"  in numpy int64 and `fractions`: a decoder's pictures -- planar,
semi-planar or packed, 8 or 10 bits, padded rows, five matrices, two ranges -- to the scaler's RGB24 or YUV420P, with the picture
selection.  Written from the specification, independently of psxavenc_amd/csrc/ingest_core.h and of include/psxav_hip.h; the CPU
program that runs that header, the library's matrix and the kernels are held to it byte for byte.

Test infrastructure only."""
from fractions import Fraction
import math

import numpy as np

(YUV420P, YUV422P, YUV444P, NV12, NV21, YUYV422, UYVY422, YUV420P10, YUV422P10, YUV444P10, P010, GRAY8,
 RGB24, BGR24, RGBA32, BGRA32) = range(16)
NAMES = ("yuv420p yuv422p yuv444p nv12 nv21 yuyv422 uyvy422 yuv420p10 yuv422p10 yuv444p10 p010 gray8 rgb24 bgr24 rgba32 bgra32").split()
ALL_FORMATS = tuple(range(16))
BT601, BT709, SMPTE240M, FCC, BT2020 = range(5)
OUT_RGB24, OUT_YUV420P = 0, 1
CHROMA_BILINEAR = 1

# Kr, Kb
K = {BT601: (Fraction(299, 1000), Fraction(114, 1000)), BT709: (Fraction(2126, 10000), Fraction(722, 10000)),
     SMPTE240M: (Fraction(212, 1000), Fraction(87, 1000)), FCC: (Fraction(30, 100), Fraction(11, 100)),
     BT2020: (Fraction(2627, 10000), Fraction(593, 10000))}

PLANAR = (YUV420P, YUV422P, YUV444P, YUV420P10, YUV422P10, YUV444P10)
SEMI = (NV12, NV21, P010)
PACKED = (YUYV422, UYVY422)
RGBS = (RGB24, BGR24, RGBA32, BGRA32)
TEN_BIT = (YUV420P10, YUV422P10, YUV444P10, P010)


def depth(fmt):
    return 10 if fmt in TEN_BIT else 8


def subsampling(fmt):
    """(horizontal, vertical): 1 where chroma has half the samples"""
    if fmt in (YUV420P, YUV420P10, NV12, NV21, P010):
        return 1, 1
    if fmt in (YUV422P, YUV422P10, YUYV422, UYVY422):
        return 1, 0
    return 0, 0


def is_yuv(fmt):
    return fmt not in RGBS


def chroma_size(fmt, w, h):
    sx, sy = subsampling(fmt)
    return (w + 1) // 2 if sx else w, (h + 1) // 2 if sy else h


def plane_sizes(fmt, w, h):
    """[(rows, row bytes)] of each plane"""
    cw, ch = chroma_size(fmt, w, h)
    b = 2 if fmt in TEN_BIT else 1
    if fmt in PLANAR:
        return [(h, w * b), (ch, cw * b), (ch, cw * b)]
    if fmt in SEMI:
        return [(h, w * b), (ch, 2 * cw * b)]
    if fmt in PACKED:
        return [(h, 2 * w)]
    if fmt == GRAY8:
        return [(h, w)]
    return [(h, w * (3 if fmt in (RGB24, BGR24) else 4))]


def layout(fmt, w, h, pad=0, first=0, gap=0):
    """plane descriptors [(offset, pitch)] one plane after the other: every row `pad` bytes longer than its samples, the first
    plane at `first`, `gap` bytes between planes -> (planes, bytes of a picture)"""
    planes, at = [], first
    for rows, row in plane_sizes(fmt, w, h):
        planes.append((at, row + pad))
        at += (rows - 1) * (row + pad) + row + gap
    return planes, at - gap


def sample_mask(fmt, w, h, planes, size):
    """bool (size,): the bytes of a picture that are samples"""
    m = np.zeros(size, bool)
    for (off, pitch), (rows, row) in zip(planes, plane_sizes(fmt, w, h)):
        m[(off + np.arange(rows)[:, None] * pitch + np.arange(row)[None, :]).reshape(-1)] = True
    return m


def output_bytes(out_format, w, h):
    return 3 * w * h if out_format == OUT_RGB24 else w * h * 3 // 2


def yuv420p_allowed(fmt, matrix, w, h):
    return is_yuv(fmt) and matrix == BT601 and w % 2 == 0 and h % 2 == 0


def round_half_up(q):
    return math.floor(q + Fraction(1, 2))


def coefficients(matrix, full_range, bits):
    """(cy, rv, gu, gv, bu, yoff, coff): 16 fractional bits, each the round-half-up of the exact rational"""
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    s = 2 ** (bits - 8)
    top = 2 ** bits - 1
    gy = Fraction(255, top) if full_range else Fraction(255, 219 * s)
    gc = Fraction(255, top) if full_range else Fraction(255, 224 * s)
    one = 65536
    return (round_half_up(one * gy), round_half_up(one * 2 * (1 - kr) * gc), round_half_up(one * -2 * kb * (1 - kb) / kg * gc),
            round_half_up(one * -2 * kr * (1 - kr) / kg * gc), round_half_up(one * 2 * (1 - kb) * gc),
            0 if full_range else 16 * s, 2 ** (bits - 1))


# ---- reading a picture

def _plane(pic, plane, rows, row):
    off, pitch = plane
    return pic[off + np.arange(rows)[:, None] * pitch + np.arange(row)[None, :]].astype(np.int64)


def _words(b):
    return b[:, 0::2] | (b[:, 1::2] << 8)


def unpack(pic, fmt, w, h, planes):
    """one picture (1-D uint8) -> (Y, Cb, Cr) sample values, Cb and Cr on the chroma grid (None for grey), or (R, G, B)"""
    sizes = plane_sizes(fmt, w, h)
    p = [_plane(pic, pl, rows, row) for pl, (rows, row) in zip(planes, sizes)]
    if fmt in RGBS:
        n = 3 if fmt in (RGB24, BGR24) else 4
        c = p[0].reshape(h, w, n)
        return (c[..., 2], c[..., 1], c[..., 0]) if fmt in (BGR24, BGRA32) else (c[..., 0], c[..., 1], c[..., 2])
    if fmt == GRAY8:
        return p[0], None, None
    if fmt in PACKED:
        q = p[0].reshape(h, w // 2, 4)
        if fmt == YUYV422:
            return q[..., 0::2].reshape(h, w), q[..., 1], q[..., 3]
        return q[..., 1::2].reshape(h, w), q[..., 0], q[..., 2]
    if fmt in TEN_BIT:
        p = [_words(x) for x in p]
        p = [x >> 6 for x in p] if fmt == P010 else [x & 1023 for x in p]
    if fmt in PLANAR:
        return p[0], p[1], p[2]
    pairs = p[1].reshape(p[1].shape[0], -1, 2)
    return (p[0], pairs[..., 1], pairs[..., 0]) if fmt == NV21 else (p[0], pairs[..., 0], pairs[..., 1])


# ---- chroma to the luma grid

def _near_far(size, n_samples):
    p = np.arange(size)
    k = p >> 1
    return k, np.clip(np.where(p & 1, k + 1, k - 1), 0, n_samples - 1)


def chroma_at_pixels(c, fmt, w, h, bilinear):
    sx, sy = subsampling(fmt)
    if not sx:
        return c
    kx, fx = _near_far(w, c.shape[1])
    if sy:
        ky, fy = _near_far(h, c.shape[0])
        if not bilinear:
            return c[ky][:, kx]
        return (9 * c[ky][:, kx] + 3 * c[ky][:, fx] + 3 * c[fy][:, kx] + c[fy][:, fx] + 8) >> 4
    if not bilinear:
        return c[:, kx]
    return (3 * c[:, kx] + c[:, fx] + 2) >> 2


# ---- the two outputs

def matrix_sums(y, cb, cr, coef):
    """(..., 3) int64: the sums before the shift and the clamp (cb, cr None: grey)"""
    cy, rv, gu, gv, bu, yoff, coff = coef
    base = cy * (y - yoff) + 32768
    if cb is None:
        return np.stack([base, base, base], axis=-1)
    u, v = cb - coff, cr - coff
    return np.stack([base + rv * v, base + gu * u + gv * v, base + bu * u], axis=-1)


def to_rgb24(pic, fmt, w, h, planes, matrix, full_range, bilinear):
    a, b, c = unpack(pic, fmt, w, h, planes)
    if fmt in RGBS:
        rgb = np.stack([a, b, c], axis=-1)
    else:
        coef = coefficients(matrix, full_range, depth(fmt))
        if b is not None:
            b, c = chroma_at_pixels(b, fmt, w, h, bilinear), chroma_at_pixels(c, fmt, w, h, bilinear)
        rgb = np.clip(matrix_sums(a, b, c, coef) >> 16, 0, 255)
    return rgb.astype(np.uint8).reshape(-1)


def box420(c, fmt):
    """chroma on the format's grid -> 4:2:0, 8 bits, one rounding"""
    sx, sy = subsampling(fmt)
    ten = fmt in TEN_BIT
    if sx and sy:
        v = (c + 2) >> 2 if ten else c
    elif sx:
        s = c[0::2] + c[1::2]
        v = (s + 4) >> 3 if ten else (s + 1) >> 1
    else:
        s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        v = (s + 8) >> 4 if ten else (s + 2) >> 2
    return np.minimum(v, 255)


def to_yuv420p(pic, fmt, w, h, planes):
    assert w % 2 == 0 and h % 2 == 0 and is_yuv(fmt)
    y, cb, cr = unpack(pic, fmt, w, h, planes)
    if fmt in TEN_BIT:
        y = np.minimum(255, (y + 2) >> 2)
    if cb is None:
        u = v = np.full((h // 2, w // 2), 128, np.int64)
    else:
        u, v = box420(cb, fmt), box420(cr, fmt)
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).astype(np.uint8)


def convert_one(pic, fmt, w, h, planes, matrix=BT601, full_range=False, out_format=OUT_RGB24, options=0):
    if out_format == OUT_YUV420P:
        assert yuv420p_allowed(fmt, matrix, w, h)
        return to_yuv420p(pic, fmt, w, h, planes)
    return to_rgb24(pic, fmt, w, h, planes, matrix, full_range, bool(options & CHROMA_BILINEAR))


def convert(src, fmt, w, h, planes, matrix=BT601, full_range=False, out_format=OUT_RGB24, options=0, index=None, out=None):
    """src (n_src, src_stride) uint8 -> (n_out, out_stride) uint8.  index: the source picture of each output picture (None:
    identity; negative: that picture is left as it is).  out: the destination as it was before the call (its row length is
    out_stride); None: zeros, tightly packed"""
    index = list(range(src.shape[0])) if index is None else [int(i) for i in index]
    size = output_bytes(out_format, w, h)
    out = np.zeros((len(index), size), np.uint8) if out is None else out.copy()
    assert out.shape[0] == len(index) and out.shape[1] >= size
    done = {}
    for i, k in enumerate(index):
        if k < 0:
            continue
        if k not in done:
            done[k] = convert_one(src[k], fmt, w, h, planes, matrix, full_range, out_format, options)
        out[i, :size] = done[k]
    return out


# ---- the planners (psxavenc/decoding.c:275-285 and :412-461), restated

def c_round(x):
    """round() of C: halves away from zero"""
    a = abs(x)
    f = math.floor(a)
    if a - f >= 0.5:                  # (exact: a and f are neighbours on the same binade or f is 0)
        f += 1
    return f if x >= 0 else -f


def fit(src_w, src_h, max_w, max_h, ignore_aspect=False):
    """(w, h), or None where the library says EINVAL"""
    if src_w < 1 or src_h < 1 or max_w % 16 or max_h % 16 or not 16 <= max_w <= 1024 or not 16 <= max_h <= 1024:
        return None
    w, h = max_w, max_h
    if not ignore_aspect:
        src_ratio = float(src_w) / float(src_h)
        dst_ratio = float(max_w) / float(max_h)
        if src_ratio < dst_ratio:
            w = (int(c_round(float(h) * src_ratio)) + 15) & ~15
        else:
            h = (int(c_round(float(w) / src_ratio)) + 15) & ~15
    if w < 1 or h < 1 or w > max_w or h > max_h:
        return None
    return w, h


def pace(pts, tb_num, tb_den, fps_num, fps_den):
    """the source picture of every output frame"""
    step = float(fps_den) / float(fps_num)
    out, nxt = [], 0.0
    for i, t in enumerate(pts):
        p = float(t) * float(tb_num) / float(tb_den)
        if len(out) >= 1 and p < nxt:
            continue
        if len(out) < 1:
            nxt = p
        else:
            nxt += step
        dupes = max(0, int(math.ceil((p - nxt) / step)))
        for _ in range(dupes):
            out.append(out[-1])
            nxt += step
        out.append(i)
    return out
