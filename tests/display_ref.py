"""The statement of "psxhip display v1"  in numpy int64: NV21 frames -> RGB24 / RGBX32 / RGB555, both chroma
modes, dither, mask bit, pitch and stride, the decoder's gate.  Written from the specification, independently of
psxavenc_amd/csrc/display_core.h; the CPU program that runs that header and the kernels are held to it byte for byte.

Test infrastructure only."""
import numpy as np

OUT_RGB24, OUT_RGBX32, OUT_RGB555 = 0, 1, 2
CHROMA_BILINEAR, DITHER, MASK_BIT = 1, 2, 4
FORMATS = (OUT_RGB24, OUT_RGBX32, OUT_RGB555)

# the 16-bit matrix: (Y, cb, cr) coefficients of R, G, B
MATRIX = np.array([[65536, 0, 91881], [65536, -22553, -46802], [65536, 116130, 0]], np.int64)
# the PlayStation GPU's ordered dither, D[y & 3][x & 3]
D = np.array([[-4, 0, -3, 1], [2, -2, 3, -1], [-3, 1, -4, 0], [3, -1, 2, -2]], np.int64)


def row_bytes(out_format, width):
    return {OUT_RGB24: 3, OUT_RGBX32: 4, OUT_RGB555: 2}[out_format] * width


def all_option_sets():
    """every (out_format, options) the specification allows"""
    out = []
    for fmt in FORMATS:
        for chroma in (0, CHROMA_BILINEAR):
            for extra in ((0, DITHER, MASK_BIT, DITHER | MASK_BIT) if fmt == OUT_RGB555 else (0,)):
                out.append((fmt, chroma | extra))
    return out


def planes(frames, w, h):
    """(n, >= w h 3 / 2) uint8 -> Y (n, h, w), Cb, Cr (n, h / 2, w / 2), int64"""
    frames = np.asarray(frames)
    n = frames.shape[0]
    y = frames[:, :w * h].reshape(n, h, w).astype(np.int64)
    c = frames[:, w * h:w * h * 3 // 2].reshape(n, h // 2, w // 2, 2).astype(np.int64)
    return y, c[..., 1], c[..., 0]                     # NV21: Cr at even bytes, Cb at odd bytes


def bilinear_indices(size):
    """per pixel coordinate p of an axis of `size` pixels: its chroma sample k and the far sample f, clamped"""
    p = np.arange(size)
    k = p >> 1
    f = np.clip(np.where(p & 1, k + 1, k - 1), 0, size // 2 - 1)
    return k, f


def chroma_at_pixels(c, w, h, bilinear):
    """(n, h / 2, w / 2) chroma bytes -> (n, h, w): step 1"""
    kx, fx = bilinear_indices(w)
    ky, fy = bilinear_indices(h)
    near = c[:, ky]
    if not bilinear:
        return near[:, :, kx]
    far = c[:, fy]
    return (9 * near[:, :, kx] + 3 * near[:, :, fx] + 3 * far[:, :, kx] + far[:, :, fx] + 8) >> 4


def matrix_sums(y, cb, cr):
    """step 2 before the shift and the clamp: (..., 3) int64"""
    v = np.stack([y, cb - 128, cr - 128], axis=-1)
    return v @ MATRIX.T + 32768


def rgb(frames, w, h, bilinear):
    """(n, h, w, 3) int64 in 0 .. 255: steps 1 and 2"""
    y, cb, cr = planes(frames, w, h)
    return np.clip(matrix_sums(y, chroma_at_pixels(cb, w, h, bilinear), chroma_at_pixels(cr, w, h, bilinear)) >> 16, 0, 255)


def pictures(frames, w, h, out_format, options=0):
    """(n, h, row bytes) uint8: the pixels of every frame"""
    return pack(rgb(frames, w, h, bool(options & CHROMA_BILINEAR)), out_format, options)


def pack(c, out_format, options=0):
    """step 3: (n, h, w, 3) colours in 0 .. 255 -> (n, h, row bytes) uint8"""
    assert not options & ~7 and (out_format == OUT_RGB555 or not options & (DITHER | MASK_BIT))
    n, h, w, _ = c.shape
    if out_format == OUT_RGB24:
        return c.astype(np.uint8).reshape(n, h, 3 * w)
    if out_format == OUT_RGBX32:
        return np.concatenate([c, np.full((n, h, w, 1), 255, np.int64)], axis=-1).astype(np.uint8).reshape(n, h, 4 * w)
    assert out_format == OUT_RGB555
    if options & DITHER:
        c = np.clip(c + D[np.arange(h)[:, None] & 3, np.arange(w)[None, :] & 3][None, :, :, None], 0, 255)
    c5 = c >> 3
    px = c5[..., 0] | (c5[..., 1] << 5) | (c5[..., 2] << 10) | ((1 << 15) if options & MASK_BIT else 0)
    return np.ascontiguousarray(px.astype("<u2")).view(np.uint8).reshape(n, h, 2 * w)


def place(dst, pics, dst_pitch, dst_stride, offset=0, statuses=None):
    """steps 5 and 6: writes pics (n, h, row bytes) into the flat uint8 buffer `dst` -- picture i at offset + i dst_stride, row y at
    + y dst_pitch, only the row bytes of each row; pictures whose status is not 0 are skipped"""
    n, h, row = pics.shape
    assert dst.ndim == 1 and dst.dtype == np.uint8 and dst_pitch >= row and dst_stride >= (h - 1) * dst_pitch + row
    assert offset % 4 == 0 and dst_pitch % 4 == 0 and dst_stride % 4 == 0
    assert n == 0 or offset + (n - 1) * dst_stride + (h - 1) * dst_pitch + row <= dst.size
    for i in range(n):
        if statuses is not None and statuses[i] != 0:
            continue
        at = offset + i * dst_stride
        for y in range(h):
            dst[at + y * dst_pitch:at + y * dst_pitch + row] = pics[i, y]
    return dst


def convert(frames, w, h, out_format, options=0, statuses=None, dst_pitch=None, fill=0):
    """what convert_device returns for a destination it allocates or is handed as (n, h, dst_pitch), every byte `fill` before"""
    pics = pictures(frames, w, h, out_format, options)
    n, _, row = pics.shape
    pitch = row if dst_pitch is None else dst_pitch
    out = np.full(n * h * pitch, fill, np.uint8)
    return place(out, pics, pitch, h * pitch, 0, statuses).reshape(n, h, pitch)
