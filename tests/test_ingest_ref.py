"""The statement of "psxhip ingest v1" (tests/ingest_ref.py) held to first principles: its coefficients to exact rational arithmetic
written out here, its BT.601 full-range row to the display back-end's constants, its colours to a float64 model, its NV21 path to the
display back-end's statement (tests/display_ref.py, written independently), its box averages and depth reduction to exact rational
rounding.  No library code runs here."""
from fractions import Fraction
import math

import numpy as np
import pytest

import display_ref as DR
import ingest_ref as R

KR_KB = {R.BT601: ("0.299", "0.114"), R.BT709: ("0.2126", "0.0722"), R.SMPTE240M: ("0.212", "0.087"), R.FCC: ("0.30", "0.11"),
         R.BT2020: ("0.2627", "0.0593")}
COMBINATIONS = [(m, full, bits) for m in KR_KB for full in (False, True) for bits in (8, 10)]


def _half_up(q):
    return math.floor(q + Fraction(1, 2))


def _exact(matrix, full, bits):
    """the seven numbers from the specification's rationals, nothing shared with ingest_ref"""
    kr, kb = (Fraction(s) for s in KR_KB[matrix])
    kg = 1 - kr - kb
    s = Fraction(2) ** (bits - 8)
    luma = Fraction(255) / (2 ** bits - 1) if full else Fraction(255) / (219 * s)
    chroma = Fraction(255) / (2 ** bits - 1) if full else Fraction(255) / (224 * s)
    return (_half_up(65536 * luma), _half_up(65536 * chroma * 2 * (1 - kr)), _half_up(65536 * chroma * (-2 * kb * (1 - kb) / kg)),
            _half_up(65536 * chroma * (-2 * kr * (1 - kr) / kg)), _half_up(65536 * chroma * 2 * (1 - kb)),
            0 if full else int(16 * s), 2 ** (bits - 1))


def test_the_twenty_coefficient_rows_are_the_exact_rationals_rounded_half_up():
    assert len(COMBINATIONS) == 20
    for m, full, bits in COMBINATIONS:
        assert R.coefficients(m, full, bits) == _exact(m, full, bits), (m, full, bits)
        assert all(isinstance(v, int) and -2 ** 31 <= v < 2 ** 31 for v in R.coefficients(m, full, bits))


def test_bt601_full_range_8_bit_is_the_display_back_ends_matrix():
    assert R.coefficients(R.BT601, True, 8) == (65536, 91881, -22553, -46802, 116130, 0, 128)
    cy, rv, gu, gv, bu, _, _ = R.coefficients(R.BT601, True, 8)
    assert [[cy, 0, rv], [cy, gu, gv], [cy, bu, 0]] == DR.MATRIX.tolist()


def test_every_partial_sum_fits_int32():
    """|cy (Y - yoff)| + 32768 + |cu| max|Cb - coff| + |cv| max|Cr - coff| over every sample value of the depth (garbage luma above
    the nominal range included): the bound DESIGN.md section 19 states"""
    worst = 0
    for m, full, bits in COMBINATIONS:
        cy, rv, gu, gv, bu, yoff, coff = R.coefficients(m, full, bits)
        top = 2 ** bits - 1
        luma = max(abs(cy * (0 - yoff)), abs(cy * (top - yoff))) + 32768
        c = max(coff, top - coff)
        worst = max(worst, luma + max(abs(rv) * c, (abs(gu) + abs(gv)) * c, abs(bu) * c))
    assert worst < 2 ** 26 < 2 ** 31, worst


def _model(y, cb, cr, matrix, full, bits):
    """float64: normalise, then the textbook inverse matrix"""
    kr, kb = (float(Fraction(s)) for s in KR_KB[matrix])
    kg = 1 - kr - kb
    s = 2.0 ** (bits - 8)
    top = 2.0 ** bits - 1
    if full:
        yn, pb, pr = y / top, (cb - 2 ** (bits - 1)) / top, (cr - 2 ** (bits - 1)) / top
    else:
        yn, pb, pr = (y - 16 * s) / (219 * s), (cb - 128 * s) / (224 * s), (cr - 128 * s) / (224 * s)
    r = yn + 2 * (1 - kr) * pr
    b = yn + 2 * (1 - kb) * pb
    g = (yn - kr * r - kb * b) / kg
    return np.clip(np.stack([r, g, b], axis=-1) * 255, 0, 255)


def _forward(rgb, matrix, full, bits):
    """R'G'B' in 0 .. 1 -> integer Y, Cb, Cr of the given range"""
    kr, kb = (float(Fraction(s)) for s in KR_KB[matrix])
    y = kr * rgb[0] + (1 - kr - kb) * rgb[1] + kb * rgb[2]
    pb, pr = (rgb[2] - y) / (2 * (1 - kb)), (rgb[0] - y) / (2 * (1 - kr))
    s, top = 2 ** (bits - 8), 2 ** bits - 1
    if full:
        return round(y * top), round(pb * top + 2 ** (bits - 1)), round(pr * top + 2 ** (bits - 1))
    return round(16 * s + 219 * s * y), round(128 * s + 224 * s * pb), round(128 * s + 224 * s * pr)


def test_grey_ramps_and_colour_bars_agree_with_a_float_model_within_one_lsb():
    for m, full, bits in COMBINATIONS:
        coef = R.coefficients(m, full, bits)
        top = 2 ** bits - 1
        y = np.arange(top + 1, dtype=np.int64)
        mid = np.full_like(y, 2 ** (bits - 1))
        got = np.clip(R.matrix_sums(y, mid, mid, coef) >> 16, 0, 255)
        assert np.abs(got - _model(y.astype(float), mid.astype(float), mid.astype(float), m, full, bits)).max() <= 1, (m, full, bits)
        grey = np.clip(R.matrix_sums(y, None, None, coef) >> 16, 0, 255)
        assert np.array_equal(grey, got), "a grey source is the luma term alone"
        for bar in [(r, g, b) for r in (0, 1) for g in (0, 1) for b in (0, 1)]:
            yy, cb, cr = (np.array([v], np.int64) for v in _forward(bar, m, full, bits))
            out = np.clip(R.matrix_sums(yy, cb, cr, coef) >> 16, 0, 255)[0]
            assert np.abs(out - 255 * np.array(bar)).max() <= 1, (m, full, bits, bar, out.tolist())
            assert np.abs(out - _model(yy.astype(float), cb.astype(float), cr.astype(float), m, full, bits)[0]).max() <= 1


@pytest.mark.parametrize("bilinear", [False, True])
def test_nv21_bt601_full_range_is_the_display_back_end_byte_for_byte(bilinear):
    """two modules written independently: a misreading one of them has fails here"""
    rng = np.random.default_rng(19)
    for w, h in [(16, 16), (48, 32), (64, 16)]:
        frames = rng.integers(0, 256, (3, w * h * 3 // 2)).astype(np.uint8)
        frames[2, :w * h] = (np.arange(w * h) & 1) * 255
        planes, size = R.layout(R.NV21, w, h)
        assert size == w * h * 3 // 2 and planes == [(0, w), (w * h, w)]
        got = R.convert(frames, R.NV21, w, h, planes, R.BT601, True, R.OUT_RGB24, R.CHROMA_BILINEAR if bilinear else 0)
        want = DR.pictures(frames, w, h, DR.OUT_RGB24, DR.CHROMA_BILINEAR if bilinear else 0)
        assert np.array_equal(got, want.reshape(3, -1))


def test_box_averages_and_depth_reduction_round_the_exact_mean_half_up():
    rng = np.random.default_rng(23)
    for fmt, n, bits in [(R.YUV420P, 1, 8), (R.YUV422P, 2, 8), (R.YUV444P, 4, 8), (R.YUV420P10, 1, 10), (R.YUV422P10, 2, 10), (R.YUV444P10, 4, 10)]:
        top = 2 ** bits - 1
        sx, sy = R.subsampling(fmt)
        rows, cols = (1 if sy else 2), (1 if sx else 2)
        assert rows * cols == n
        cases = [np.full((rows, cols), v, np.int64) for v in (0, 1, 2, 3, top - 1, top)] + \
                [rng.integers(0, top + 1, (rows, cols)) for _ in range(400)]
        for c in cases:
            mean8 = Fraction(int(c.sum()), n) / (4 if bits == 10 else 1)          # the average, scaled 10 -> 8 bits by 1 / 4
            assert int(R.box420(c, fmt)[0, 0]) == min(255, _half_up(mean8)), (fmt, c.tolist())
    # luma: min(255, (v + 2) >> 2)
    v = np.arange(1024, dtype=np.int64)
    planes, size = R.layout(R.YUV420P10, 1024, 2)
    pic = np.zeros(size, np.uint8)
    words = np.concatenate([v, v]).astype("<u2").view(np.uint8)
    pic[:words.size] = words
    y = R.to_yuv420p(pic, R.YUV420P10, 1024, 2, planes)[:1024].astype(np.int64)
    assert [int(t) for t in y] == [min(255, _half_up(Fraction(int(t), 4))) for t in v]
    assert y[1021] == 255 and y[1023] == 255                                       # 1022 / 4 rounds to 256: the clamp


def test_pictures_are_selected_by_index():
    w, h = 6, 4
    planes, size = R.layout(R.GRAY8, w, h)
    src = np.arange(3 * size, dtype=np.uint8).reshape(3, size)
    before = np.full((5, w * h * 3 + 7), 0x5A, np.uint8)
    out = R.convert(src, R.GRAY8, w, h, planes, R.BT601, True, R.OUT_RGB24, 0, index=[2, 2, -1, 0, 1], out=before)
    assert np.array_equal(out[0], out[1]) and (out[2] == 0x5A).all() and (out[:, w * h * 3:] == 0x5A).all()
    assert np.array_equal(out[3, :w * h * 3], np.repeat(src[0], 3))
