"""The statement of "psxhip display v1" (tests/display_ref.py) held to what the specification promises, on the
CPU: the 32-bit bound of the matrix, the colour round trip through the front-end's matrix over all 2^24 colours, agreement with a
real-valued BT.601 model within a bound derived from the roundings taken, and the small facts of the bilinear weights and of the
dither table.  The kernels are held to the statement (tests/test_gpu_display.py); this file holds the statement."""
import numpy as np
import pytest

import display_ref as R

# BT.601 full range, Kr = 0.299, Kb = 0.114: (Y, cb, cr) coefficients of R, G, B
KR, KB = 0.299, 0.114
KG = 1.0 - KR - KB
EXACT = np.array([[1.0, 0.0, 2 * (1 - KR)], [1.0, -KB * 2 * (1 - KB) / KG, -KR * 2 * (1 - KR) / KG], [1.0, 2 * (1 - KB), 0.0]])


def test_the_coefficients_are_the_exact_ones_rounded_to_16_bits():
    assert np.array_equal(R.MATRIX, np.rint(EXACT * 65536).astype(np.int64))


def test_the_matrix_sums_fit_32_bits():
    """Y in 0 .. 255, |cb|, |cr| <= 128: the largest |sum| of step 2, computed from the coefficients"""
    reach = np.array([255, 128, 128], np.int64)
    worst = int((np.abs(R.MATRIX) @ reach).max()) + 32768
    print("largest |sum| %d" % worst)
    assert worst == 31609088 and worst < 2 ** 31
    # ... and the sums the statement really takes at the extremes stay inside it
    ext = np.array([[y, cb, cr] for y in (0, 255) for cb in (0, 255) for cr in (0, 255)], np.int64)
    assert np.abs(R.matrix_sums(ext[:, 0], ext[:, 1], ext[:, 2])).max() <= worst


def frontend_matrix(r, g, b):
    """RGB24 -> Y, Cb, Cr of the front-end (oracle/frontend_oracle.c:16-19), restated"""
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = np.clip(((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128, 0, 255)
    cr = np.clip(((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128, 0, 255)
    return y, cb, cr


def test_every_colour_survives_the_round_trip_within_one():
    """all 2^24 RGB colours as flat pictures (both chroma modes give a flat plane's own value): front-end matrix, then step 2"""
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    worst = np.zeros(3, np.int64)
    for r in range(256):
        rr = np.full_like(g, r)
        back = np.clip(R.matrix_sums(*frontend_matrix(rr, g, b)) >> 16, 0, 255)
        worst = np.maximum(worst, np.abs(back - np.stack([rr, g, b], axis=-1)).reshape(-1, 3).max(axis=0))
    print("largest round-trip error R, G, B: %s" % worst.tolist())
    assert worst.tolist() == [1, 1, 1]


def float_model(frames, w, h, bilinear):
    """the exact BT.601 inverse on the unrounded chroma, clamped to the bytes' range: (n, h, w, 3) float64"""
    y, cb, cr = (p.astype(np.float64) for p in R.planes(frames, w, h))

    def at_pixels(c):
        kx, fx = R.bilinear_indices(w)
        ky, fy = R.bilinear_indices(h)
        near, far = c[:, ky], c[:, fy]
        if not bilinear:
            return near[:, :, kx]
        return (9 * near[:, :, kx] + 3 * near[:, :, fx] + 3 * far[:, :, kx] + far[:, :, fx]) / 16.0
    v = np.stack([y, at_pixels(cb) - 128.0, at_pixels(cr) - 128.0], axis=-1)
    return np.clip(v @ EXACT.T, 0.0, 255.0)


def error_bound(bilinear):
    """|integer - model| per channel, from the roundings taken.  The final >> 16 with its + 32768 rounds to nearest: 1/2.  A 16-bit
    coefficient is off by |k / 65536 - exact|, times a chroma difference of at most 128.  Bilinear: the chroma byte is rounded
    once more, by at most 1/2, and that passes through the coefficient.  The clamp moves neither value away from the other."""
    coefficient = np.abs(R.MATRIX / 65536.0 - EXACT)[:, 1:].sum(axis=1) * 128.0
    chroma_rounding = 0.5 * np.abs(EXACT)[:, 1:].sum(axis=1) if bilinear else 0.0
    return 0.5 + coefficient + chroma_rounding


@pytest.fixture(scope="module")
def noise():
    w, h, n = 64, 48, 24
    return w, h, np.random.default_rng(18).integers(0, 256, (n, w * h * 3 // 2)).astype(np.uint8)


@pytest.mark.parametrize("bilinear", [False, True])
def test_agreement_with_the_real_valued_model(noise, bilinear):
    w, h, frames = noise
    bound = error_bound(bilinear)
    assert (bound < (1.6 if bilinear else 0.51)).all(), bound          # (the bound itself stays a rounding or two)
    err = R.rgb(frames, w, h, bilinear) - float_model(frames, w, h, bilinear)
    worst = np.abs(err).reshape(-1, 3).max(axis=0)
    print("bilinear %d: largest |error| %s, bound %s" % (bilinear, worst.round(4).tolist(), bound.round(4).tolist()))
    assert (worst <= bound + 1e-9).all()


@pytest.mark.parametrize("bilinear", [False, True])
def test_mean_error_on_noise_is_unbiased(noise, bilinear):
    """Uniform noise in all three planes, every pixel: |mean(integer - model)| < 0.05 per channel, the figure of the scaler's and
    the reconstruction's tests.

    Most of such noise lies outside the RGB gamut, where both values are clamped and the error is 0.  The pixels inside it are
    looked at separately.  Replicate: the same 0.05.  Bilinear: `(s + 8) >> 4` rounds the one tie of sixteen residues upwards, so
    the chroma byte is high by 1/2 * 1/16 = 1/32 on average -- a property of the specification's rounding, not of an
    implementation -- and the matrix passes that on: +1.402/32 on R, -(0.344 + 0.714)/32 on G, +1.772/32 = 0.055 on B.  Inside the
    gamut the mean error is held to that predicted offset within the same 0.05."""
    w, h, frames = noise
    got, model = R.rgb(frames, w, h, bilinear).astype(np.float64), float_model(frames, w, h, bilinear)
    err = (got - model).reshape(-1, 3)
    mean = err.mean(axis=0)
    inside = ((model > 0.5) & (model < 254.5)).reshape(-1, 3)
    mean_inside = np.array([err[inside[:, c], c].mean() for c in range(3)])
    predicted = EXACT[:, 1:].sum(axis=1) / 32.0 if bilinear else np.zeros(3)
    print("bilinear %d: mean error %s; inside the gamut %s (%s of the pixels), predicted %s" % (
        bilinear, mean.round(4).tolist(), mean_inside.round(4).tolist(), inside.mean(axis=0).round(3).tolist(), predicted.round(4).tolist()))
    assert err.shape[0] > 50000 and (inside.sum(axis=0) > 20000).all()
    assert (np.abs(mean) < 0.05).all(), mean
    assert (np.abs(mean_inside - predicted) < 0.05).all(), (mean_inside, predicted)


def test_constant_chroma_gives_the_same_picture_in_both_modes():
    w, h = 48, 32
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (6, w * h * 3 // 2)).astype(np.uint8)
    for i, (cr, cb) in enumerate([(0, 0), (255, 255), (0, 255), (128, 128), (77, 201), (1, 254)]):
        frames[i, w * h::2], frames[i, w * h + 1::2] = cr, cb
    for fmt, options in R.all_option_sets():
        if not options & R.CHROMA_BILINEAR:
            assert np.array_equal(R.pictures(frames, w, h, fmt, options), R.pictures(frames, w, h, fmt, options | R.CHROMA_BILINEAR))


@pytest.mark.parametrize("w,h", [(16, 16), (32, 16), (16, 32)])
def test_bilinear_weights_sum_to_16_everywhere(w, h):
    """the response to one chroma sample of value 16 is that sample's weight at every pixel: the weights of a pixel are 9, 3, 3, 1,
    merged where the far sample is clamped onto the near one (12 and 4 on an edge, 16 in a corner), and sum to 16"""
    cw, ch = w // 2, h // 2
    impulses = np.zeros((cw * ch, ch, cw), np.int64)
    impulses.reshape(cw * ch, cw * ch)[np.arange(cw * ch), np.arange(cw * ch)] = 16
    weights = R.chroma_at_pixels(impulses, w, h, True)               # (sample, y, x)
    assert (weights.sum(axis=0) == 16).all()
    seen = set()
    for y in range(h):
        for x in range(w):
            nz = tuple(sorted(int(v) for v in weights[:, y, x] if v))
            edges = (x in (0, w - 1)) + (y in (0, h - 1))
            assert nz == {0: (1, 3, 3, 9), 1: (4, 12), 2: (16,)}[edges], (x, y, nz)
            seen.add(nz)
            assert weights[(y >> 1) * cw + (x >> 1), y, x] == max(nz)      # the pixel's own sample weighs most
    assert len(seen) == 3


def test_the_dither_table():
    """what is true of the PlayStation GPU's table: the sixteen offsets are -4 .. 3, each twice, and sum to -8 (a mean of -1/2: with
    the truncating >> 3 a dithered ramp keeps its level); every column sums to -2; the 2x2 quadrants sum to -4, 0, 0, -4 (not to
    -2 each); rows 2 and 3 are rows 0 and 1 moved by two columns"""
    assert R.D.sum() == -8
    assert sorted(R.D.reshape(-1).tolist()) == sorted(list(range(-4, 4)) * 2)
    assert R.D.sum(axis=0).tolist() == [-2, -2, -2, -2]
    assert [[int(R.D[qy:qy + 2, qx:qx + 2].sum()) for qx in (0, 2)] for qy in (0, 2)] == [[-4, 0], [0, -4]]
    assert np.array_equal(R.D[2:], np.roll(R.D[:2], 2, axis=1))


def test_dither_mask_and_formats_agree_on_the_colours():
    """the three formats carry the same R, G, B; RGB555 without dither is their top five bits; the mask bit is bit 15 and nothing else"""
    w, h = 32, 16
    frames = np.random.default_rng(9).integers(0, 256, (2, w * h * 3 // 2)).astype(np.uint8)
    for chroma in (0, R.CHROMA_BILINEAR):
        rgb24 = R.pictures(frames, w, h, R.OUT_RGB24, chroma).reshape(2, h, w, 3)
        rgbx = R.pictures(frames, w, h, R.OUT_RGBX32, chroma).reshape(2, h, w, 4)
        assert np.array_equal(rgbx[..., :3], rgb24) and (rgbx[..., 3] == 255).all()
        p = R.pictures(frames, w, h, R.OUT_RGB555, chroma).view("<u2").astype(np.int64)
        assert np.array_equal(np.stack([p & 31, (p >> 5) & 31, (p >> 10) & 31], axis=-1), rgb24 >> 3) and not (p >> 15).any()
        for extra in (0, R.DITHER):
            a = R.pictures(frames, w, h, R.OUT_RGB555, chroma | extra).view("<u2")
            b = R.pictures(frames, w, h, R.OUT_RGB555, chroma | extra | R.MASK_BIT).view("<u2")
            assert np.array_equal(a | 0x8000, b) and not (a & 0x8000).any()
        d = R.pictures(frames, w, h, R.OUT_RGB555, chroma | R.DITHER).view("<u2").astype(np.int64)
        offs = R.D[np.arange(h)[:, None] & 3, np.arange(w)[None, :] & 3]
        assert np.array_equal(d & 31, np.clip(rgb24[..., 0] + offs, 0, 255) >> 3)
        assert (d != p).any()


def test_placement_and_gate_of_the_statement():
    w, h = 16, 16
    frames = np.random.default_rng(3).integers(0, 256, (3, w * h * 3 // 2)).astype(np.uint8)
    pics = R.pictures(frames, w, h, R.OUT_RGB24)
    row, pitch = 3 * w, 3 * w + 4
    stride = h * pitch + 256
    dst = R.place(np.full(8 + 3 * stride, 0xA5, np.uint8), pics, pitch, stride, offset=8, statuses=[0, -5, 0])
    written = np.zeros(dst.size, bool)
    for i in (0, 2):
        for y in range(h):
            at = 8 + i * stride + y * pitch
            assert np.array_equal(dst[at:at + row], pics[i, y])
            written[at:at + row] = True
    assert (dst[~written] == 0xA5).all() and written.sum() == 2 * h * row
    assert np.array_equal(R.convert(frames, w, h, R.OUT_RGB24, statuses=[0, -5, 0])[1], np.zeros((h, row), np.uint8))
