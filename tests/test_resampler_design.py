"""psxhip_resampler_design / _output_count (pure host, no GPU) against the closed forms of DESIGN.md section 10, and the statement
(tests/resample_ref.py) against the design properties it was chosen for: tone SNR and alias rejection."""
import math

import numpy as np
import pytest

import resample_ref as R

SRC = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000)
DST = (18900, 37800, 22050, 44100, 48000)
PAIRS = [(s, d) for s in SRC for d in DST if s * 16 >= d and d * 16 >= s] + [(44100, 44099), (16000, 256000), (384000, 24000)]


def _res():
    from psxavenc_amd import resample
    return resample


@pytest.mark.parametrize("src,dst", PAIRS)
def test_design_follows_the_closed_forms(src, dst):
    rs = _res()
    P, T, coef = rs.design(src, dst)
    L, M, P0, T0, H, factor = R.params(src, dst)
    assert (P, T) == (P0, T0)
    if src == dst:
        return
    assert T % 2 == 0 and coef.shape == (P, T)
    assert (coef.astype(np.int64).sum(axis=1) == 32768).all()
    a = np.abs(coef.astype(np.int64))
    assert a[:, :H].sum(axis=1).max() <= 65535 and a[:, H:].sum(axis=1).max() <= 65535
    # every tap within +-1 of the formula, except the ones the rounding residue went to (at most a few per phase)
    want = R.taps_double(src, dst) * 32768.0
    off = np.abs(coef - np.rint(want)) > 1
    assert (off.sum(axis=1) <= 1).all(), (src, dst, np.nonzero(off.sum(axis=1) > 1)[0][:5])
    assert np.abs(coef - want).max() <= T, (src, dst)         # the residue stays small


def test_the_extremes_of_the_range():
    rs = _res()
    assert rs.design(48000, 3000)[:2] == (1, 528)                             # 1/16: T = 528
    assert rs.design(44100, 44099)[0] == 1024                                 # L > 1024: P = 1024
    assert rs.design(44100, 44100)[:2] == (1, 0)                              # bypass


def test_output_count_matches_enumeration_and_splits_add_up():
    rs = _res()
    rng = np.random.default_rng(5)
    for src, dst in [(48000, 37800), (44100, 37800), (48000, 18900), (22050, 37800), (32000, 44100), (44100, 44099),
                     (192000, 18900), (44100, 44100), (8000, 128000)]:
        L, M, P, T, H, _ = R.params(src, dst)
        for N in list(range(0, 3 * max(H, 4) + 5)) + [1000, 4033]:
            if src == dst:
                want_open = want_flush = N
            else:
                n = np.arange(0, 16 * N + 64, dtype=np.int64)
                i = n * M // L
                want_open = int(((i + H) <= N - 1).sum())
                want_flush = int((i <= N - 1).sum())
            assert rs.output_count(src, dst, 0, N) == want_open, (src, dst, N)
            assert rs.output_count(src, dst, 0, N, flush=True) == want_flush, (src, dst, N)
        for trial in range(20):
            cuts = np.sort(rng.integers(0, 200000, rng.integers(1, 12)))
            sizes = np.diff(np.concatenate([[0], cuts, [200000 + trial]]))
            got, done = 0, 0
            for j, s in enumerate(sizes):
                got += rs.output_count(src, dst, done, int(s), flush=j == len(sizes) - 1)
                done += int(s)
            assert got == rs.output_count(src, dst, 0, done, flush=True)


def test_out_of_range_arguments_are_rejected():
    from psxavenc_amd import _lib
    rs = _res()
    # below 1 000 Hz, above 384 000 Hz, just past 1/16, just past 16x (18 900 x 16 = 302 400)
    for src, dst in [(999, 18900), (48000, 384001), (48000, 2999), (18900, 302401)]:
        with pytest.raises(_lib.PsxHipError):
            rs.design(src, dst)
        with pytest.raises(_lib.PsxHipError):
            rs.output_count(src, dst, 0, 100)
    # create checks its arguments before it looks for a device: these are EINVAL with or without one
    for args in [(rs.PCM_S16, 9, 48000, 2, 37800), (rs.PCM_S16, 2, 48000, 9, 37800), (rs.PCM_S16, 3, 48000, 2, 37800),
                 (6, 2, 48000, 2, 37800), (rs.PCM_S16, 2, 48000, 2, 2000)]:
        with pytest.raises(_lib.PsxHipError) as e:
            rs.Resampler(*args)
        assert e.value.code == _lib.PSXHIP_EINVAL, args
    bad = np.array([[30000, 30000, 5536], [0, 16384, 0]], np.int16)            # row 0: sum |m| = 65536
    with pytest.raises(_lib.PsxHipError) as e:
        rs.Resampler(rs.PCM_S16, 3, 48000, 2, 37800, mix=bad)
    assert e.value.code == _lib.PSXHIP_EINVAL


def test_no_device_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from psxavenc_amd import _lib
    rs = _res()
    with pytest.raises(_lib.PsxHipError) as e:
        rs.Resampler(rs.PCM_F32P, 2, 48000, 2, 37800)
    assert e.value.code == _lib.PSXHIP_EDEVICE


# ---------------------------------------------------------------- design properties of the statement
def _tone(src, f, n, amp=0.5):
    t = np.arange(n, dtype=np.float64)
    return np.rint(amp * 32767 * np.sin(2 * np.pi * f * t / src)).astype(np.int16)


def _run(src, dst, x):
    P, T, coef = _res().design(src, dst)
    return R.resample_mixed(x.reshape(-1, 1), src, dst, coef, flush=True)[:, 0]


@pytest.mark.parametrize("src,dst,freqs", [(48000, 37800, (1000, 7000, 12000)), (44100, 37800, (1000, 7000, 12000)),
                                           (48000, 18900, (1000, 4000, 7000)), (44100, 18900, (1000, 4000, 7000))])
def test_tone_snr_is_at_least_75_db(src, dst, freqs):
    n = src // 2
    for f in freqs:
        y = _run(src, dst, _tone(src, f, n)).astype(np.float64)
        m = np.arange(y.size, dtype=np.float64)
        ideal = 0.5 * 32767 * np.sin(2 * np.pi * f * m / dst)
        sl = slice(200, y.size - 200)                                        # away from the stream's edges
        snr = 10 * math.log10((ideal[sl] ** 2).sum() / ((y[sl] - ideal[sl]) ** 2).sum())
        assert snr >= 75, (src, dst, f, snr)


@pytest.mark.parametrize("src", [48000, 44100])
def test_alias_rejection_is_at_least_75_db(src):
    dst = 18900
    for mult in (1.3, 1.5):
        f = mult * dst / 2
        x = _tone(src, f, src // 2)
        y = _run(src, dst, x).astype(np.float64)[200:-200]
        rej = 10 * math.log10((x.astype(np.float64) ** 2).mean() / max((y ** 2).mean(), 1e-12))
        assert rej >= 75, (src, mult, rej)
