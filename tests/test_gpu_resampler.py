"""psxhip_resampler_* on the device against the statement of "psxhip audio front-end v1" (tests/resample_ref.py, DESIGN.md
section 10).  Bar: bit-exact, for every format, channel map and rate pair of the matrix, for any cut of a stream into calls, and
as the input of the device STR muxer."""
import numpy as np
import pytest

import oracle_lib as O
import resample_ref as R

pytestmark = pytest.mark.gpu

RATES = [(48000, 37800), (44100, 37800), (48000, 18900), (22050, 37800), (32000, 44100), (44100, 44100), (44100, 44099),
         (192000, 18900)]
MIX_3_2 = np.array([[12000, -7000, 9000], [-3000, 15000, 11000]], np.int16)
MAPS = [(1, 1, None), (2, 2, None), (2, 1, None), (1, 2, None), (6, 2, None), (3, 2, MIX_3_2)]
_DT = {0: np.int16, 1: np.int16, 2: np.int32, 3: np.int32, 4: np.float32, 5: np.float32}


def _res():
    from psxavenc_amd import resample
    return resample


def _source(fmt, channels, n, seed):
    """(n, channels) of the format's dtype: noise, tones, full scale, and for F32 values beyond +-1, NaN and +-inf"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    base = 0.45 * np.sin(2 * np.pi * (t * (0.013 + 0.007 * np.arange(channels)[None, :]))) + 0.25 * rng.standard_normal((n, channels))
    if fmt in (4, 5):
        x = base.astype(np.float32) * np.float32(1.3)
        k = rng.integers(0, n, (12, channels))
        x[k[:4], np.arange(channels)] = np.nan
        x[k[4:6], np.arange(channels)] = np.inf
        x[k[6:8], np.arange(channels)] = -np.inf
        x[k[8:10], np.arange(channels)] = 1.0
        x[k[10:], np.arange(channels)] = np.float32(-1.75)
        x[:8] = np.float32(0.99997)                             # rint(x * 32768) on the half-way values
        x[8:16] = (np.arange(8, dtype=np.float32)[:, None] + np.float32(0.5)) / np.float32(32768)
        return x
    if fmt in (2, 3):
        x = np.clip(base * 2 ** 31, -2 ** 31, 2 ** 31 - 1).astype(np.int32)
        x[:4] = 2 ** 31 - 1
        x[4:8] = -2 ** 31
        x[8:12] = 32767 * 65536 + 32768                         # (x + 32768) >> 16 = 32768: clamps
        return x
    x = np.clip(base * 40000, -32768, 32767).astype(np.int16)
    x[:6] = 32767
    x[6:12] = -32768
    return x


def _to_device(fmt, x, torch):
    """interleaved (n, ch) or planar (ch, n) CUDA tensor of the format"""
    a = np.ascontiguousarray(x.T if fmt & 1 else x)
    return torch.from_numpy(a).to("cuda:0")


def _want(fmt, x, sch, src, dst, dch, mix, flush=True):
    m = mix if mix is not None else _res().default_matrix(sch, dch)
    P, T, coef = _res().design(src, dst)
    planes = [x[:, k] for k in range(sch)] if fmt & 1 else [x.reshape(-1)]
    return R.statement(fmt, planes, sch, src, dst, m, coef, flush=flush)


def test_bit_exact_over_formats_channel_maps_and_rates():
    import torch
    rs = _res()
    case = 0
    for ri, (src, dst) in enumerate(RATES):
        for mi, (sch, dch, mix) in enumerate(MAPS):
            fmts = range(6) if mi == 1 and ri < 2 else [(ri + mi) % 6]
            for fmt in fmts:
                n = 3000 + 517 * case % 4000
                x = _source(fmt, sch, n, 100 + case)
                r = rs.Resampler(fmt, sch, src, dch, dst, mix=mix)
                got = r.convert_device(_to_device(fmt, x, torch), flush=True).cpu().numpy()
                want = _want(fmt, x, sch, src, dst, dch, mix)
                assert got.shape == want.shape, (src, dst, sch, dch, fmt, got.shape, want.shape)
                bad = np.nonzero((got != want).any(axis=1))[0]
                assert bad.size == 0, (src, dst, sch, dch, fmt, bad[:8].tolist())
                r.close()
                case += 1
    assert case >= 48 + 5 * 2


def test_adversarial_input_for_every_phase_is_exact():
    """a window of +-32767 that follows the taps' signs, for every phase: the exact sum exceeds an int32 (sum |h| up to 2.35 x 32768
    when upsampling); two int32 halves added as int64 give the clamped full-scale value"""
    import torch
    rs = _res()
    for src, dst in [(32000, 37800), (22050, 37800), (48000, 37800)]:
        L, M, P, T, H, _ = R.params(src, dst)
        _, _, coef = rs.design(src, dst)
        gap = 2 * T + 8                                          # outputs far enough apart that their windows do not overlap
        n_of_phase = []
        x = np.zeros(0, np.int16)
        for ph in range(P):
            # the first output of that phase beyond the last window
            n = int(len(x) * L // M) + gap
            while (n * M % L if P == L else (n * M % L) * P // L) != ph:
                n += 1
            i = n * M // L
            need = i + H + 1
            if need > len(x):
                x = np.concatenate([x, np.zeros(need - len(x), np.int16)])
            x[i - H + 1:i + H + 1] = np.where(coef[ph] >= 0, 32767, -32767)
            n_of_phase.append(n)
        x = np.concatenate([x, np.zeros(T, np.int16)])
        r = rs.Resampler(0, 1, src, 1, dst)
        got = r.convert_device(torch.from_numpy(x).to("cuda:0"), flush=True).cpu().numpy()[:, 0]
        want = R.resample_mixed(x.reshape(-1, 1), src, dst, coef)[:, 0]
        assert np.array_equal(got, want), (src, dst, np.nonzero(got != want)[0][:8].tolist())
        assert (got[n_of_phase] == 32767).all()
        big = np.abs(coef.astype(np.int64)).sum(axis=1).max() * 32767
        if src == 32000:
            assert big > 2 ** 31 - 1                             # where one int32 accumulator would wrap
        r.close()


def test_random_chunking_equals_one_call_host_equals_device_and_reset_repeats():
    import torch
    rs = _res()
    rng = np.random.default_rng(77)
    for fmt, sch, dch, src, dst in [(5, 2, 2, 48000, 37800), (2, 6, 2, 44100, 18900), (0, 1, 2, 22050, 37800),
                                    (4, 2, 1, 192000, 18900), (1, 2, 2, 44100, 44100), (0, 2, 2, 44100, 44099)]:
        L, M, P, T, H, _ = R.params(src, dst)
        n = 40000
        x = _source(fmt, sch, n, fmt * 7 + sch)
        want = _want(fmt, x, sch, src, dst, dch, None)
        sizes = [0, 1, max(1, H - 1), 3, 0, 2 * 256 * M // L + 5, 1]
        while sum(sizes) < n:
            sizes.append(int(rng.choice([0, 1, 7, H + 1, 300, 2500, 9000])))
        sizes[-1] -= sum(sizes) - n
        r = rs.Resampler(fmt, sch, src, dch, dst)
        for rep in range(2):
            outs_d, outs_h, done = [], [], 0
            for j, s in enumerate(sizes):
                chunk = x[done:done + s]
                last = j == len(sizes) - 1
                outs_d.append(r.convert_device(_to_device(fmt, chunk, torch), flush=last).cpu().numpy())
                done += s
            r.reset()
            done = 0
            for j, s in enumerate(sizes):
                chunk = np.ascontiguousarray(x[done:done + s].T if fmt & 1 else x[done:done + s])
                outs_h.append(r.convert_host(chunk, flush=j == len(sizes) - 1))
                done += s
            got_d, got_h = np.concatenate(outs_d), np.concatenate(outs_h)
            assert np.array_equal(got_d, want), (fmt, src, dst, rep, np.nonzero((got_d != want).any(axis=1))[0][:8].tolist())
            assert np.array_equal(got_h, want), (fmt, src, dst, rep)
            from psxavenc_amd import _lib
            with pytest.raises(_lib.PsxHipError):                 # flushed: nothing more until reset
                r.convert_host(x[:10].T.copy() if fmt & 1 else x[:10])
            r.reset()
        r.close()


def test_convert_host_small_larger_small_on_one_handle():
    """pieces of 100, 20000 and 100 input frames through convert_host of ONE handle: its staging buffers are allocated, outgrown and
    reused; the pieces' outputs are the statement's over the concatenation"""
    rs = _res()
    fmt, sch, dch, src, dst = 0, 2, 2, 44100, 37800
    pieces = [100, 20000, 100]
    x = _source(fmt, sch, sum(pieces), 5)
    want = _want(fmt, x, sch, src, dst, dch, None)
    r = rs.Resampler(fmt, sch, src, dch, dst)
    outs, done = [], 0
    for j, n in enumerate(pieces):
        outs.append(r.convert_host(np.ascontiguousarray(x[done:done + n]), flush=j == len(pieces) - 1))
        done += n
    assert all(o.shape[0] > 0 for o in outs)
    assert np.array_equal(np.concatenate(outs), want)
    r.close()


def test_chain_48k_f32p_in_hbm_to_the_device_str_muxer():
    """decoded 48 kHz stereo float in HBM -> resampler -> psxhip_str_encode_device (STRCD): the sectors equal encode_file_str over
    the reference's own XA encoder fed the statement's PCM"""
    import torch
    import str_reference_loop as SRL
    from psxavenc_amd import strmux
    rs = _res()
    w, h, n_frames = 320, 240, 150
    s = strmux.settings()
    pl = strmux.plan(s, n_frames)
    n_out = (pl.n_audio_sectors + 2) * 2016 + 100
    n_in = n_out * 48000 // 37800 + 64
    t = np.arange(n_in, dtype=np.float64)
    x = np.stack([0.6 * np.sin(2 * np.pi * 440 * t / 48000) + 0.3 * np.sin(2 * np.pi * 5300 * t / 48000),
                  0.8 * np.sin(2 * np.pi * 1250 * t / 48000 + 0.5)]).astype(np.float32)      # planar (2, n)
    d_x = torch.from_numpy(x).to("cuda:0")
    r = rs.Resampler(rs.PCM_F32P, 2, 48000, 2, 37800)
    d_pcm = r.convert_device(d_x, flush=True)
    pcm = _want(5, x.T, 2, 48000, 37800, 2, None)
    assert np.array_equal(d_pcm.cpu().numpy(), pcm)
    frames = O.synth_frames(w, h, n_frames, seed=33, amp=5)
    mux = strmux.StrMuxer((0,))
    d_out, p = mux.encode_device(s, torch.from_numpy(frames).to("cuda:0"), d_pcm.reshape(1, -1))
    got = d_out.cpu().numpy()[0]
    want, qsum, _ = SRL.encode_file_str(7, 0, w, h, 15, 1, 2, frames, pcm.reshape(-1),
                                        xa_encode=O.ref_xa_encode if O.ref() is not None else None)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, bad[:8].tolist()
    assert p.quant_scale_sum == qsum
    mux.close()
    r.close()


def _long_source(c, j, seed):
    """the long job's input, sample j of channel c, in float32: the same integer hash and float ops on the device and here"""
    h = (np.asarray(j, np.int64) * 2654435761 + c * 40503 + seed * 69069) % (1 << 32)
    return (h >> 8).astype(np.float32) * np.float32(2.4 / (1 << 24)) - np.float32(1.2)


def test_long_job_8_streams_of_60_minutes_spot_checked():
    import torch
    rs = _res()
    src, dst, n = 48000, 37800, 48000 * 3600
    L, M, P, T, H, _ = R.params(src, dst)
    _, _, coef = rs.design(src, dst)
    m = rs.default_matrix(2, 2)
    rng = np.random.default_rng(2024)
    for stream in range(8):
        d_x = torch.empty((2, n), dtype=torch.float32, device="cuda:0")
        j = torch.arange(n, dtype=torch.int64, device="cuda:0")
        for c in range(2):
            hh = (j * 2654435761 + c * 40503 + stream * 69069) % (1 << 32)
            d_x[c] = (hh >> 8).to(torch.float32) * np.float32(2.4 / (1 << 24)) - np.float32(1.2)
        del j, hh
        r = rs.Resampler(rs.PCM_F32P, 2, src, 2, dst, device=0)
        d_out = r.convert_device(d_x, flush=True)
        assert d_out.shape[0] == R.total_outputs(src, dst, n, True) == rs.output_count(src, dst, 0, n, True)
        idx = np.sort(rng.choice(d_out.shape[0], 10000, replace=False)).astype(np.int64)
        idx[:2] = (0, d_out.shape[0] - 1)
        got = d_out[torch.from_numpy(idx).to("cuda:0")].cpu().numpy()
        i, ph = R.positions(idx, L, M, P)
        jj = (i - H + 1)[:, None] + np.arange(T)[None, :]
        valid = (jj >= 0) & (jj < n)
        xs = np.stack([_long_source(c, np.clip(jj, 0, n - 1), stream) for c in range(2)], axis=-1)     # (K, T, 2)
        y = R.mix(R.to_int16(4, xs).reshape(-1, 2), m).reshape(xs.shape)
        y[~valid] = 0
        want = R.filter_windows(y, ph, coef)
        assert np.array_equal(got, want), (stream, np.nonzero((got != want).any(axis=1))[0][:8].tolist())
        r.close()
        del d_x, d_out
        torch.cuda.empty_cache()


def test_wide_channel_counts_at_the_largest_span():
    """output channel counts past stereo (the per-channel store path) at a 16x downsample: 8 -> 8 at 1/16 stages the largest span the
    kernel has (T = 528, about 148 KB of LDS per workgroup)"""
    import torch
    rs = _res()
    eye = lambda n: rs.default_matrix(n, n)                           # noqa: E731
    for fmt, sch, dch, src, dst, mix in [(0, 8, 8, 48000, 3000, None), (5, 6, 6, 96000, 6000, None), (3, 4, 3, 44100, 37800, eye(4)[:3]),
                                         (4, 5, 5, 16000, 256000, None), (1, 8, 7, 48000, 37800, eye(8)[:7])]:
        n = 24000 if src > dst else 3000
        x = _source(fmt, sch, n, 300 + sch * 10 + dch)
        r = rs.Resampler(fmt, sch, src, dch, dst, mix=mix)
        got = r.convert_device(_to_device(fmt, x, torch), flush=True).cpu().numpy()
        want = _want(fmt, x, sch, src, dst, dch, mix)
        assert got.shape == want.shape and got.shape[1] == dch
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (src, dst, sch, dch, fmt, bad[:8].tolist())
        r.close()


def test_a_call_longer_than_one_launch_is_cut_exactly():
    """convert_device cuts a call at 2^28 new samples per launch (the history carries across): one call of 2^28 + 5000 samples equals
    the same stream in two calls cut elsewhere, and outputs around the cut equal the statement"""
    import torch
    rs = _res()
    src, dst, n = 48000, 37800, (1 << 28) + 5000
    L, M, P, T, H, _ = R.params(src, dst)
    _, _, coef = rs.design(src, dst)

    def host_x(j):
        h = (np.asarray(j, np.int64) * 2654435761 + 977) % (1 << 32)
        return ((h >> 16) - 32768).astype(np.int16)

    j = torch.arange(n, dtype=torch.int64, device="cuda:0")
    d_x = (((j * 2654435761 + 977) % (1 << 32)) >> 16).sub_(32768).to(torch.int16)
    del j
    r = rs.Resampler(rs.PCM_S16, 1, src, 1, dst)
    one = r.convert_device(d_x, flush=True)
    assert one.shape[0] == rs.output_count(src, dst, 0, n, True)
    r.reset()
    cut = 100_000_007
    a = r.convert_device(d_x[:cut])
    b = r.convert_device(d_x[cut:], flush=True)
    assert a.shape[0] + b.shape[0] == one.shape[0]
    assert torch.equal(torch.cat([a, b]), one)
    # the outputs whose windows straddle the launch boundary, and a few at the ends
    first = int(rs.output_count(src, dst, 0, 1 << 28)) - 40
    idx = np.concatenate([np.arange(first, first + 80), [0, 1, one.shape[0] - 2, one.shape[0] - 1]]).astype(np.int64)
    got = one[torch.from_numpy(idx).to("cuda:0")].cpu().numpy()
    i, ph = R.positions(idx, L, M, P)
    jj = (i - H + 1)[:, None] + np.arange(T)[None, :]
    y = np.where((jj >= 0) & (jj < n), host_x(np.clip(jj, 0, n - 1)), 0).astype(np.int16)[:, :, None]
    assert np.array_equal(got, R.filter_windows(y, ph, coef))
    r.close()
