"""Format 8 (STRSPU, "psxhip STRSPU v1") on the GPU: the audio sector kernel alone on random records, whole
streams through psxhip_str_encode_device and psxhip_str_encode_host against the format's restatement (tests/strspu_ref.py: the CPU
oracle's frames, the reference build's SPU encoder where it is there), both ADPCM routes, several streams, strides and canaries, the
PCM edge cases, the SPUI writer as a cross-check of the lanes, the existing reader over the video sectors, and one handle through a
sequence of formats.  Bar: bit-exact, everywhere."""
import numpy as np
import pytest

import oracle_lib as O
import strspu_ref as R
from test_gpu_str_device_settings import _assert_sectors, _pcm, _raw_call, _reference, _threshold

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W, H = 48, 32
RATES = [(44100, 2, 2), (44100, 1, 2), (44100, 2, 1), (32000, 2, 2), (48000, 2, 1), (11025, 1, 2)]
OPTION_SETS = [0, R.LOOP, R.NO_LEADING_DUMMY, R.LOOP | R.NO_LEADING_DUMMY]


def _settings(freq, ch, speed, fps=(15, 1), trailing=False, codec=0, video_id=0x8001, audio_id=0x0001, options=0, fmt=8, **kw):
    from psxavenc_amd import strmux
    return strmux.settings(fmt=fmt, codec=codec, width=W, height=H, fps_num=fps[0], fps_den=fps[1], cd_speed=speed, video_id=video_id,
                           trailing_audio=trailing, channels=ch, frequency=freq, tail=strmux.TAIL_COMPLETE, audio_id=audio_id,
                           spu_loop=bool(options & R.LOOP), spu_no_leading_dummy=bool(options & R.NO_LEADING_DUMMY), **kw)


def _want(s, fps, frames, pcm):
    return R.encode_stream(s.video_codec, W, H, fps[0], fps[1], s.str_cd_speed, frames, pcm, channels=s.audio_channels,
                           frequency=s.audio_frequency, trailing_audio=bool(s.trailing_audio), video_id=s.str_video_id,
                           options=s.strspu_options & 0xFFFFFFFF)


def _plenty(s, n_frames):
    from psxavenc_amd import strmux
    pl = strmux.plan(s, n_frames)
    return (pl.n_audio_sectors + 1) * pl.audio_samples_per_sector + 100


def _units(s, n_frames):
    """(U, K): units every chain of the call encodes, from the plan alone: K audio sectors of 126 / channels blocks per channel, the
    first of them the dummy block unless the option says otherwise"""
    from psxavenc_amd import strmux
    rows = strmux.plan_sectors(s, n_frames)
    K = int((rows[:, 0] == strmux.SECTOR_AUDIO).sum())
    d = 0 if s.strspu_options & R.NO_LEADING_DUMMY else 1
    return (K * (126 // s.audio_channels) - d if K else 0), K


def _device(mux, s, frames, pcm):
    import torch
    d_out, p = mux.encode_device(s, torch.from_numpy(frames).to(DEV), torch.from_numpy(pcm).to(DEV) if pcm.size else None)
    return d_out.cpu().numpy()[0], p


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("ch,K", [(ch, K) for ch in (1, 2) for K in (1, 2, 3)])
def test_audio_sector_kernel_on_random_records(ch, K):
    """psxhip_strspu_audio_sectors_device through the raw binding: random records, the four option combinations, 1 and 3 streams, dense
    and scattered destinations.  d_out starts 4 bytes (and a guard sector) into a noise buffer -- it is promised no more than 4-byte
    alignment -- the streams' units and outputs lie further apart than a stream, and every byte the call does not own stays as it was."""
    import torch
    from psxavenc_amd import _lib, strmux
    L = strmux._bind()
    rng = np.random.default_rng(1000 * ch + K)
    freq = 44100 + 7 * K
    for options in OPTION_SETS:
        opt = options | (0x0001 if not options else 0x1200 + K)
        for S in (1, 3):
            for scattered in (False, True):
                ctx = (ch, K, hex(opt), S, scattered)
                records = rng.integers(0, 256, (S, K * 126, 16), dtype=np.uint8)
                ustride = K * 126 * 16 + 48                              # a multiple of 16, larger than a stream
                h_units = rng.integers(0, 256, 32 + S * ustride, dtype=np.uint8)
                for i in range(S):
                    h_units[32 + i * ustride: 32 + i * ustride + K * 126 * 16] = records[i].reshape(-1)
                slots = (rng.permutation(2 * K + 1)[:K] if scattered else np.arange(K)).astype(np.int32)
                n_slots = 2 * K + 1 if scattered else K
                ostride = (n_slots + 2) * 2048 + 12
                lead = 2048 + 4
                h_out = rng.integers(0, 256, lead + S * ostride, dtype=np.uint8)
                d_units, d_out, d_slots = (torch.from_numpy(a).to(DEV) for a in (h_units, h_out, slots))
                rc = L.psxhip_strspu_audio_sectors_device(0, d_units.data_ptr() + 32, K, ch, freq, opt, S, ustride, d_out.data_ptr() + lead,
                                                          d_slots.data_ptr() if scattered else None, ostride, torch.cuda.current_stream(DEV).cuda_stream)
                torch.cuda.synchronize()
                _lib.check(rc)
                assert np.array_equal(d_units.cpu().numpy(), h_units), ctx
                got = d_out.cpu().numpy()
                want = h_out.copy()
                for i in range(S):
                    sectors = R.audio_sectors(R.records_to_lanes(records[i], K, ch), K, ch, freq, opt)
                    for k in range(K):
                        at = lead + i * ostride + int(slots[k]) * 2048
                        want[at: at + 2048] = sectors[k]
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, "%s: bytes differ at %s" % (ctx, bad[:8].tolist())


def test_audio_sector_builder_through_the_python_mirror():
    import torch
    from psxavenc_amd import strmux
    rng = np.random.default_rng(5)
    records = rng.integers(0, 256, (2, 2 * 126, 16), dtype=np.uint8)
    d_out = strmux.strspu_audio_sectors_device(torch.from_numpy(records).to(DEV), 2, 2, 32000, 0x0007 | strmux.STRSPU_LOOP)
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(d_out[i].cpu().numpy(), R.audio_sectors(R.records_to_lanes(records[i], 2, 2), 2, 2, 32000, 0x0007 | R.LOOP))


# ---------------------------------------------------------------------------------------------------------------- 2. whole streams
@pytest.mark.parametrize("trailing", [False, True], ids=["leading", "trailing"])
@pytest.mark.parametrize("rate", RATES, ids=lambda r: "%d-%dch-%dx" % r)
def test_whole_streams_on_the_device(rate, trailing):
    """every audio rate of the matrix, both audio positions: v2 with the options off and the default ids over three frames, v3 with
    options on and ids off their defaults over four -- every sector against the restatement, with the plan's counts"""
    from psxavenc_amd import strmux
    freq, ch, speed = rate
    case = RATES.index(rate) * 2 + int(trailing)
    mux = strmux.StrMuxer((0,))
    for codec, n_frames, options, video_id, audio_id in ((0, 3, 0, 0x8001, 0x0001), (1, 4, OPTION_SETS[1 + case % 3], 0x4321 + case, 0x0100 + case)):
        s = _settings(freq, ch, speed, trailing=trailing, codec=codec, video_id=video_id, audio_id=audio_id, options=options)
        frames = O.synth_frames(W, H, n_frames, seed=300 + case, amp=6)
        pcm = _pcm(ch, _plenty(s, n_frames), 400 + case, kind=case % 3)
        want, qsum, rows, K = _want(s, (15, 1), frames, pcm)
        got, p = _device(mux, s, frames, pcm)
        _assert_sectors(got, want, (rate, trailing, codec))
        assert (p.n_sectors, p.n_audio_sectors, p.n_frames_encoded, p.quant_scale_sum, p.sector_size) == (rows.shape[0], K, n_frames, qsum, 2048)
        assert np.array_equal(strmux.plan_sectors(s, n_frames), rows)
    mux.close()


@pytest.mark.parametrize("fps", [(30, 1), (30000, 1001)], ids=["30fps", "29.97fps"])
def test_whole_streams_at_other_frame_rates(fps):
    from psxavenc_amd import strmux
    mux = strmux.StrMuxer((0,))
    for i, (freq, ch, speed) in enumerate([(32000, 2, 2), (44100, 1, 2)]):
        s = _settings(freq, ch, speed, fps=fps, trailing=bool(i), codec=2 * i, options=OPTION_SETS[2 + i], audio_id=0x00AA)
        frames = O.synth_frames(W, H, 5, seed=330 + i, amp=7)
        pcm = _pcm(ch, _plenty(s, 5), 430 + i, kind=1)
        want, qsum, rows, K = _want(s, fps, frames, pcm)
        got, p = _device(mux, s, frames, pcm)
        _assert_sectors(got, want, (fps, freq, ch, speed))
        assert (p.n_audio_sectors, p.quant_scale_sum) == (K, qsum)
    mux.close()


def test_lanes_equal_the_recorded_reference_blocks():
    """the two cases of tests/golden/strspu_ref.npz muxed on the device: their audio sectors are the chunks of the blocks the reference
    build's psx_audio_spu_encode gave when the fixture was made -- the audio is pinned where the reference build is absent"""
    from psxavenc_amd import strmux
    mux = strmux.StrMuxer((0,))
    shapes = {2: (44100, 2, 2), 1: (11025, 1, 2)}
    for case, pcm, blocks in R.golden_cases():
        freq, ch, speed = shapes[case["channels"]]
        s = _settings(freq, ch, speed, audio_id=case["options"] & 0xFFFF, options=case["options"])
        n_frames = next(n for n in range(1, 9) if _units(s, n)[1] == case["K"])
        assert _units(s, n_frames) == (blocks.shape[1], case["K"])
        got, p = _device(mux, s, O.synth_frames(W, H, n_frames, seed=9, amp=5), pcm)
        rows = strmux.plan_sectors(s, n_frames)
        audio = got[rows[:, 0] == strmux.SECTOR_AUDIO]
        _assert_sectors(audio, R.audio_sectors(blocks, case["K"], ch, freq, case["options"]), case)
    mux.close()


# ---------------------------------------------------------------------------------------------------------------- 3. both ADPCM routes
@pytest.mark.parametrize("rate,S", [((48000, 2, 1), 1), ((44100, 1, 2), 1), ((48000, 2, 1), 3)], ids=["stereo", "mono", "three-stereo-streams"])
def test_both_adpcm_routes(rate, S):
    """one shape whose chains are shorter than psxhip_adpcm_chunked_threshold (the serial chains kernel) and one at or past it (the
    speculate-and-verify session), on one handle; which route a shape takes is computed from the plan and asserted"""
    import torch
    from psxavenc_amd import strmux
    freq, ch, speed = rate
    s = _settings(freq, ch, speed, options=R.LOOP if S == 3 else 0)
    thr = _threshold(S * ch)
    long_n = next(n for n in range(1, 60) if _units(s, n)[0] >= thr)
    short_n = 3
    assert _units(s, short_n)[0] < thr <= _units(s, long_n)[0] and _units(s, short_n)[1] >= 2
    mux = strmux.StrMuxer((0,))
    for n_frames in (long_n, short_n, long_n):
        U, K = _units(s, n_frames)
        print("rate %s streams %d: n_frames %d, K %d, units per chain %d (threshold %d): %s" % (rate, S, n_frames, K, U, thr, "session" if U >= thr else "serial"))
        frames = np.stack([O.synth_frames(W, H, n_frames, seed=500 + i, amp=4 + i) for i in range(S)])
        pcm = np.stack([_pcm(ch, _plenty(s, n_frames), 510 + i, kind=i % 3) for i in range(S)])
        d_out, p = mux.encode_device(s, torch.from_numpy(frames).to(DEV), torch.from_numpy(pcm).to(DEV))
        qsum = 0
        for i in range(S):
            want, qs, rows, K2 = _want(s, (15, 1), frames[i], pcm[i])
            assert K2 == K
            _assert_sectors(d_out[i].cpu().numpy(), want, (rate, n_frames, i))
            qsum += qs
        assert p.quant_scale_sum == qsum
    mux.close()


# ---------------------------------------------------------------------------------------------------------------- 4. host path, streams, strides
@pytest.mark.parametrize("rate", [(44100, 2, 2), (11025, 1, 2), (48000, 2, 1)], ids=lambda r: "%d-%dch-%dx" % r)
def test_host_path_three_streams_and_strides(rate):
    """psxhip_str_encode_host == psxhip_str_encode_device == the restatement; three streams in one call == three calls; the raw call
    with noise around d_out, d_frames and d_pcm and strides larger than a stream leaves everything it does not own as it was"""
    from psxavenc_amd import strmux
    freq, ch, speed = rate
    case = RATES.index(rate)
    s = _settings(freq, ch, speed, trailing=bool(case & 1), codec=case % 3, options=OPTION_SETS[case % 4], audio_id=0x0002 + case, video_id=0x8000 + case)
    S, n_frames = 3, 4
    frames = np.stack([O.synth_frames(W, H, n_frames, seed=600 + i, amp=3 + 2 * i) for i in range(S)])
    pcm = np.stack([_pcm(ch, _plenty(s, n_frames), 610 + i, kind=i) for i in range(S)])
    mux, single = strmux.StrMuxer((0,)), strmux.StrMuxer((0,))
    got, p = _raw_call(mux, s, frames, pcm, np.random.default_rng(77 + case))
    again, _ = _raw_call(mux, s, frames, pcm, np.random.default_rng(78 + case), use_stream=True)          # (the cached shape)
    qsum = 0
    for i in range(S):
        want, qs, rows, K = _want(s, (15, 1), frames[i], pcm[i])
        _assert_sectors(got[i], want, (rate, i, "three streams"))
        _assert_sectors(again[i], want, (rate, i, "three streams, again"))
        one, p1 = _device(single, s, frames[i], pcm[i])
        _assert_sectors(one, want, (rate, i, "alone"))
        host, ph = mux.encode(s, frames[i], pcm[i])
        _assert_sectors(host, want, (rate, i, "host path"))
        assert ph.quant_scale_sum == p1.quant_scale_sum == qs and ph.n_audio_sectors == K
        qsum += qs
    assert p.quant_scale_sum == qsum
    mux.close()
    single.close()


# ---------------------------------------------------------------------------------------------------------------- 5. edge cases
def test_no_audio_is_the_strv_stream():
    """audio_channels 0: the bytes of format 9 -- of whose 2336-byte sector buffer (the reference loop's, filefmt.c:391-520) the file
    takes the first 2048 bytes (filefmt.c:575,613)"""
    from psxavenc_amd import strmux
    mux = strmux.StrMuxer((0,))
    frames = O.synth_frames(W, H, 5, seed=70, amp=6)
    for codec in (0, 1):
        s8 = _settings(44100, 0, 2, codec=codec, video_id=0x0102)
        s9 = _settings(44100, 0, 2, codec=codec, video_id=0x0102, fmt=9)
        got8, p8 = _device(mux, s8, frames, np.zeros(0, np.int16))
        got9, p9 = _device(mux, s9, frames, np.zeros(0, np.int16))
        assert got8.shape[1] == 2048 and got9.shape[1] == 2336
        _assert_sectors(got8, got9[:, :2048], codec)
        host8, _ = mux.encode(s8, frames)
        _assert_sectors(host8, got8, (codec, "host path"))
        assert (p8.n_sectors, p8.quant_scale_sum) == (p9.n_sectors, p9.quant_scale_sum)
        want, qsum, rows, K = _want(s8, (15, 1), frames, np.zeros(0, np.int16))
        _assert_sectors(got8, want, (codec, "restatement"))
        assert K == 0
    mux.close()


@pytest.mark.parametrize("options", [0, R.NO_LEADING_DUMMY | R.LOOP], ids=["dummy-trap", "nodummy-loop"])
def test_short_and_long_pcm(options):
    """PCM one sample short of the fit, a whole sector short (silence behind it), a lot longer (cut), and a single sample: device path
    and host path against the restatement, which pads and cuts by the format's rule"""
    from psxavenc_amd import strmux
    mux = strmux.StrMuxer((0,))
    for freq, ch, speed in ((44100, 2, 2), (44100, 1, 2)):
        s = _settings(freq, ch, speed, options=options)
        n_frames = 3
        U, K = _units(s, n_frames)
        assert K >= 2
        fit, spc = 28 * U, 28 * (126 // ch)
        frames = O.synth_frames(W, H, n_frames, seed=80, amp=5)
        full = _pcm(ch, fit + 3 * spc, 81, kind=2)
        results = {}
        for n in (fit - 1, fit - spc, fit, fit + 1, fit + 3 * spc, 1):
            pcm = full[:n * ch]
            want, _, _, _ = _want(s, (15, 1), frames, pcm)
            got, _ = _device(mux, s, frames, pcm)
            _assert_sectors(got, want, (freq, ch, n - fit, "device"))
            host, _ = mux.encode(s, frames, pcm)
            _assert_sectors(host, want, (freq, ch, n - fit, "host"))
            results[n] = got
        # longer PCM is cut: the same bytes as the exact fit; shorter PCM differs from it
        assert np.array_equal(results[fit], results[fit + 1]) and np.array_equal(results[fit], results[fit + 3 * spc])
        assert not np.array_equal(results[fit], results[fit - spc])
    mux.close()


@pytest.mark.parametrize("trailing,K", [(True, 0), (False, 1)], ids=["trailing-K0", "leading-K1"])
def test_streams_of_no_and_one_audio_sector(trailing, K):
    """11025 Hz mono at speed 2 is one audio sector in 48: two frames hold none of them with trailing audio and one with leading
    audio -- with the dummy block that one sector is this format's own rule (the SPUI writer would make two chunks of it)"""
    from psxavenc_amd import strmux
    mux = strmux.StrMuxer((0,))
    frames = O.synth_frames(W, H, 2, seed=90, amp=6)
    for options in OPTION_SETS:
        s = _settings(11025, 1, 2, trailing=trailing, options=options, audio_id=0x0003)
        assert _units(s, 2)[1] == K
        pcm = _pcm(1, 4000, 91)
        want, qsum, rows, K2 = _want(s, (15, 1), frames, pcm)
        assert K2 == K and rows.shape[0] == 19 + K
        got, p = _raw_call(mux, s, frames[None], pcm[None], np.random.default_rng(92))
        _assert_sectors(got[0], want, (trailing, hex(options), "device"))
        host, _ = mux.encode(s, frames, pcm)
        _assert_sectors(host, want, (trailing, hex(options), "host"))
        assert p.n_audio_sectors == K
        if K:
            flags = int(want[0, 0x1C])
            assert flags == 1 | (0 if options & R.NO_LEADING_DUMMY else 2) | (4 if options & R.LOOP else 0)
    mux.close()


def test_no_frames_is_an_empty_stream():
    from psxavenc_amd import strmux
    mux = strmux.StrMuxer((0,))
    s = _settings(44100, 2, 2)
    got, p = _raw_call(mux, s, np.zeros((1, 0, W * H * 3 // 2), np.uint8), _pcm(2, 500, 3)[None], np.random.default_rng(4))
    assert got.shape[1] == 0 and p.n_sectors == 0
    mux.close()


# ---------------------------------------------------------------------------------------------------------------- 6. SPUI cross-check
@pytest.mark.parametrize("rate", [(44100, 2, 2), (44100, 1, 2), (48000, 2, 1)], ids=lambda r: "%d-%dch-%dx" % r)
def test_payloads_are_the_spui_file(rate):
    """the concatenated payloads of the audio sectors == the SPUI file psxhip_spu_file_encode_host writes with audio_interleave = L,
    alignment 1 and no loop point over the PCM fitted to 28 U (K >= 2)"""
    from psxavenc_amd import spufile, strmux
    freq, ch, speed = rate
    mux = strmux.StrMuxer((0,))
    for options in OPTION_SETS:
        s = _settings(freq, ch, speed, options=options)
        n_frames = 4
        U, K = _units(s, n_frames)
        assert K >= 2
        frames = O.synth_frames(W, H, n_frames, seed=95, amp=5)
        pcm = _pcm(ch, 28 * U - 40, 96, kind=1)                      # (short of the fit: the fitted PCM ends in silence)
        got, _ = _device(mux, s, frames, pcm)
        rows = strmux.plan_sectors(s, n_frames)
        payload = got[rows[:, 0] == strmux.SECTOR_AUDIO][:, 0x20:].reshape(-1)
        fitted = np.ascontiguousarray(R.fit_pcm(pcm, ch, U).T).reshape(-1)
        fs = spufile.settings(spufile.FORMAT_SPUI, channels=ch, freq=freq, interleave=16 * (126 // ch), alignment=1,
                              enable_loop=bool(options & R.LOOP), no_dummy=bool(options & R.NO_LEADING_DUMMY))
        want = spufile.encode(fs, fitted, device=0)
        assert want.size == K * 2016 and np.array_equal(payload, want), (rate, hex(options))
    mux.close()


# ---------------------------------------------------------------------------------------------------------------- 7. the existing reader
def test_the_reader_takes_the_video_sectors_as_format_9():
    """the reader is unchanged (it keeps refusing format 8: tests/test_str_demux_resources.py); handed the stream as format 9 it counts the audio chunks as `other`
    sectors and reports every frame whole -- rows, sizes and records equal to those of the stream's video sectors alone (a format 9
    stream) and to the oracle's bitstreams"""
    import torch
    from psxavenc_amd import strdemux, strmux
    mux = strmux.StrMuxer((0,))
    reader = strdemux.StrReader(0)
    s = _settings(44100, 2, 2, codec=1, video_id=0x8001, audio_id=0x0001)
    n_frames = 4
    frames = O.synth_frames(W, H, n_frames, seed=97, amp=6)
    pcm = _pcm(2, _plenty(s, n_frames), 98)
    got, p = _device(mux, s, frames, pcm)
    rows = strmux.plan_sectors(s, n_frames)
    K = int((rows[:, 0] == strmux.SECTOR_AUDIO).sum())
    assert K >= 2
    s9 = _settings(44100, 0, 2, codec=1, video_id=0x8001, fmt=9)
    stride = p.max_frame_size
    out = reader.demux_device(s9, torch.from_numpy(got).to(DEV), n_frames, stride, first_frame=1)
    video_only = reader.demux_device(s9, torch.from_numpy(np.ascontiguousarray(got[rows[:, 0] == strmux.SECTOR_VIDEO])).to(DEV), n_frames, stride, first_frame=1)
    torch.cuda.synchronize()
    summary = dict(zip(strdemux.SUMMARY_FIELDS, out["summary"][0].cpu().tolist()))
    assert (summary["n_video"], summary["n_other"], summary["n_audio"], summary["n_complete"], summary["n_rows"]) == (p.n_video_sectors, K, 0, n_frames, n_frames)
    info, info_v = out["info"][0].cpu().numpy(), video_only["info"][0].cpu().numpy()
    status = strdemux.INFO_FIELDS.index("status")
    first = strdemux.INFO_FIELDS.index("first_sector")
    assert (info[:, status] == 0).all() and (info_v[:, status] == 0).all()
    keep = [i for i in range(8) if i != first]
    assert np.array_equal(info[:, keep], info_v[:, keep])
    assert np.array_equal(out["bs"][0].cpu().numpy(), video_only["bs"][0].cpu().numpy())
    assert np.array_equal(out["sizes"][0].cpu().numpy(), video_only["sizes"][0].cpu().numpy())
    budgets = strmux.frame_budgets(s, 0, n_frames)
    bs, res, rc = O.mdec_encode(1, W, H, frames, budgets, stride=stride)
    assert rc == 0
    for f in range(n_frames):
        assert np.array_equal(out["bs"][0, f, :budgets[f]].cpu().numpy(), bs[f, :budgets[f]]), f
    reader.close()
    mux.close()


# ---------------------------------------------------------------------------------------------------------------- 8. one handle
def test_one_handle_through_a_sequence_of_formats():
    """STRCD -> STRSPU -> STRV -> STRSPU with other options -> STRSPU with another channel count on one handle: the handle's cache keys
    on the settings, so every call rebuilds its tables and its unit buffer and gives the right bytes"""
    from psxavenc_amd import strmux
    mux = strmux.StrMuxer((0,))
    n_frames = 6
    frames = O.synth_frames(W, H, n_frames, seed=110, amp=6)

    def xa(fmt, ch):
        s = strmux.settings(fmt=fmt, codec=0, width=W, height=H, channels=ch, tail=strmux.TAIL_COMPLETE)
        pl = strmux.plan(s, n_frames)
        n = pl.n_audio_sectors * pl.audio_samples_per_sector
        pcm = np.zeros((n + 4032) * max(ch, 1), np.int16)
        if ch:
            pcm[:n * ch] = _pcm(ch, n, 111)
        else:
            pcm = np.zeros(0, np.int16)
        got, p = _device(mux, s, frames, pcm)
        want, qsum = _reference(s, (15, 1), frames, pcm)
        _assert_sectors(got, want, ("xa", fmt))
        assert p.quant_scale_sum == qsum

    def spu(ch, options, audio_id):
        s = _settings(44100, ch, 2, options=options, audio_id=audio_id)
        pcm = _pcm(ch, _plenty(s, n_frames), 112 + ch)
        got, p = _device(mux, s, frames, pcm)
        want, qsum, rows, K = _want(s, (15, 1), frames, pcm)
        _assert_sectors(got, want, ("spu", ch, hex(options)))
        assert (p.quant_scale_sum, p.n_audio_sectors) == (qsum, K)

    xa(7, 2)
    spu(2, 0, 0x0001)
    xa(9, 0)
    spu(2, R.LOOP | R.NO_LEADING_DUMMY, 0x0001)
    spu(2, R.LOOP | R.NO_LEADING_DUMMY, 0x0002)
    spu(1, 0, 0x0001)
    xa(7, 2)
    spu(2, 0, 0x0001)
    mux.close()
