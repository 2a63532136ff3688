"""psxhip_str_encode_device over everything its settings can ask for: every XA layout (mono / stereo, 4 / 8 bit, 18900 / 37800 Hz), both
CD speeds, every frame rate, XA file / channel numbers and video ids off their defaults, both tails, several streams per call, strided
inputs and outputs with canaries around them, the handle's cache, an error return, and inputs of a few frames -- every sector against
the reference's sector loop restated over the CPU oracle (tests/str_reference_loop.py) and against the host-buffer path.
Bar: bit-exact, everywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------- helpers
def _pcm(channels, n, seed, kind=0):
    pcm = np.zeros(n * max(1, channels), np.int16)
    for c in range(channels):
        pcm[c::channels] = O.synth_pcm(seed, c, 0, n, kind) if n else 0
    return pcm


def _xa_encode():
    """the reference's own psx_audio_xa_encode where its build is there, else the oracle's restatement"""
    return O.ref_xa_encode if O.ref() is not None else None


def _assert_sectors(got, want, ctx):
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: sectors differ: %s" % (ctx, bad[:8].tolist())


def _threshold(n_chains):
    from psxavenc_amd import _lib
    return int(_lib.lib().psxhip_adpcm_chunked_threshold(int(n_chains)))


def _units_per_chain(s, n_frames, per_ch):
    """units every ADPCM chain of the call encodes (psxhip_str.cpp, rebuild_shape: units_per_chain = na * units_per_sector / channels), from the plan alone:
    a sector holds 18 sound groups of 8 (4-bit) or 4 (8-bit) units, shared by the channels"""
    from psxavenc_amd import strmux
    rows = strmux.plan_sectors(s, n_frames, per_ch)
    na = int((rows[:, 0] == strmux.SECTOR_AUDIO).sum())
    return na * 18 * (8 if s.audio_bit_depth == 4 else 4) // s.audio_channels, na


def _plenty(s, n_frames):
    """per-channel PCM length: a little more than the plan needs"""
    from psxavenc_amd import strmux
    pl = strmux.plan(s, n_frames)
    return (pl.n_audio_sectors + 2) * pl.audio_samples_per_sector + 100


def _reference(s, fps, frames, pcm):
    import str_reference_loop as R
    from psxavenc_amd import strmux
    f = R.encode_stream_complete if s.tail_mode == strmux.TAIL_COMPLETE else R.encode_file_str
    return f(s.format, s.video_codec, s.video_width, s.video_height, fps[0], fps[1], s.str_cd_speed, frames, pcm,
             channels=s.audio_channels, freq=s.audio_frequency, bits=s.audio_bit_depth, trailing_audio=bool(s.trailing_audio),
             xa_file=s.audio_xa_file, xa_channel=s.audio_xa_channel, video_id=s.str_video_id, xa_encode=_xa_encode())


def _noise(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8)


def _raw_call(mux, s, frames, pcm, rng, use_stream=False):
    """psxhip_str_encode_device through the raw binding with everything the library does not own surrounded by seeded noise.
    frames: (S, n_frames, fsz) uint8; pcm: (S, per_ch * channels) int16 (or per_ch == 0).  d_out, d_frames and d_pcm each start one
    guard row into a larger noise buffer and their stream strides are larger than a stream; after the call every byte outside the S
    output blocks must be what it was, and the inputs byte-identical to what was uploaded.
    use_stream: a non-default stream, with the uploads enqueued on it right before the call.
    Returns (got (S, n_sectors, sector_size), plan)."""
    import torch
    from psxavenc_amd import _lib, strmux
    S, n_frames, fsz = frames.shape
    ch = s.audio_channels
    per_ch = pcm.shape[1] // ch if ch else 0
    pl = strmux.plan(s, n_frames, per_ch)
    ns, ssz = pl.n_sectors, pl.sector_size
    # output: one guard row, then S blocks (n_sectors + 3) sectors apart
    ostride = ((ns + 3) * ssz + 3) & ~3
    h_out = _noise(rng, ssz + S * ostride)
    # frames: one guard frame, then S blocks (n_frames + 2) frames apart, noise between
    fstride = (n_frames + 2) * fsz
    assert fsz % 4 == 0
    h_fr = _noise(rng, fsz + S * fstride)
    for i in range(S):
        h_fr[fsz + i * fstride: fsz + i * fstride + n_frames * fsz] = frames[i].reshape(-1)
    # PCM: a guard of 6 samples, then S blocks 10 samples further apart than a stream (even, so 4-byte aligned)
    plen = per_ch * max(1, ch)
    pstride = (plen + 10 + 1) & ~1
    h_pc = rng.integers(-32768, 32768, 6 + S * pstride, dtype=np.int16)
    for i in range(S):
        h_pc[6 + i * pstride: 6 + i * pstride + plen] = pcm[i][:plen]
    d_out, d_fr, d_pc = (torch.empty(h.size, dtype=torch.from_numpy(h).dtype, device=DEV) for h in (h_out, h_fr, h_pc))
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=DEV) if use_stream else torch.cuda.current_stream(DEV)
    pins = [torch.from_numpy(h).pin_memory() for h in (h_out, h_fr, h_pc)]
    with torch.cuda.stream(st):
        for d, p in zip((d_out, d_fr, d_pc), pins):
            d.copy_(p, non_blocking=True)
    p = strmux.StrPlan()
    has_pcm = bool(ch) and per_ch > 0
    rc = strmux._bind().psxhip_str_encode_device(
        mux._h, C.byref(s), S, d_fr.data_ptr() + fsz, fstride, n_frames, d_pc.data_ptr() + 12 if has_pcm else None,
        pstride if has_pcm else 0, per_ch, d_out.data_ptr() + ssz, ostride, C.byref(p), st.cuda_stream)
    torch.cuda.synchronize()
    _lib.check(rc)
    a_out, a_fr, a_pc = d_out.cpu().numpy(), d_fr.cpu().numpy(), d_pc.cpu().numpy()
    assert np.array_equal(a_fr, h_fr), "the call wrote into d_frames"
    assert np.array_equal(a_pc, h_pc), "the call wrote into d_pcm"
    mask = np.ones(h_out.size, bool)
    for i in range(S):
        mask[ssz + i * ostride: ssz + i * ostride + ns * ssz] = False
    touched = np.nonzero(mask & (a_out != h_out))[0]
    assert touched.size == 0, "bytes outside the streams' sectors were written: offsets %s (guard row %d, stream stride %d, stream %d bytes)" % (
        touched[:8].tolist(), ssz, ostride, ns * ssz)
    got = np.stack([a_out[ssz + i * ostride: ssz + i * ostride + ns * ssz].reshape(ns, ssz) for i in range(S)])
    assert (p.n_sectors, p.sector_size) == (ns, ssz)
    return got, p


# ---------------------------------------------------------------------------------------------------------------- 1. layouts
def _layout_case(case):
    """the 32 audio layouts; codec, trailing audio, XA file / channel and video id vary with the case so that none is at its default"""
    fmt = (6, 7)[case & 1]
    channels = 1 + ((case >> 1) & 1)
    bits = (4, 8)[(case >> 2) & 1]
    freq = (18900, 37800)[(case >> 3) & 1]
    speed = 1 + ((case >> 4) & 1)
    return dict(fmt=fmt, codec=case % 3, width=48, height=32, fps_num=15, fps_den=1, cd_speed=speed, channels=channels, frequency=freq,
                bits=bits, trailing_audio=bool(case & 1), xa_file=2 + 8 * case, xa_channel=1 + case % 31, video_id=0x1234 + 0x0101 * case)


def _layout_frames(s):
    """(n_frames of the long call, n_frames of the short call): the smallest stream whose chains are one sector's worth of units past
    the chunking threshold, and the smallest with two audio sectors"""
    thr = _threshold(s.audio_channels)
    per_sector = 18 * (8 if s.audio_bit_depth == 4 else 4) // s.audio_channels
    long_n = short_n = None
    for n in range(1, 400):
        u, na = _units_per_chain(s, n, _plenty(s, n))
        if short_n is None and na >= 2:
            short_n = n
        if u >= thr + per_sector:
            long_n = n
            break
    assert long_n is not None and short_n is not None
    return long_n, short_n


@pytest.mark.parametrize("case", range(32))
def test_audio_layout_matrix_both_adpcm_routes(case):
    """format x channels x bits x frequency x CD speed, each with a stream long enough for the ADPCM session (speculate and verify)
    and one short enough for the serial chain kernel, on one handle: reference loop, host path, frame count and quant scale sum"""
    import torch
    from psxavenc_amd import strmux
    kw = _layout_case(case)
    s = strmux.settings(**kw)
    long_n, short_n = _layout_frames(s)
    thr = _threshold(s.audio_channels)
    mux = strmux.StrMuxer((0,))
    for which, n_frames in (("long", long_n), ("short", short_n)):
        n = _plenty(s, n_frames)
        units, na = _units_per_chain(s, n_frames, n)
        # the two calls take the two routes (psxhip_str.cpp, audio_leg: chunked = units_per_chain >= threshold), whatever the threshold becomes
        if which == "long":
            assert units >= thr, (units, thr)
        else:
            # (2 or 3 audio sectors everywhere but at interleave 2 with trailing audio, where 3 frames give one and 4 frames four)
            assert units < thr and 2 <= na <= 4, (units, thr, na)
        print("case %2d fmt %d ch %d bits %d freq %5d speed %d interleave %2d: %-5s n_frames %3d audio sectors %2d units/chain %4d (threshold %d)"
              % (case, kw["fmt"], kw["channels"], kw["bits"], kw["frequency"], kw["cd_speed"], strmux.plan(s, n_frames).interleave, which,
                 n_frames, na, units, thr))
        frames = O.synth_frames(48, 32, n_frames, seed=50 + case, amp=6)
        pcm = _pcm(kw["channels"], n, 70 + case, kind=case % 3)
        d_out, p = mux.encode_device(s, torch.from_numpy(frames).to(DEV), torch.from_numpy(pcm).to(DEV))
        got = d_out.cpu().numpy()[0]
        want, qsum, frames_encoded = _reference(s, (15, 1), frames, pcm)
        _assert_sectors(got, want, (case, which, kw))
        assert (p.quant_scale_sum, p.n_frames_encoded) == (qsum, frames_encoded), (case, which)
        host, ph = mux.encode(s, frames, pcm)
        _assert_sectors(host, got, (case, which, "host path"))
        assert (ph.quant_scale_sum, ph.n_frames_encoded) == (qsum, frames_encoded)
    mux.close()


# ---------------------------------------------------------------------------------------------------------------- 2. fuzz
FUZZ_SEED = 20261018
FUZZ_TRIALS = 40
FUZZ_FPS = [(15, 1), (10, 1), (12, 1), (25, 1), (30, 1), (24000, 1001), (30000, 1001)]


@functools.lru_cache(maxsize=None)
def _fuzz_draws():
    rng = np.random.default_rng(FUZZ_SEED)
    draws = []
    for trial in range(FUZZ_TRIALS):
        w, h = [(48, 32), (64, 48), (96, 64)][int(rng.integers(0, 3))]
        draws.append(dict(
            fmt=int(rng.choice([6, 7, 9])), codec=int(rng.integers(0, 3)), w=w, h=h, fps=FUZZ_FPS[int(rng.integers(0, len(FUZZ_FPS)))],
            speed=int(rng.integers(1, 3)), channels=int(rng.integers(0, 3)), bits=int(rng.choice([4, 8])), freq=int(rng.choice([18900, 37800])),
            trailing=bool(rng.integers(0, 2)), n_frames=int(rng.integers(1, 40)), audio=int(rng.integers(0, 5)), amp=int(rng.integers(2, 10)),
            xa_file=int(rng.integers(0, 256)), xa_channel=int(rng.integers(0, 32)), video_id=int(rng.integers(0, 65536)),
            streams=int(rng.integers(1, 4)), kinds=[int(k) for k in rng.integers(0, 3, 3)], noise_seed=int(rng.integers(0, 1 << 31))))
    return draws


@pytest.mark.parametrize("part", range(4))
def test_device_mux_randomised_settings_strides_and_canaries(part):
    """seeded fuzz, 40 trials in four parts of ten (one handle per part), none skipped or caught: container flavour, codec, picture size,
    frame rate, CD speed, audio layout, trailing audio, XA file / channel, video id, frame count, amount of audio (none, less than the
    video, more) and 1..3 streams with their own pictures and audio -- every stream against the reference's sector loop.  Every call
    goes through the raw binding with noise around d_out, d_frames and d_pcm and strides larger than a stream: nothing outside the
    streams' sectors may change and the inputs stay as uploaded.  Every other trial runs on a non-default stream with its uploads
    enqueued on that stream right before the call (the audio leg runs on the handle's own stream behind an event recorded on the
    caller's): that is a smoke test of the ordering -- a missing wait would only show when the copy happens to be slow -- not a proof."""
    from psxavenc_amd import strmux
    mux = strmux.StrMuxer((0,))
    for trial in range(part * 10, part * 10 + 10):
        d = _fuzz_draws()[trial]
        s = strmux.settings(fmt=d["fmt"], codec=d["codec"], width=d["w"], height=d["h"], fps_num=d["fps"][0], fps_den=d["fps"][1],
                            cd_speed=d["speed"], video_id=d["video_id"], trailing_audio=d["trailing"], channels=d["channels"],
                            frequency=d["freq"], bits=d["bits"], xa_file=d["xa_file"], xa_channel=d["xa_channel"])
        p0 = strmux.plan(s, d["n_frames"])              # (every frame rate of the draw leaves a frame at least one sector: no refusal)
        sps, ch, S = p0.audio_samples_per_sector, d["channels"], d["streams"]
        n_audio = [0, sps // 3, sps, 3 * sps + 11, (p0.n_audio_sectors + 3) * sps][d["audio"]] if ch else 0
        frames = np.stack([O.synth_frames(d["w"], d["h"], d["n_frames"], seed=100 + 7 * trial + i, amp=d["amp"]) for i in range(S)])
        pcm = np.stack([_pcm(ch, n_audio, 1000 + 7 * trial + i, kind=d["kinds"][i]) for i in range(S)]).reshape(S, -1)
        got, p = _raw_call(mux, s, frames, pcm, np.random.default_rng(d["noise_seed"]), use_stream=bool(trial & 1))
        qsum = 0
        for i in range(S):
            want, qs, frames_encoded = _reference(s, d["fps"], frames[i], pcm[i])
            _assert_sectors(got[i], want, (trial, i, d))
            assert p.n_frames_encoded == frames_encoded, (trial, i, d)
            qsum += qs
        assert p.quant_scale_sum == qsum, (trial, d)
    mux.close()


# ---------------------------------------------------------------------------------------------------------------- 3. COMPLETE tail
def _complete_pcm(s, n_frames, seed, kind=0):
    """a whole sector's samples for every audio slot, then the zeros the encoder reads past the end (as the host muxer's test)"""
    from psxavenc_amd import strmux
    p = strmux.plan(s, n_frames)
    ch = s.audio_channels
    if not ch:
        return np.zeros(0, np.int16)
    n = p.n_audio_sectors * p.audio_samples_per_sector
    pcm = np.zeros((n + 4032) * ch, np.int16)
    pcm[:n * ch] = _pcm(ch, n, seed, kind)
    return pcm


COMPLETE_CASES = [
    # the three shapes of the host muxer's COMPLETE-tail test, scaled down
    dict(fmt=7, codec=0, width=96, height=64, channels=2, n_frames=40),
    dict(fmt=6, codec=1, width=64, height=48, channels=1, n_frames=40),
    dict(fmt=9, codec=2, width=96, height=64, channels=0, n_frames=30),
    # three layouts of the matrix above: 8-bit, 18900 Hz, CD speed 1
    dict(_layout_case(6 | 8 | 16), n_frames=24),          # STR stereo 8-bit 37800 Hz 2x
    dict(_layout_case(1 | 16), n_frames=33),              # STRCD mono 4-bit 18900 Hz 2x, trailing audio
    dict(_layout_case(1 | 2 | 4 | 8), n_frames=17),       # STRCD stereo 8-bit 37800 Hz 1x: interleave 2, trailing audio
]


@pytest.mark.parametrize("kw", COMPLETE_CASES, ids=lambda kw: "fmt%d-ch%d-%dbit-%d-%dx" % (
    kw["fmt"], kw["channels"], kw.get("bits", 4), kw.get("frequency", 37800), kw.get("cd_speed", 2)))
def test_complete_tail_on_the_device(kw):
    """PSXHIP_STR_TAIL_COMPLETE through the device path: every frame in the stream, EOF on the last audio sector alone"""
    import torch
    from psxavenc_amd import strmux
    kw = dict(kw)
    n_frames = kw.pop("n_frames")
    s = strmux.settings(tail=strmux.TAIL_COMPLETE, **kw)
    frames = O.synth_frames(s.video_width, s.video_height, n_frames, seed=21, amp=6)
    pcm = _complete_pcm(s, n_frames, 9)
    mux = strmux.StrMuxer((0,))
    d_out, p = mux.encode_device(s, torch.from_numpy(frames).to(DEV), torch.from_numpy(pcm).to(DEV) if pcm.size else None)
    want, qsum = _reference(s, (15, 1), frames, pcm)
    _assert_sectors(d_out.cpu().numpy()[0], want, kw)
    assert (p.quant_scale_sum, p.n_frames_encoded) == (qsum, n_frames)
    host, ph = mux.encode(s, frames, pcm)
    _assert_sectors(host, want, (kw, "host path"))
    mux.close()


@pytest.mark.parametrize("kw", [dict(fmt=7, codec=0, width=48, height=32, channels=2, n_frames=40),
                                dict(_layout_case(4 | 8 | 16), n_frames=70)],          # STR mono 8-bit 37800 Hz 2x (long enough for the session)
                         ids=["strcd-stereo-4bit", "str-mono-8bit"])
def test_complete_tail_three_streams_single_batch_and_batch_list(kw):
    """three streams in one contiguous (3, n_frames, frame) tensor: with the COMPLETE tail every frame is encoded, the streams' frames
    are one run in memory and go to the MDEC encoder as ONE batch; the same streams further apart go as a list of batches.  Either way
    every stream equals the oracle and the call on that stream alone."""
    import torch
    from psxavenc_amd import strmux
    kw = dict(kw)
    n_frames = kw.pop("n_frames")
    s = strmux.settings(tail=strmux.TAIL_COMPLETE, **kw)
    S = 3
    frames = np.stack([O.synth_frames(s.video_width, s.video_height, n_frames, seed=30 + i, amp=3 + 2 * i) for i in range(S)])
    pcm = np.stack([_complete_pcm(s, n_frames, 40 + i, kind=i) for i in range(S)])
    mux = strmux.StrMuxer((0,))
    d_frames = torch.from_numpy(frames).to(DEV)
    assert d_frames.stride(0) == n_frames * frames.shape[2]             # what makes the single-batch route
    d_out, p = mux.encode_device(s, d_frames, torch.from_numpy(pcm).to(DEV))
    assert p.n_frames_encoded == n_frames
    got = d_out.cpu().numpy()
    padded, p2 = _raw_call(mux, s, frames, pcm, np.random.default_rng(77))          # frames (n_frames + 2) apart: the batch list
    single = strmux.StrMuxer((0,))
    qsum = 0
    for i in range(S):
        want, qs = _reference(s, (15, 1), frames[i], pcm[i])
        _assert_sectors(got[i], want, (i, "one batch"))
        _assert_sectors(padded[i], want, (i, "batch list"))
        d_one, _ = single.encode_device(s, torch.from_numpy(frames[i]).to(DEV), torch.from_numpy(pcm[i]).to(DEV))
        _assert_sectors(d_one.cpu().numpy()[0], want, (i, "alone"))
        qsum += qs
    assert p.quant_scale_sum == qsum == p2.quant_scale_sum
    mux.close()
    single.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the cache
def test_handle_cache_shape_sequence_same_pointers_new_contents_and_after_an_error():
    """one handle through everything that decides what it keeps between calls (psxhip_str.cpp: settings, frame count, PCM length and stream count
    rebuild the shape, rebuild_shape; d_pcm, PCM stride, chunked or serial the session or chain tables, audio_leg): a sequence of shapes, the same device pointers with new contents on both ADPCM routes, and
    a call after PSXHIP_ENOFIT -- each result against the reference loop"""
    import torch
    from psxavenc_amd import _lib, strmux
    mux = strmux.StrMuxer((0,))
    keep = []                                # (device tensors stay alive: a stale pointer in the handle would read old data, not freed memory)

    def run(s, frames, pcm, ctx, d_frames=None, d_pcm=None):
        if d_frames is None:
            d_frames = torch.from_numpy(frames).to(DEV)
            d_pcm = torch.from_numpy(pcm).to(DEV) if pcm.size else None
        keep.extend([d_frames, d_pcm])
        d_out, p = mux.encode_device(s, d_frames, d_pcm)
        want, qsum, frames_encoded = _reference(s, (15, 1), frames, pcm)
        _assert_sectors(d_out.cpu().numpy()[0], want, ctx)
        assert (p.quant_scale_sum, p.n_frames_encoded) == (qsum, frames_encoded), ctx
        return d_frames, d_pcm

    st4 = strmux.settings(fmt=7, codec=0, width=48, height=32, channels=2, bits=4, xa_file=3, xa_channel=5, video_id=0x4321)
    m8 = strmux.settings(fmt=6, codec=1, width=48, height=32, channels=1, bits=8, frequency=18900, xa_file=9, xa_channel=17)
    vid = strmux.settings(fmt=9, codec=2, width=48, height=32, channels=0)
    other = strmux.settings(fmt=7, codec=2, width=64, height=48, channels=2, bits=4, cd_speed=1, trailing_audio=True)
    long4, short4 = _layout_frames(st4)
    long8, _ = _layout_frames(m8)
    thr = _threshold(2)
    n_long, n_short = _plenty(st4, long4), _plenty(st4, short4)
    assert _units_per_chain(st4, long4, n_long)[0] >= thr > _units_per_chain(st4, short4, n_short)[0]
    assert _units_per_chain(st4, long4, n_long - 1)[0] >= thr and _units_per_chain(m8, long8, _plenty(m8, long8))[0] >= _threshold(1)
    f_long = O.synth_frames(48, 32, long4, seed=3, amp=5)
    pcm_long = _pcm(2, n_long, 4)
    # ---- a sequence of shapes
    run(st4, f_long, pcm_long, "1: stereo 4-bit, long (session)")
    run(st4, f_long[:short4], _pcm(2, n_short, 5), "2: the same settings, short (serial)")
    run(m8, O.synth_frames(48, 32, long8, seed=6, amp=7), _pcm(1, _plenty(m8, long8), 7, kind=2), "3: mono 8-bit, long")
    run(vid, O.synth_frames(48, 32, 11, seed=8, amp=4), np.zeros(0, np.int16), "4: video only")
    run(other, O.synth_frames(64, 48, 13, seed=9, amp=8), _pcm(2, _plenty(other, 13), 10, kind=1), "5: another size and codec")
    run(st4, f_long, pcm_long, "6: the first shape again")
    run(st4, f_long, pcm_long[:-2], "7: the first shape, PCM one sample per channel shorter")
    run(st4, f_long, _pcm(2, n_long, 11, kind=1), "8: the first shape from another d_pcm tensor")
    # (the shape is now cached with shape 8's d_pcm: the same shape from yet another tensor -- only the pointer differs)
    d_frames, d_pcm = run(st4, f_long, _pcm(2, n_long, 12, kind=2), "9: the same shape again, from a third d_pcm tensor")
    # ---- same pointers, new contents: the session route ...
    f2, pcm2 = O.synth_frames(48, 32, long4, seed=13, amp=9), _pcm(2, n_long, 14, kind=1)
    d_frames.copy_(torch.from_numpy(f2))
    d_pcm.copy_(torch.from_numpy(pcm2).reshape(d_pcm.shape))
    run(st4, f2, pcm2, "same pointers, new contents (session)", d_frames, d_pcm)
    # ... and the serial route
    f_short, pcm_short = O.synth_frames(48, 32, short4, seed=15, amp=5), _pcm(2, n_short, 16)
    d_frames, d_pcm = run(st4, f_short, pcm_short, "short, first contents")
    f3, pcm3 = O.synth_frames(48, 32, short4, seed=17, amp=8), _pcm(2, n_short, 18, kind=2)
    d_frames.copy_(torch.from_numpy(f3))
    d_pcm.copy_(torch.from_numpy(pcm3).reshape(d_pcm.shape))
    run(st4, f3, pcm3, "same pointers, new contents (serial)", d_frames, d_pcm)
    # ---- after an error: 320x240 at 30 fps, 1x, stereo 8-bit 37800 Hz -- interleave 2, 1.25 sectors per frame: frame 0 gets ONE sector,
    #      2016 bytes, and a 320x240 frame's 1800 blocks take 12 bits each at the least (2700 bytes) at any quant scale
    big = strmux.settings(fmt=7, codec=0, width=320, height=240, fps_num=30, cd_speed=1, channels=2, bits=8, frequency=37800)
    assert strmux.frame_budgets(big, 0, 1).tolist() == [2016]
    f_big = O.synth_frames(320, 240, 6, seed=19, amp=4)
    pcm_big = _pcm(2, _plenty(big, 6), 20)
    with pytest.raises(_lib.PsxHipError) as e:
        mux.encode_device(big, torch.from_numpy(f_big).to(DEV), torch.from_numpy(pcm_big).to(DEV))
    assert e.value.code == _lib.PSXHIP_ENOFIT and "frame 0 of stream 0" in str(e.value), str(e.value)
    with pytest.raises(_lib.PsxHipError) as e:
        mux.encode(big, f_big, pcm_big)
    assert e.value.code == _lib.PSXHIP_ENOFIT, str(e.value)
    run(st4, f_long, pcm_long, "the first shape after PSXHIP_ENOFIT")
    run(st4, f_short, pcm_short, "a short shape after that")
    mux.close()


# ---------------------------------------------------------------------------------------------------------------- 5. tiny inputs
@pytest.mark.parametrize("fmt,channels", [(7, 2), (9, 0)], ids=["strcd-stereo", "strv"])
def test_streams_of_one_to_three_frames(fmt, channels):
    """1, 2 and 3 frames with no audio, a third of a sector and three sectors of it: device path (noise around the output), host path,
    reference loop and the plan's sector count agree"""
    from psxavenc_amd import strmux
    s = strmux.settings(fmt=fmt, codec=1, width=48, height=32, channels=channels, xa_file=4, xa_channel=2, video_id=0x0102)
    sps = strmux.plan(s, 1).audio_samples_per_sector
    mux = strmux.StrMuxer((0,))
    for n_frames in (1, 2, 3):
        for n_audio in ((0, sps // 3, 3 * sps) if channels else (0,)):
            ctx = (fmt, n_frames, n_audio)
            frames = O.synth_frames(48, 32, n_frames, seed=60 + n_frames, amp=6)
            pcm = _pcm(channels, n_audio, 61)
            want, qsum, frames_encoded = _reference(s, (15, 1), frames, pcm)
            got, p = _raw_call(mux, s, frames[None], pcm[None], np.random.default_rng(n_frames * 10 + n_audio))
            assert strmux.plan(s, n_frames, n_audio).n_sectors == want.shape[0] == p.n_sectors, ctx
            _assert_sectors(got[0], want, ctx)
            assert (p.quant_scale_sum, p.n_frames_encoded) == (qsum, frames_encoded), ctx
            host, ph = mux.encode(s, frames, pcm)
            _assert_sectors(host, want, (ctx, "host path"))
            assert (ph.quant_scale_sum, ph.n_frames_encoded) == (qsum, frames_encoded), ctx
    mux.close()


@pytest.mark.parametrize("trailing", [False, True])
def test_no_frames_at_all(trailing):
    """n_frames == 0: the reference asserts in its decoder, so the host path's bytes are the expectation; the plan holds audio
    sectors and empty audio slots only, and where it holds nothing the call returns OK and leaves d_out as it was (_raw_call checks
    every byte outside the streams' sectors -- here: every byte)"""
    from psxavenc_amd import strmux
    s = strmux.settings(fmt=7, codec=0, width=48, height=32, channels=2, trailing_audio=trailing, xa_file=4, xa_channel=2)
    sps = strmux.plan(s, 1).audio_samples_per_sector
    mux = strmux.StrMuxer((0,))
    frames = np.zeros((1, 0, 48 * 32 * 3 // 2), np.uint8)
    seen = set()
    for n_audio in (0, sps // 3, 3 * sps):
        pcm = _pcm(2, n_audio, 62)
        rows = strmux.plan_sectors(s, 0, n_audio)
        assert set(rows[:, 0].tolist()) <= {strmux.SECTOR_AUDIO, strmux.SECTOR_EMPTY}, rows.tolist()
        got, p = _raw_call(mux, s, frames, pcm[None], np.random.default_rng(n_audio + 1))
        assert p.n_sectors == rows.shape[0] and p.n_frames_encoded == 0 and p.quant_scale_sum == 0
        host, ph = mux.encode(s, frames[0], pcm)
        _assert_sectors(got[0], host, (trailing, n_audio))
        seen.add(rows.shape[0])
    # the slot before any frame is an audio slot without trailing audio (one sector: audio, or empty when there is none) and a video
    # slot with it (nothing at all)
    assert seen == ({0} if trailing else {1}), seen
    mux.close()
