"""The streams the STRSPU reader's tests share (tests/test_strspu_demux_ref.py on the CPU, tests/test_gpu_strspu_demux.py on the
device): the crossing of channels, rates, CD speeds, options and audio positions at 48x32 over 2 to 5 frames, what the muxer's
statement (tests/strspu_ref.py) expects the reader to give back, and the damage done to a stream.  Test infrastructure: nothing here
reads the product."""
import functools
import types

import numpy as np

import adpcm_decode_ref as D
import oracle_lib as O
import strspu_demux_ref as R
import strspu_ref as M

W, H = 48, 32
FPS = (15, 1)
OPTION_SETS = (0, M.LOOP, M.NO_LEADING_DUMMY, M.LOOP | M.NO_LEADING_DUMMY)
# (channels, frequency, cd_speed, options, trailing_audio, n_frames, codec, audio id, video id): every channel count x rate x speed;
# each channel count meets all four option sets and both audio positions
CROSSING = tuple((ch, freq, speed, OPTION_SETS[i % 4], bool((i // 2 + i // 6) & 1), 2 + i % 4, i % 3, 0x0001 if i % 3 else 0x0100 + i, 0x8001 if i % 2 else 0x4321 + i)
                 for i, (ch, freq, speed) in enumerate((ch, freq, speed) for ch in (1, 2) for freq in (44100, 32000, 11025) for speed in (1, 2)))


def settings(ch, freq, speed, options=0, trailing=False, codec=0, audio_id=0x0001, video_id=0x8001, width=W, height=H):
    """a psxhip_str_settings_t stand-in for the statements (the GPU tests build the ctypes struct from the same fields)"""
    return types.SimpleNamespace(format=8, video_codec=codec, video_width=width, video_height=height, str_fps_num=FPS[0], str_fps_den=FPS[1],
                                 str_cd_speed=speed, str_video_id=video_id, trailing_audio=int(trailing), audio_channels=ch,
                                 audio_frequency=freq, strspu_options=audio_id | options)


def pcm_for(ch, n, seed, kind=0):
    out = np.zeros(n * max(ch, 1), np.int16)
    for c in range(ch):
        out[c::ch] = O.synth_pcm(seed, c, 0, n, kind)
    return out


@functools.lru_cache(maxsize=None)
def stream(case):
    """(settings, frames, pcm, sectors (n, 2048), rows, K, budgets): one case of CROSSING muxed by the muxer's statement"""
    ch, freq, speed, options, trailing, n_frames, codec, audio_id, video_id = case
    s = settings(ch, freq, speed, options, trailing, codec, audio_id, video_id)
    frames = O.synth_frames(W, H, n_frames, seed=700 + n_frames + ch, amp=6)
    rows, budgets, K = M.schedule(ch, freq, speed, FPS[0], FPS[1], trailing, n_frames)
    pcm = pcm_for(ch, (K + 1) * 28 * (126 // ch) + 100, 800 + ch + speed, kind=n_frames % 3) if ch else np.zeros(0, np.int16)
    sectors, _, rows, K = M.encode_stream(codec, W, H, FPS[0], FPS[1], speed, frames, pcm, channels=ch, frequency=freq, trailing_audio=trailing,
                                          video_id=video_id, options=s.strspu_options)
    sectors.setflags(write=False)
    return s, frames, pcm, sectors, rows, K, budgets


def expected_lanes(pcm, ch, K, options):
    """G: (ch, K B, 16), section 15's lane streams from the PCM: the dummy block, the chain's blocks, the loop flags or the trap block"""
    B = 126 // ch
    d = 0 if options & M.NO_LEADING_DUMMY else 1
    E = M.lanes(pcm, ch, M.units_per_channel(K, ch, options))
    G = np.zeros((ch, K * B, 16), np.uint8)
    for c in range(ch):
        G[c, d:] = E[c][:K * B - d]
        for k in range(K):
            if options & M.LOOP:
                G[c, k * B + B - 1, 1] = 0x03
            elif k == K - 1:
                G[c, k * B + B - 1] = 0
                G[c, k * B + B - 1, 1] = 0x05
    return G


def decode_lanes(G, d):
    """the statement decode of G_c[d:]: int16 PCM, interleaved when there are two lanes (5 filters, 4-bit codes, zero states)"""
    ch = G.shape[0]
    n = G.shape[1] - d
    out = np.zeros((max(n, 0) * 28, ch), np.int16)
    if n > 0:
        for c in range(ch):
            out[:, c] = D.decode_chain(G[c, d:], 4, 5)[0]
    return out.reshape(-1)


@functools.lru_cache(maxsize=None)
def expected_pcm(case):
    s, frames, pcm, sectors, rows, K, budgets = stream(case)
    if not K:
        return np.zeros(0, np.int16)
    out = decode_lanes(expected_lanes(pcm, s.audio_channels, K, s.strspu_options), 0 if s.strspu_options & M.NO_LEADING_DUMMY else 1)
    out.setflags(write=False)
    return out


def run_statement(s, sectors, first_frame, max_frames, bs_stride, capacity, fill=0):
    """the reader's statement over one stream, into buffers of `fill`: dict with bs and units added"""
    bs = np.full((max_frames, bs_stride), fill, np.uint8)
    units = np.full((capacity * 126, 16), fill, np.uint8)
    out = R.demux(s, sectors, first_frame, max_frames, bs, units)
    out.update(bs=bs, units=units)
    return out


# the ends of the format: no audio sector at all (11025 Hz mono is one sector in 48: trailing audio puts none into two frames), one
# audio sector that starts with the dummy block, and a stream without audio
EDGES = ((1, 11025, 2, 0, True, 2, 0, 0x0003, 0x8001), (1, 11025, 2, 0, False, 2, 0, 0x0003, 0x8001), (0, 44100, 2, 0, False, 3, 1, 0x0001, 0x0102))


# ---------------------------------------------------------------------------------------------------------------- damage
MISMATCH_EDITS = {            # clause -> (offset, width, new value as a function of the old)
    "chunk_index": (0x04, 2, lambda v: 1),
    "chunk_count": (0x06, 2, lambda v: 2),
    "bytes_used": (0x0C, 4, lambda v: 2015),
    "channels": (0x10, 2, lambda v: 3 - v),
    "lane_bytes": (0x12, 2, lambda v: v ^ 0x10),
    "frequency": (0x14, 4, lambda v: v + 1),
    "first_sample": (0x18, 4, lambda v: v + 28),
    "dummy_flag": (0x1C, 2, lambda v: v ^ 2),
    "loop_flag": (0x1C, 2, lambda v: v ^ 4),
    "high_flags": (0x1C, 2, lambda v: v | 0x8000),
}


def poke(sec, at, width, value):
    sec[at:at + width] = [(value >> (8 * i)) & 0xFF for i in range(width)]


def audio_positions(rows):
    return np.nonzero(rows[:, 0] == M.KIND_AUDIO)[0]


def damaged(name, sectors, rows, rng):
    """a damaged copy of a stream with at least four audio chunks"""
    out = sectors.copy()
    a = audio_positions(rows)
    assert a.size >= 4
    if name == "removed":
        out = np.delete(out, a[1], axis=0)
    elif name == "duplicated":                       # a second sector with chunk 2's number and other content, further down the stream
        extra = out[a[2]].copy()
        extra[0x20:] = rng.integers(0, 256, 2016, dtype=np.uint8)
        out = np.insert(out, a[3], extra, axis=0)
    elif name == "reordered":
        out[[a[0], a[2]]] = out[[a[2], a[0]]]
        out[[a[1], a[3]]] = out[[a[3], a[1]]]
    elif name == "number-0":
        poke(out[a[1]], 8, 4, 0)
    elif name == "number-max":
        poke(out[a[1]], 8, 4, 0xFFFFFFFF)
    elif name in MISMATCH_EDITS:
        at, width, edit = MISMATCH_EDITS[name]
        old = int.from_bytes(bytes(out[a[2], at:at + width].tolist()), "little")
        poke(out[a[2]], at, width, edit(old))
    else:
        raise KeyError(name)
    return out


def random_sectors(seed, n, audio_id, video_id):
    """n sectors of seeded random bytes, most of them given 60 01 and the audio or the video id at random, chunk numbers and frame
    numbers pulled into a range where they meet each other"""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, (n, 2048), dtype=np.uint8)
    for i in range(n):
        r = rng.integers(0, 8)
        if r < 7:
            out[i, 0:2] = (0x60, 0x01)
            poke(out[i], 2, 2, audio_id if r < 4 else video_id)
        if r < 6:
            poke(out[i], 8, 4, int(rng.integers(0, 12)))
        if r >= 4:
            poke(out[i], 4, 2, int(rng.integers(0, 3)))
            poke(out[i], 6, 2, int(rng.integers(1, 4)))
    return out
