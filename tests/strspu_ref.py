"""Format 8, "psxhip STRSPU v1" (DESIGN.md section 15), restated in numpy from the format's text: the sector schedule, the frame
budgets, the video sectors (the CPU oracle's frames behind the chunk header of mdec.c:782-832), the audio lanes (the reference build's
psx_audio_spu_encode where it is there, else the oracle's restatement of it) and the audio chunks.

Test infrastructure (like oracle_lib and str_reference_loop): the checker of the muxer's format 8 and of the audio sector kernel.
Nothing here reads the product."""
import math

import numpy as np

import oracle_lib as O

SECTOR = 2048
LOOP, NO_LEADING_DUMMY = 1 << 16, 1 << 17
KIND_VIDEO, KIND_AUDIO = 0, 1


def layout(channels, frequency, cd_speed):
    """(B, L, spc, p, q): blocks per channel per audio sector, lane bytes, samples per channel per sector, audio share p / q"""
    B = 126 // channels
    spc = 28 * B
    den = spc * 75 * cd_speed
    g = math.gcd(frequency, den)
    return B, 16 * B, spc, frequency // g, den // g


def audio_before(p, q, trailing, n):
    """a(n): audio sectors among the first n sectors"""
    return n * p // q if trailing else -(-n * p // q)


def is_audio(p, q, trailing, n):
    return audio_before(p, q, trailing, n + 1) > audio_before(p, q, trailing, n)


def budget_terms(channels, frequency, cd_speed, fps_num, fps_den):
    """(base, den) of mdec.c:768-775: the video share of 75 x speed sectors a second over the frame rate"""
    if not channels:
        return 75 * cd_speed * fps_den, fps_num
    _, _, _, p, q = layout(channels, frequency, cd_speed)
    return 75 * cd_speed * (q - p) * fps_den, q * fps_num


def frame_budgets(channels, frequency, cd_speed, fps_num, fps_den, n_frames):
    base, den = budget_terms(channels, frequency, cd_speed, fps_num, fps_den)
    out, num = [], 0
    for _ in range(n_frames):
        num += base
        out.append(num // den * 2016)
        num %= den
    return np.array(out, np.int32).reshape(-1)


def schedule(channels, frequency, cd_speed, fps_num, fps_den, trailing, n_frames):
    """The COMPLETE stream: every frame, ending with the last frame's last sector.
    Returns (rows (n, 4) int32 [kind, frame, index, eof], budgets (n_frames,), K)."""
    budgets = frame_budgets(channels, frequency, cd_speed, fps_num, fps_den, n_frames)
    p, q = layout(channels, frequency, cd_speed)[3:] if channels else (0, 1)
    rows = []
    frame, chunk, K, n = 0, 0, 0, 0
    while frame < n_frames:
        if channels and is_audio(p, q, trailing, n):
            rows.append([KIND_AUDIO, -1, K, 0])
            K += 1
        else:
            rows.append([KIND_VIDEO, frame, chunk, 0])
            chunk += 1
            if chunk * 2016 >= budgets[frame]:
                frame, chunk = frame + 1, 0
        n += 1
    rows = np.array(rows, np.int32).reshape(-1, 4)
    audio = np.nonzero(rows[:, 0] == KIND_AUDIO)[0]
    if audio.size:
        rows[audio[-1], 3] = 1
    return rows, budgets, K


def units_per_channel(K, channels, options):
    """U: a channel's K B blocks less the leading dummy"""
    return K * (126 // channels) - (0 if options & NO_LEADING_DUMMY else 1) if K else 0


def spu_blocks(samples):
    """(n / 28, 16): one zero-state SPU chain over the samples (a multiple of 28 of them)"""
    assert samples.size % 28 == 0
    if not samples.size:
        return np.zeros((0, 16), np.uint8)
    enc = O.ref_spu_encode if O.ref() is not None else O.spu_encode
    out, _ = enc(np.ascontiguousarray(samples, np.int16))
    return out.reshape(-1, 16).copy()


def fit_pcm(pcm, channels, U):
    """(channels, 28 U): every channel's samples, cut or completed with silence"""
    pcm = np.asarray(pcm, np.int16).reshape(-1)
    per_ch = pcm.size // channels
    out = np.zeros((channels, 28 * U), np.int16)
    n = min(per_ch, 28 * U)
    for c in range(channels):
        out[c, :n] = pcm[c:per_ch * channels:channels][:n]
    return out


def lanes(pcm, channels, U):
    """E: (channels, U, 16), channel c's encoded blocks"""
    fitted = fit_pcm(pcm, channels, U)
    return np.stack([spu_blocks(fitted[c]) for c in range(channels)])


def le(value, n):
    return [(value >> (8 * i)) & 0xFF for i in range(n)]


def audio_sectors(E, K, channels, frequency, options):
    """(K, 2048): the audio chunks from the channels' encoded blocks E (channels, >= U, 16)"""
    B = 126 // channels
    L = 16 * B
    d = 0 if options & NO_LEADING_DUMMY else 1
    loop = bool(options & LOOP)
    out = np.zeros((K, SECTOR), np.uint8)
    for c in range(channels):
        G = np.zeros((K * B, 16), np.uint8)               # the lane stream: the dummy block, then the chain's blocks
        G[d:] = E[c][:K * B - d]
        for k in range(K):
            last = G[k * B + B - 1]
            if loop:
                last[1] = 0x03
            elif k == K - 1:
                last[:] = 0
                last[1] = 0x05
            out[k, 0x20 + c * L: 0x20 + (c + 1) * L] = G[k * B:(k + 1) * B].reshape(-1)
    for k in range(K):
        hd = out[k]
        hd[0x00:0x02] = [0x60, 0x01]
        hd[0x02:0x04] = le(options & 0xFFFF, 2)
        hd[0x04:0x06] = le(0, 2)
        hd[0x06:0x08] = le(1, 2)
        hd[0x08:0x0C] = le(k + 1, 4)
        hd[0x0C:0x10] = le(2016, 4)
        hd[0x10:0x12] = le(channels, 2)
        hd[0x12:0x14] = le(L, 2)
        hd[0x14:0x18] = le(frequency, 4)
        hd[0x18:0x1C] = le(0 if k == 0 else 28 * (k * B - d), 4)
        hd[0x1C:0x1E] = le((1 if k == K - 1 else 0) | (2 if k == 0 and d else 0) | (4 if loop else 0), 2)
    return out


def records_to_lanes(records, K, channels):
    """unit records in the interleaved order (record u * channels + c = unit u of channel c) -> E (channels, K B, 16)"""
    return np.stack([records[c::channels] for c in range(channels)])


def video_sector(bs_row, result, frame, chunk, budget, width, height, video_id):
    """mdec.c:782-832 with the chunk header at offset 0 (format 9's video sector)"""
    sec = np.zeros(SECTOR, np.uint8)
    sec[0x00:0x02] = [0x60, 0x01]
    sec[0x02:0x04] = le(video_id & 0xFFFF, 2)
    sec[0x04:0x06] = le(chunk, 2)
    sec[0x06:0x08] = le(budget // 2016, 2)
    sec[0x08:0x0C] = le(frame + 1, 4)
    sec[0x0C:0x10] = le(int(result[1]), 4)
    sec[0x10:0x12] = le(width, 2)
    sec[0x12:0x14] = le(height, 2)
    sec[0x14:0x1C] = bs_row[:8]
    sec[0x20:0x20 + 2016] = bs_row[chunk * 2016:(chunk + 1) * 2016]
    return sec


def encode_stream(codec, width, height, fps_num, fps_den, cd_speed, frames, pcm, channels=2, frequency=44100, trailing_audio=False,
                  video_id=0x8001, options=0x0001):
    """Returns (sectors (n, 2048) uint8, quant_scale_sum, rows, K)."""
    n_frames = frames.shape[0]
    rows, budgets, K = schedule(channels, frequency, cd_speed, fps_num, fps_den, trailing_audio, n_frames)
    out = np.zeros((rows.shape[0], SECTOR), np.uint8)
    qsum = 0
    if n_frames:
        stride = int(budgets.max())
        bs, res, rc = O.mdec_encode(codec, width, height, frames, budgets, stride=stride)
        assert rc == 0
        qsum = int(res[:, 0].sum())
    if K:
        U = units_per_channel(K, channels, options)
        audio = audio_sectors(lanes(pcm, channels, U), K, channels, frequency, options)
    for n, (kind, frame, index, _) in enumerate(rows.tolist()):
        if kind == KIND_AUDIO:
            out[n] = audio[index]
        else:
            out[n] = video_sector(bs[frame], res[frame], frame, index, int(budgets[frame]), width, height, video_id)
    return out, qsum, rows, K


def golden_cases():
    """tests/golden/strspu_ref.npz (tests/golden/make_strspu_golden.py): [(case dict, pcm, blocks (channels, U, 16))] -- the lanes the
    reference build's psx_audio_spu_encode gave, recorded"""
    import os
    data = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "strspu_ref.npz"))
    out = []
    for i in range(int(data["n_cases"])):
        case = dict(zip(("channels", "K", "options", "samples", "seed", "kind"), (int(v) for v in data["params_%d" % i])))
        ch, n = case["channels"], case["samples"]
        pcm = np.zeros(n * ch, np.int16)
        for c in range(ch):
            pcm[c::ch] = O.synth_pcm(case["seed"], c, 0, n, case["kind"])
        out.append((case, pcm, data["blocks_%d" % i]))
    return out
