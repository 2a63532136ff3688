"""'psxhip STRSPU demux v1' -- the statement the device STRSPU reader (psxhip_strspu_demux_device, psxhip_spu_deinterleave_device,
DESIGN.md section 16) is held to, bit for bit.

Sequential numpy / plain Python, written from section 15's text of the format (the audio chunk header and the lanes behind it) and from
'psxhip STR demux v1' (tests/str_demux_ref.py) for the video half; defined for arbitrary bytes.  Test infrastructure, like oracle_lib:
never imported by psxavenc_amd/.

Symbols are section 15's: ch = audio_channels, B = 126 / ch, L = 16 B, id = strspu_options & 0xFFFF, d = 0 with the no-leading-dummy
option else 1, loop = the loop option.  Video is format 9's; with ch != 0 a sector is audio iff it starts 60 01 and le16(2) == id; its
chunk number is k = le32(8) - 1; of the sectors of one k the one at the lowest position owns it; the owner's lanes become unit
records (k B + b) ch + c.
"""
import types

import numpy as np

import str_demux_ref as V

SECTOR = 2048
LOOP, NO_LEADING_DUMMY = 1 << 16, 1 << 17
MISSING, DUPLICATE, MISMATCH = 1, 2, 4
VIDEO, AUDIO, OTHER = 0, 1, 2
# psxhip_strspu_chunk_info_t / psxhip_strspu_audio_summary_t as rows of int32
CHUNK_FIELDS = ("first_sector", "status", "channels", "lane_bytes", "frequency", "first_sample", "flags", "reserved")
AUDIO_SUMMARY_FIELDS = ("n_chunks", "n_complete", "last_chunk", "reserved")


def _le(sec, at, n):
    return int.from_bytes(bytes(sec[at:at + n].tolist()), "little")


def is_audio(sec, ch, audio_id):
    return ch != 0 and sec[0] == 0x60 and sec[1] == 0x01 and _le(sec, 2, 2) == audio_id


def chunk_number(sec):
    return _le(sec, 8, 4) - 1


def mismatch_clauses(sec, k, ch, frequency, options):
    """the names of the MISMATCH clauses the 32-byte header `sec` of chunk k meets (empty: the header is section 15's)"""
    B = 126 // ch
    d = 0 if options & NO_LEADING_DUMMY else 1
    loop = 1 if options & LOOP else 0
    flags = _le(sec, 0x1C, 2)
    out = []
    if _le(sec, 4, 2) != 0:
        out.append("chunk_index")
    if _le(sec, 6, 2) != 1:
        out.append("chunk_count")
    if _le(sec, 0xC, 4) != 2016:
        out.append("bytes_used")
    if _le(sec, 0x10, 2) != ch:
        out.append("channels")
    if _le(sec, 0x12, 2) != 16 * B:
        out.append("lane_bytes")
    if frequency != 0 and _le(sec, 0x14, 4) != frequency:
        out.append("frequency")
    if _le(sec, 0x18, 4) != (0 if k == 0 else 28 * (k * B - d)):
        out.append("first_sample")
    if (flags >> 1) & 1 != (1 if k == 0 and d else 0):
        out.append("dummy_flag")
    if (flags >> 2) & 1 != loop:
        out.append("loop_flag")
    if flags >> 3:
        out.append("high_flags")
    return out


def deinterleave(chunks, lane_offset, lane_bytes, channels, units, src_chunk=None):
    """psxhip_spu_deinterleave_device for one stream: chunks (n, chunk_stride) uint8; block b of lane c of chunk k -> record
    (k B + b) channels + c of units (records, 16) uint8, in place; src_chunk: per k the row of `chunks`, negative = skipped"""
    B = lane_bytes // 16
    n = len(src_chunk) if src_chunk is not None else chunks.shape[0]
    for k in range(n):
        src = k if src_chunk is None else int(src_chunk[k])
        if src < 0:
            continue
        for c in range(channels):
            lane = chunks[src, lane_offset + c * lane_bytes: lane_offset + (c + 1) * lane_bytes].reshape(B, 16)
            units[k * B * channels + c: (k + 1) * B * channels: channels] = lane


def demux(s, sectors, first_frame, max_frames, bs, units):
    """One stream.  s: psxhip_str_settings_t-like (str_video_id, audio_channels, audio_frequency, strspu_options, video_width,
    video_height).  sectors: (n, 2048) uint8.  bs (max_frames, bs_stride) and units (audio_capacity * 126, 16) uint8 are written in
    place, only where the statement says so.  Returns dict(sizes, info, table, summary (8,) int32, chunk_info (audio_capacity, 8) int32,
    audio_summary (4,) int32)."""
    sectors = np.asarray(sectors, np.uint8).reshape(-1, SECTOR)
    n = sectors.shape[0]
    ch, options = s.audio_channels, s.strspu_options & 0xFFFFFFFF
    audio_id = options & 0xFFFF
    assert ch in (0, 1, 2) and units.shape[0] % 126 == 0 and options >> 18 == 0
    assert ch == 0 or (s.str_video_id != -1 and s.str_video_id & 0xFFFF != audio_id)
    capacity = units.shape[0] // 126
    v = types.SimpleNamespace(format=9, str_video_id=s.str_video_id, audio_channels=0, audio_xa_file=-1, audio_xa_channel=-1,
                              video_width=s.video_width, video_height=s.video_height)
    out = V.demux(v, sectors, first_frame, max_frames, bs, np.zeros((0, SECTOR), np.uint8))
    table, summary = out["table"], out["summary"].copy()

    owner, count = {}, {}
    n_audio = dropped = 0
    for i in range(n):
        if not is_audio(sectors[i], ch, audio_id):
            continue
        assert table[i, 0] == OTHER                      # (the ids differ: never a video sector)
        n_audio += 1
        k = chunk_number(sectors[i])
        flag = _le(sectors[i], 0x1C, 2) & 1
        if not 0 <= k < capacity:
            dropped += 1
            table[i] = (AUDIO, -1, -1, flag)
            continue
        table[i] = (AUDIO, -1, k, flag)
        owner.setdefault(k, i)                           # (positions ascend: the first one seen is the lowest)
        count[k] = count.get(k, 0) + 1
    summary[V.SUMMARY_FIELDS.index("n_audio")] += n_audio
    summary[V.SUMMARY_FIELDS.index("n_other")] -= n_audio
    summary[V.SUMMARY_FIELDS.index("n_dropped_audio")] += dropped

    info = np.zeros((capacity, 8), np.int64)
    info[:, 0], info[:, 1] = -1, MISSING
    last = -1
    if ch:
        src = np.full(capacity, -1, np.int64)
        for k, i in owner.items():
            src[k] = i
        deinterleave(sectors, 0x20, 16 * (126 // ch), ch, units, src)
    for k in sorted(owner):
        sec = sectors[owner[k]]
        status = (DUPLICATE if count[k] > 1 else 0) | (MISMATCH if mismatch_clauses(sec, k, ch, s.audio_frequency, options) else 0)
        flags = _le(sec, 0x1C, 2)
        info[k] = (owner[k], status, _le(sec, 0x10, 2), _le(sec, 0x12, 2), _le(sec, 0x14, 4), _le(sec, 0x18, 4), flags, 0)
        if flags & 1 and last < 0:
            last = k
    audio_summary = np.array([max(owner) + 1 if owner else 0, len(owner), last, 0], np.int32)
    out.update(table=table, summary=summary, chunk_info=info.astype(np.uint32).view(np.int32), audio_summary=audio_summary)
    return out


def lane_streams(units, channels):
    """G: (channels, K B, 16), the lane streams of section 15 from the unit records"""
    return np.stack([units[c::channels] for c in range(channels)])
