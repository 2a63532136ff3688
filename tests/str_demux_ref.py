"""'psxhip STR demux v1' -- the statement the device reader (psxhip_str_demux_device) is held to, bit for bit.

Sequential numpy / plain Python, written from the sector layout of the reference's muxer (chunk header psxavenc/mdec.c:782-820, its place
in the sector :822-829, the EDC libpsxav/cdrom.c:28-41) and defined for arbitrary bytes.  Test infrastructure, like oracle_lib: never
imported by psxavenc_amd/.

A sector is audio / video / other by its subheader and chunk header; a video sector belongs to row frame_index - first_frame; of the
placeable sectors of one (row, chunk_index) the one at the lowest position is placed; a row's fields are its lead's (the sector with
chunk_index 0 at the lowest position, else the row's sector at the lowest position); status bits say what is wrong with a row.
"""
import numpy as np

#            sector size, subheader at, chunk header at
GEOMETRY_OF = {6: (2336, 0, 0x08), 7: (2352, 0x10, 0x18), 9: (2048, None, 0x00)}
CHUNK = 2016
MISSING, DUPLICATE, MISMATCH, RANGE, EDC, GEOMETRY = 1, 2, 4, 8, 16, 32
VIDEO, AUDIO, OTHER = 0, 1, 2
# psxhip_str_frame_info_t / psxhip_str_summary_t as rows of 8 int32
INFO_FIELDS = ("frame_index", "chunk_count", "chunks_placed", "bytes_used", "width", "height", "first_sector", "status")
SUMMARY_FIELDS = ("n_video", "n_audio", "n_other", "first_frame", "n_rows", "n_complete", "n_dropped_video", "n_dropped_audio")

_TABLE = None


def edc(blocks):
    """the CD-ROM EDC (reflected CRC-32, polynomial 0xD8018001, zero start, no final xor; cdrom.c:28-41) of every row of `blocks`"""
    global _TABLE
    if _TABLE is None:
        t = np.arange(256, dtype=np.uint32)
        for _ in range(8):
            t = (t >> 1) ^ np.where(t & 1, np.uint32(0xD8018001), np.uint32(0))
        _TABLE = t
    blocks = np.atleast_2d(np.asarray(blocks, np.uint8))
    c = np.zeros(blocks.shape[0], np.uint32)
    for k in range(blocks.shape[1]):
        c = (c >> 8) ^ _TABLE[(c ^ blocks[:, k]) & 0xFF]
    return c


def _le16(a, at):
    return a[:, at].astype(np.int64) | a[:, at + 1].astype(np.int64) << 8


def _le32(a, at):
    return _le16(a, at) | _le16(a, at + 2) << 16


def edc_bad(fmt, sectors):
    """the EDC rule for video sectors: one bool per sector"""
    sectors = np.asarray(sectors, np.uint8)
    n = sectors.shape[0]
    if fmt == 9 or n == 0:
        return np.zeros(n, bool)
    as_muxed = _le32(sectors, 0x818)
    c1 = edc(sectors[:, 0x10:0x818]).astype(np.int64)
    if fmt == 7:
        return (as_muxed != 0) & (as_muxed != c1)
    on_disc = _le32(sectors, 0x808)
    c2 = edc(sectors[:, 0x000:0x808]).astype(np.int64)
    return ~((as_muxed == c1) | (on_disc == c2) | ((as_muxed == 0) & (on_disc == 0)))


def classify(s, sectors):
    """(audio, video) bool arrays over the sectors of one stream"""
    ssz, sub_at, P = GEOMETRY_OF[s.format]
    n = sectors.shape[0]
    audio = np.zeros(n, bool)
    data = np.ones(n, bool)
    if sub_at is not None:
        sub = sectors[:, sub_at:sub_at + 4].astype(np.int64)
        data = (sub[:, 2] & 0x04) == 0
        if s.audio_channels != 0:
            audio = ~data
            if s.audio_xa_file != -1:
                audio &= sub[:, 0] == s.audio_xa_file
            if s.audio_xa_channel != -1:
                audio &= (sub[:, 1] & 0x1F) == (s.audio_xa_channel & 0x1F)
    video = ~audio & data & (sectors[:, P] == 0x60) & (sectors[:, P + 1] == 0x01)
    if s.str_video_id != -1:
        video &= _le16(sectors, P + 2) == s.str_video_id
    return audio, video


def demux(s, sectors, first_frame, max_frames, bs, xa):
    """One stream.  s: psxhip_str_settings_t-like (format, str_video_id, audio_channels, audio_xa_file, audio_xa_channel, video_width,
    video_height).  sectors: (n, sector size) uint8.  bs: (max_frames, bs_stride) uint8 and xa: (xa_capacity, sector size) uint8 are
    written in place, only where the statement says so.  Returns dict(sizes (max_frames,) int32, info (max_frames, 8) int32, table (n, 4)
    int32, summary (8,) int32)."""
    ssz, sub_at, P = GEOMETRY_OF[s.format]
    sectors = np.asarray(sectors, np.uint8).reshape(-1, ssz)
    n = sectors.shape[0]
    assert bs.shape[0] == max_frames and bs.shape[1] >= CHUNK and xa.shape[1] == ssz
    bs_stride, xa_capacity = bs.shape[1], xa.shape[0]
    audio, video = classify(s, sectors)
    table = np.zeros((n, 4), np.int32)
    table[:] = (OTHER, -1, -1, 0)

    # ---- audio: compacted in stream order
    dropped_audio = 0
    for k, i in enumerate(np.nonzero(audio)[0]):
        table[i] = (AUDIO, -1, k, int(sectors[i, sub_at + 2]) >> 7 & 1)
        if k < xa_capacity:
            xa[k] = sectors[i]
        else:
            dropped_audio += 1

    # ---- video
    vid = np.nonzero(video)[0]
    v = sectors[vid]
    chunk_index, chunk_count, frame_index = _le16(v, P + 4), _le16(v, P + 6), _le32(v, P + 8)
    fields = np.stack([chunk_count, _le32(v, P + 0xC), _le16(v, P + 0x10), _le16(v, P + 0x12), _le32(v, P + 0x14), _le32(v, P + 0x18)], axis=1)
    bad = edc_bad(s.format, v)
    if first_frame < 0:
        first_frame = int(frame_index.min()) if vid.size else 0
    rows = {}
    dropped_video = 0
    for jj, i in enumerate(vid):
        row, ci = int(frame_index[jj]) - first_frame, int(chunk_index[jj])
        if not 0 <= row < max_frames:
            dropped_video += 1
            table[i] = (VIDEO, -1, ci, 0)
            continue
        placeable = ci < int(chunk_count[jj]) and (ci + 1) * CHUNK <= bs_stride
        flags = (0 if placeable else RANGE) | (EDC if bad[jj] else 0)
        table[i] = (VIDEO, row, ci, flags)
        r = rows.setdefault(row, dict(members=[], owner={}, status=0))
        r["members"].append(jj)
        r["status"] |= flags
        if placeable:
            if ci in r["owner"]:
                r["status"] |= DUPLICATE
            else:                                     # (positions ascend: the first one seen is the lowest)
                r["owner"][ci] = jj
                bs[row, ci * CHUNK:(ci + 1) * CHUNK] = v[jj, P + 0x20:P + 0x20 + CHUNK]

    info = np.zeros((max_frames, 8), np.int64)
    info[:, 7] = MISSING
    sizes = np.zeros(max_frames, np.int32)
    for row, r in rows.items():
        zero = [jj for jj in r["members"] if chunk_index[jj] == 0]
        lead = zero[0] if zero else r["members"][0]
        status = r["status"]
        if any((fields[jj] != fields[lead]).any() for jj in r["members"]):
            status |= MISMATCH
        if chunk_index[lead] == 0 and not np.array_equal(v[lead, P + 0x14:P + 0x1C], v[lead, P + 0x20:P + 0x28]):
            status |= MISMATCH
        cc = int(chunk_count[lead])
        if cc == 0 or any(c not in r["owner"] for c in range(cc)):
            status |= MISSING
        w, h = int(fields[lead, 2]), int(fields[lead, 3])
        if (s.video_width != 0 and s.video_width != w) or (s.video_height != 0 and s.video_height != h):
            status |= GEOMETRY
        info[row] = (frame_index[lead], cc, len(r["owner"]), fields[lead, 1], w, h, vid[lead], status)
        sizes[row] = 0 if status & MISSING else cc * CHUNK
    summary = np.array([vid.size, int(audio.sum()), n - vid.size - int(audio.sum()), first_frame if vid.size else 0,
                        max(rows) + 1 if rows else 0, int(((info[:, 7] & MISSING) == 0).sum()), dropped_video, dropped_audio], np.int64)
    return dict(sizes=sizes, info=info.astype(np.uint32).view(np.int32), table=table, summary=summary.astype(np.uint32).view(np.int32))
