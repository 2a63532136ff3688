"""Streams for the STR reader's tests (tests/test_str_demux_ref.py on the CPU, tests/test_gpu_str_demux.py on the device): a seeded
synthetic corpus that reaches every rule of 'psxhip STR demux v1' (tests/str_demux_ref.py), and targeted edits of clean streams.
Test infrastructure only."""
import numpy as np

import str_demux_ref as D


def pcm_for(channels, n, seed, kind=0):
    import oracle_lib as O
    pcm = np.zeros(n * max(1, channels), np.int16)
    for c in range(channels):
        pcm[c::channels] = O.synth_pcm(seed, c, 0, n, kind) if n else 0
    return pcm


def put16(sec, at, v):
    sec[at] = v & 0xFF
    sec[at + 1] = (v >> 8) & 0xFF


def put32(sec, at, v):
    put16(sec, at, v & 0xFFFF)
    put16(sec, at + 2, (v >> 16) & 0xFFFF)


def refresh_edc(fmt, sectors, which, placement="muxed"):
    """write the EDC of the sectors `which` (index array) where the muxer ('muxed'; STRCD's only place) or a disc ('disc', STR) has it"""
    which = np.atleast_1d(np.asarray(which, np.int64))
    if fmt == 9 or which.size == 0:
        return
    if placement == "muxed":
        c = D.edc(sectors[which, 0x10:0x818])
        at = 0x818
    else:
        assert fmt == 6
        sectors[which, 0x818:0x81C] = 0
        c = D.edc(sectors[which, 0x000:0x808])
        at = 0x808
    for k in range(4):
        sectors[which, at + k] = (c >> (8 * k)) & 0xFF


def video_sector(fmt, frame_index, ci, cc, bytes_used, w, h, payload, video_id=0x8001, xa_file=1, xa_channel=0):
    """one video sector as the muxer lays it out (mdec.c:782-832, filefmt.c:73-91), without its EDC"""
    ssz, sub_at, P = D.GEOMETRY_OF[fmt]
    sec = np.zeros(ssz, np.uint8)
    if sub_at is not None:
        sec[sub_at:sub_at + 4] = (xa_file, xa_channel & 0x1F, 0x48, 0)
        sec[sub_at + 4:sub_at + 8] = sec[sub_at:sub_at + 4]
    put16(sec, P, 0x0160)
    put16(sec, P + 2, video_id)
    put16(sec, P + 4, ci)
    put16(sec, P + 6, cc)
    put32(sec, P + 8, frame_index)
    put32(sec, P + 0xC, bytes_used)
    put16(sec, P + 0x10, w)
    put16(sec, P + 0x12, h)
    sec[P + 0x20:P + 0x20 + 2016] = payload
    return sec


def synthetic(fmt, seed, n=3000, first=1000, window=260, width=48, height=32):
    """n sectors of kinds at random positions (audio share about 0.4 where the format has audio: the ordinals, not a schedule, drive
    the prefix count); frame indices from [first - 30, first - 30 + window): read with first_frame = `first` and fewer than window - 30 rows, both
    ends drop; chunk counts 1 .. 11 per frame, chunk indices up to and beyond them; a few sectors with another chunk_count / size /
    BS-header copy / EDC placement / bad EDC / video id / XA file / XA channel.  Returns (sectors (n, sector size), dict of index arrays
    by what was done)."""
    rng = np.random.default_rng(seed)
    ssz, sub_at, P = D.GEOMETRY_OF[fmt]
    sectors = np.zeros((n, ssz), np.uint8)
    # every third frame whole (each chunk once), the others a random draw of chunk indices, up to and beyond their count
    specs = []
    for f in range(first - 30, first - 30 + window):
        cc = 1 + f % 11
        specs += [(f, ci) for ci in (range(cc) if f % 3 == 0 else rng.integers(cc + 2, size=int(rng.integers(1, cc + 3))))]
    specs = [specs[k] for k in rng.permutation(len(specs))][:n * 6 // 10]
    kind = np.where(rng.random(n) < (0.8 if sub_at is not None else 0.0), 1, 2)
    kind[rng.choice(n, len(specs), replace=False)] = 0
    heads = {}                                        # frame -> the 8 bytes its BS header copy carries
    done = dict(video=[], audio=[], disc=[], zero_edc=[], bad_edc=[], foreign=[])
    for i in range(n):
        if kind[i] == 0:
            f, ci = specs[len(done["video"])]
            ci = int(ci)
            cc = 1 + f % 11
            w, h, used = width, height, 4 * (f % 1000) + 8
            payload = rng.integers(0, 256, 2016).astype(np.uint8)
            head = heads.setdefault(f, rng.integers(0, 256, 8).astype(np.uint8))
            if ci == 0:
                payload[:8] = head
            roll = rng.random()
            if roll < 0.01:
                cc += 1
            elif roll < 0.02:
                used += 4
            elif roll < 0.03:
                head = head ^ np.uint8(1)
            elif roll < 0.06 and ci == 0:
                payload[3] ^= 0x10
            if f % 13 == 0:
                w += 16
            sec = video_sector(fmt, f, ci, cc, used, w, h, payload, video_id=0x8001 if rng.random() > 0.01 else 0x8002)
            sec[P + 0x14:P + 0x1C] = head
            sectors[i] = sec
            done["video"].append(i)
        elif kind[i] == 1:
            sec = rng.integers(0, 256, ssz).astype(np.uint8)
            roll = rng.random()
            file, channel = (1, 0) if roll > 0.1 else ((2, 0) if roll > 0.05 else (1, 3))
            if roll <= 0.1:
                done["foreign"].append(i)
            sec[sub_at:sub_at + 4] = (file, channel | (0x20 if rng.random() < 0.3 else 0), 0x64 | (0x80 if rng.random() < 0.2 else 0), 0x01)
            sectors[i] = sec
            done["audio"].append(i)
        elif rng.random() < 0.5:
            sectors[i] = rng.integers(0, 256, ssz).astype(np.uint8)
            if sub_at is not None:
                sectors[i, sub_at + 2] &= 0xFB            # (else it might be audio)
            sectors[i, P] = 0x61
    video = np.array(done["video"], np.int64)
    refresh_edc(fmt, sectors, video)
    if fmt != 9:
        roll = rng.random(video.size)
        if fmt == 6:
            done["disc"] = video[roll < 0.2]
            refresh_edc(fmt, sectors, done["disc"], "disc")
            done["zero_edc"] = video[(roll >= 0.2) & (roll < 0.3)]
            sectors[done["zero_edc"], 0x808:0x80C] = 0
        else:
            done["zero_edc"] = video[roll < 0.1]
        sectors[done["zero_edc"], 0x818:0x81C] = 0
        done["bad_edc"] = video[roll > 0.96]
        sectors[done["bad_edc"], P + 0x20 + 100] ^= 0x04
    return sectors, {k: np.asarray(v, np.int64) for k, v in done.items()}


# ---- targeted edits of a clean stream.  Each returns (sectors, settings changes as a dict, note); `table` is the clean stream's sector
# table (kind, frame, index, flag) -- psxhip_str_plan_sectors' or the statement's
def _video_at(table, frame, index):
    hit = np.nonzero((table[:, 0] == D.VIDEO) & (table[:, 1] == frame) & (table[:, 2] == index))[0]
    assert hit.size == 1, (frame, index)
    return int(hit[0])


def edits(fmt, sectors, table, seed=5):
    """yields (name, edited sectors, settings overrides) for one clean stream with at least 6 frames of at least 2 chunks"""
    ssz, sub_at, P = D.GEOMETRY_OF[fmt]
    rng = np.random.default_rng(seed)

    def fresh():
        return sectors.copy()

    e = fresh()                                       # one chunk zeroed: its frame is MISSING
    e[_video_at(table, 2, 1)] = 0
    yield "chunk_zeroed", e, {}

    e = fresh()                                       # a chunk again, later, with another payload: the lowest position wins
    src, dst = _video_at(table, 1, 1), _video_at(table, 4, 0)
    e[dst] = e[src]
    e[dst, P + 0x20 + 7] ^= 0xFF
    refresh_edc(fmt, e, [dst])
    yield "chunk_duplicated_later", e, {}

    e = fresh()                                       # ... and earlier: now the copy wins
    src, dst = _video_at(table, 3, 1), _video_at(table, 0, 1)
    e[dst] = e[src]
    e[dst, P + 0x20 + 9] ^= 0xFF
    refresh_edc(fmt, e, [dst])
    yield "chunk_duplicated_earlier", e, {}

    yield "order_shuffled", fresh()[rng.permutation(sectors.shape[0])], {}

    for name, frame, index, at in (("count_altered_in_non_lead", 2, 1, P + 6), ("size_altered_in_lead", 3, 0, P + 0xC),
                                   ("width_altered_in_non_lead", 1, 1, P + 0x10), ("header_copy_altered_in_non_lead", 4, 1, P + 0x15),
                                   ("header_copy_altered_in_lead", 5, 0, P + 0x15), ("chunk_index_beyond_count", 2, 1, P + 5)):
        e = fresh()
        i = _video_at(table, frame, index)
        e[i, at] ^= 0x01 if at != P + 5 else 0x40
        refresh_edc(fmt, e, [i])
        yield name, e, {}

    e = fresh()                                       # one payload bit, the EDC left as it was
    e[_video_at(table, 1, 0), P + 0x20 + 1000] ^= 0x20
    yield "payload_bit_flipped", e, {}

    if fmt == 6:
        e = fresh()                                   # the EDC where a disc has it
        i = np.nonzero(table[:, 0] == D.VIDEO)[0][::2]
        refresh_edc(fmt, e, i, "disc")
        yield "edc_on_disc_placement", e, {}

    yield "wrong_video_id", fresh(), dict(str_video_id=0x8002)
    yield "any_video_id", fresh(), dict(str_video_id=-1)
    if sub_at is not None and (table[:, 0] == D.AUDIO).any():
        audio = np.nonzero(table[:, 0] == D.AUDIO)[0]
        e = fresh()
        e[audio[1::3], sub_at] = 2                    # a foreign file, a foreign channel
        e[audio[2::3], sub_at + 1] = 5
        yield "foreign_xa_filtered", e, {}
        yield "foreign_xa_file_taken", e, dict(audio_xa_file=-1)
        yield "foreign_xa_all_taken", e, dict(audio_xa_file=-1, audio_xa_channel=-1)
        yield "audio_ignored", fresh(), dict(audio_channels=0)
