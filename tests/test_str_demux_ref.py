"""'psxhip STR demux v1' (tests/str_demux_ref.py) against the reference's own sector loop
(tests/str_reference_loop.py: psxavenc/filefmt.c:391-520 over the CPU oracle), and on a corrupted corpus: the statement the device
reader is held to must itself read what the reference writes, and must reach every rule it states.  No GPU.

STRV: the sector loop (and this library's muxer) hold an STRV sector in the 2336-byte buffer of the other flavours; the file takes its
first 2048 bytes (filefmt.c:575,613) -- what the reader reads."""
import copy

import numpy as np
import pytest

import oracle_lib as O
import str_demux_corpus as K
import str_demux_ref as D
import str_reference_loop as R
from psxavenc_amd import strmux

W, H = 48, 32
ALL_BITS = D.MISSING | D.DUPLICATE | D.MISMATCH | D.RANGE | D.EDC | D.GEOMETRY


def as_written(fmt, sectors):
    return np.ascontiguousarray(sectors[:, :2048]) if fmt == 9 else sectors


def loop_stream(fmt, codec, channels, fps, n_frames, trailing=False, audio_sectors=None, seed=3):
    """(settings, frames, sectors as written, positions of the loop's audio sectors, frames encoded)"""
    s = strmux.settings(fmt=fmt, codec=codec, width=W, height=H, fps_num=fps, channels=channels, trailing_audio=trailing)
    frames = O.synth_frames(W, H, n_frames, seed=seed, amp=6)
    per = 0
    if channels:
        pl = strmux.plan(s, n_frames)
        per = pl.audio_samples_per_sector * ((pl.n_audio_sectors + 2) if audio_sectors is None else audio_sectors) + (100 if audio_sectors is None else -50)
    pcm = K.pcm_for(channels, max(per, 0), seed + 1)
    at = []

    def xa_encode(settings, samples, count, lba=0, state=None):      # the loop's own audio sectors, as it asks for them
        at.append(lba)
        return O.xa_encode(settings, samples, count, lba=lba, state=state)

    sectors, _, encoded = R.encode_file_str(fmt, codec, W, H, fps, 1, 2, frames, pcm, channels=channels, trailing_audio=trailing,
                                            xa_encode=xa_encode)
    return s, frames, as_written(fmt, sectors), np.array(at, np.int64), encoded


def run(s, sectors, first_frame, max_frames, bs_stride, xa_capacity=None, margin=0):
    """the statement into canaried buffers: (result, rows, xa, the buffers whole)"""
    ssz = D.GEOMETRY_OF[s.format][0]
    cap = sectors.shape[0] if xa_capacity is None else xa_capacity
    rng = np.random.default_rng(99)
    bs_all = rng.integers(0, 256, (max_frames + 2, bs_stride + margin)).astype(np.uint8)
    xa_all = rng.integers(0, 256, (cap + 2, ssz)).astype(np.uint8)
    before = bs_all.copy(), xa_all.copy()
    res = D.demux(s, sectors, first_frame, max_frames, bs_all[1:-1, :bs_stride], xa_all[1:-1])
    assert np.array_equal(bs_all[[0, -1]], before[0][[0, -1]]) and np.array_equal(bs_all[:, bs_stride:], before[0][:, bs_stride:])
    assert np.array_equal(xa_all[[0, -1]], before[1][[0, -1]])
    res["bs"], res["xa"], res["bs_before"] = bs_all[1:-1, :bs_stride], xa_all[1:-1], before[0][1:-1, :bs_stride]
    return res


CLEAN = [(7, 0, 2, 15, False, None), (6, 1, 1, 15, False, None), (9, 2, 0, 15, False, None), (7, 1, 2, 25, True, None),
         (6, 2, 2, 60, False, None), (7, 2, 1, 15, True, None), (6, 0, 0, 25, False, None), 
         (7, 0, 2, 15, False, 2), (6, 1, 2, 15, True, 6), (7, 0, 2, 15, False, 0)]     # the audio ends first: EOF flags, the zero sector


@pytest.mark.parametrize("fmt,codec,channels,fps,trailing,audio_sectors", CLEAN)
def test_reads_what_the_reference_loop_writes(fmt, codec, channels, fps, trailing, audio_sectors):
    s, frames, sectors, audio_at, encoded = loop_stream(fmt, codec, channels, fps, 14, trailing, audio_sectors)
    assert encoded >= (4 if audio_sectors is None else 0)
    budgets = strmux.frame_budgets(s, 0, max(encoded, 1))
    stride = int(budgets.max())
    res = run(s, sectors, 1, encoded + 1, stride)
    want, want_res, rc = O.mdec_encode(codec, W, H, frames[:max(encoded, 1)], budgets)
    assert rc == 0
    for f in range(encoded):
        info = dict(zip(D.INFO_FIELDS, res["info"][f]))
        cc = int(budgets[f]) // 2016
        assert info["status"] == 0 and info["frame_index"] == f + 1 and info["chunk_count"] == cc == info["chunks_placed"], (f, info)
        assert info["bytes_used"] == want_res[f, 1] and (info["width"], info["height"]) == (W, H)
        assert res["sizes"][f] == cc * 2016 and np.array_equal(res["bs"][f, :cc * 2016], want[f, :cc * 2016]), f
        assert np.array_equal(res["bs"][f, cc * 2016:], res["bs_before"][f, cc * 2016:])
    assert res["info"][encoded].tolist() == [0, 0, 0, 0, 0, 0, 0, D.MISSING] and res["sizes"][encoded] == 0
    # the table against what the loop did: its audio sectors where it asked for them, all-zero sectors for its empty audio slots
    kinds = np.full(sectors.shape[0], D.VIDEO)
    kinds[audio_at] = D.AUDIO
    kinds[~sectors.any(axis=1)] = D.OTHER
    assert np.array_equal(res["table"][:, 0], kinds)
    assert np.array_equal(res["xa"][:audio_at.size], sectors[audio_at])
    if audio_at.size:
        sub_at = D.GEOMETRY_OF[fmt][1]
        assert np.array_equal(res["table"][audio_at, 3], sectors[audio_at, sub_at + 2] >> 7)
        assert np.array_equal(res["table"][audio_at, 2], np.arange(audio_at.size))
        if audio_sectors is not None:      # the audio ends first: the loop finalises the sectors it writes from then on
            assert res["table"][audio_at, 3].any()
    if audio_sectors == 0:                 # no samples at all: the audio slot is the all-zero sector
        assert (kinds == D.OTHER).any() and audio_at.size == 0
    if audio_sectors is None:          # (a plan needs the amount of audio; plenty, as the stream was made)
        pl = strmux.plan(s, 14)
        n_pcm = pl.audio_samples_per_sector * (pl.n_audio_sectors + 2) + 100 if channels else 0
        assert np.array_equal(res["table"], strmux.plan_sectors(s, 14, n_pcm))
    summary = dict(zip(D.SUMMARY_FIELDS, res["summary"]))
    assert summary == dict(n_video=int((kinds == D.VIDEO).sum()), n_audio=audio_at.size, n_other=int((kinds == D.OTHER).sum()), first_frame=1 if encoded else 0,
                           n_rows=encoded, n_complete=encoded, n_dropped_video=0, n_dropped_audio=0)
    # first_frame found from the stream; fewer rows and less room for audio than the stream has
    auto = run(s, sectors, -1, encoded + 1, stride)
    for k in ("sizes", "info", "table", "summary", "bs"):
        assert np.array_equal(auto[k], res[k]), k
    if encoded < 5:
        return
    few = run(s, sectors, 2, 3, stride, xa_capacity=min(2, audio_at.size))
    assert np.array_equal(few["bs"][:, :2016], res["bs"][1:4, :2016]) and np.array_equal(few["xa"], res["xa"][:min(2, audio_at.size)])
    fs = dict(zip(D.SUMMARY_FIELDS, few["summary"]))
    assert fs["n_rows"] == 3 and fs["n_complete"] == 3 and fs["n_dropped_audio"] == audio_at.size - min(2, audio_at.size)
    assert fs["n_dropped_video"] == summary["n_video"] - int(few["info"][:, 1].sum())


@pytest.mark.parametrize("fmt", [6, 7, 9])
def test_corrupted_corpus_reaches_every_rule(fmt):
    sectors, done = K.synthetic(fmt, seed=fmt)
    s = strmux.settings(fmt=fmt, width=W, height=H, channels=2)
    res = run(s, sectors, 1000, 200, 8 * 2016 + 32, xa_capacity=900, margin=16)
    status = res["info"][:, 7]
    reached = int(np.bitwise_or.reduce(status))
    assert reached == (ALL_BITS if fmt != 9 else ALL_BITS & ~D.EDC), bin(reached)
    assert (status == 0).any() and (res["sizes"] > 0).any() and ((status & D.MISSING) != 0).any()
    summary = dict(zip(D.SUMMARY_FIELDS, res["summary"]))
    assert summary["n_dropped_video"] > 0 and summary["n_rows"] == 200 and 0 < summary["n_complete"] < 200
    assert (summary["n_audio"] > 900 and summary["n_dropped_audio"] == summary["n_audio"] - 900) or fmt == 9
    assert summary["n_video"] < done["video"].size                       # (some carry another video id)
    if fmt != 9:
        assert 0 < summary["n_audio"] < done["audio"].size               # (some carry another file or channel)
        table = res["table"]
        in_row = (table[:, 0] == D.VIDEO) & (table[:, 1] >= 0)
        flagged = np.nonzero(in_row & ((table[:, 3] & D.EDC) != 0))[0]
        assert np.array_equal(flagged, np.intersect1d(done["bad_edc"], np.nonzero(in_row)[0])) and flagged.size > 0
        assert np.intersect1d(done["zero_edc"], np.nonzero(in_row)[0]).size > 0
    if fmt == 6:                                                         # both accepted placements, and a wrong word in either
        ok = K.video_sector(6, 5, 0, 1, 8, W, H, np.arange(2016) % 251)[None].repeat(4, axis=0)
        K.refresh_edc(6, ok, [0, 2], "muxed")
        K.refresh_edc(6, ok, [1, 3], "disc")
        ok[2, 0x818] ^= 1
        ok[3, 0x808] ^= 1
        assert D.edc_bad(6, ok).tolist() == [False, False, True, True]
        assert np.intersect1d(done["disc"], np.nonzero(in_row)[0]).size > 0
    # rows nothing was placed in are as they were
    untouched = res["info"][:, 2] == 0
    assert untouched.any() and np.array_equal(res["bs"][untouched], res["bs_before"][untouched])


def _settings_with(s, **over):
    s2 = copy.copy(s)
    for k, v in over.items():
        setattr(s2, k, v)
    return s2


@pytest.mark.parametrize("fmt,channels", [(7, 2), (6, 1), (9, 0)])
def test_targeted_edits(fmt, channels):
    s, frames, sectors, audio_at, encoded = loop_stream(fmt, 0, channels, 15, 12)
    stride = int(strmux.frame_budgets(s, 0, encoded).max())
    clean = run(s, sectors, 1, encoded, stride)
    assert not clean["info"][:, 7].any()
    seen = set()
    for name, edited, over in K.edits(fmt, sectors, clean["table"]):
        seen.add(name)
        res = run(_settings_with(s, **over), edited, 1, encoded, stride)
        st = res["info"][:, 7]
        same_rows = [f for f in range(encoded) if res["sizes"][f] and np.array_equal(res["bs"][f], clean["bs"][f])]
        if name == "chunk_zeroed":
            assert st[2] == D.MISSING and res["sizes"][2] == 0 and not np.delete(st, 2).any() and len(same_rows) == encoded - 1
        elif name == "chunk_duplicated_later":
            assert st[1] == D.DUPLICATE and st[4] & D.MISSING and 1 in same_rows and not np.delete(st, [1, 4]).any()
        elif name == "chunk_duplicated_earlier":
            assert st[3] == D.DUPLICATE and st[0] & D.MISSING and 3 not in same_rows and res["sizes"][3] == clean["sizes"][3]
            assert np.array_equal(res["bs"][3, 2016:4032] != clean["bs"][3, 2016:4032], np.arange(2016) == 9)
        elif name == "order_shuffled":
            assert np.array_equal(res["bs"], clean["bs"]) and np.array_equal(res["sizes"], clean["sizes"]) and not st.any()
            assert np.array_equal(res["xa"][:audio_at.size], edited[res["table"][:, 0] == D.AUDIO])
        elif name.endswith("_altered_in_non_lead") or name.endswith("_altered_in_lead"):
            assert np.count_nonzero(st) == 1 and st[st != 0][0] == D.MISMATCH and len(same_rows) == encoded, (name, st)
        elif name == "chunk_index_beyond_count":
            assert st[2] == D.RANGE | D.MISSING and not np.delete(st, 2).any()
        elif name == "payload_bit_flipped":
            assert st[1] == (D.EDC if fmt != 9 else 0) and not np.delete(st, 1).any()
        elif name in ("edc_on_disc_placement", "any_video_id", "audio_ignored"):
            assert not st.any() and np.array_equal(res["bs"], clean["bs"])
            assert name != "audio_ignored" or (res["summary"][1] == 0 and res["summary"][2] == clean["summary"][1] + clean["summary"][2])
        elif name == "wrong_video_id":
            assert (st == D.MISSING).all() and res["summary"][0] == 0 and res["summary"][3] == 0
        elif name == "foreign_xa_filtered":
            assert res["summary"][1] == audio_at.size - audio_at[1::3].size - audio_at[2::3].size
        elif name == "foreign_xa_file_taken":
            assert res["summary"][1] == audio_at.size - audio_at[2::3].size
        elif name == "foreign_xa_all_taken":
            assert res["summary"][1] == audio_at.size and np.array_equal(res["xa"][:audio_at.size], edited[audio_at])
        else:
            raise AssertionError("no expectation for edit %s" % name)
    assert len(seen) == {6: 18, 7: 17, 9: 13}[fmt]
    # rows narrower than the frames, and of a width that is no multiple of a chunk
    for stride2 in (2016, 4 * 2016, 4 * 2016 + 100):
        res = run(s, sectors, 1, encoded, stride2, margin=8)
        assert ((res["info"][:, 7] & (D.RANGE | D.MISSING)) == (D.RANGE | D.MISSING)).all() and not res["sizes"].any()
        assert (res["info"][:, 2] == stride2 // 2016).all() and np.array_equal(res["bs"][:, :stride2 // 2016 * 2016], clean["bs"][:, :stride2 // 2016 * 2016])
        assert np.array_equal(res["bs"][:, stride2 // 2016 * 2016:], res["bs_before"][:, stride2 // 2016 * 2016:])
