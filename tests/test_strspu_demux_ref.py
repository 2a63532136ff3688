"""'psxhip STRSPU demux v1' (tests/strspu_demux_ref.py) held to the muxer's statement (tests/strspu_ref.py, section
15): over streams the muxer's statement builds, the reader's statement gives back the video rows, the lane streams G_c exactly (dummy
block, the chain's blocks, loop flags or trap block), every status 0 and a table equal to the schedule's rows.  No GPU, no product
code: this pins the checker the device tests use (tests/test_gpu_strspu_demux.py), and makes the PCM they expect."""
import numpy as np
import pytest

import oracle_lib as O
import strspu_demux_cases as X
import strspu_demux_ref as R
import strspu_ref as M


def test_the_crossing_covers_what_it_should():
    cases = X.CROSSING
    assert {(c[0], c[1], c[2]) for c in cases} == {(ch, f, sp) for ch in (1, 2) for f in (44100, 32000, 11025) for sp in (1, 2)}
    for ch in (1, 2):
        assert {c[3] for c in cases if c[0] == ch} == set(X.OPTION_SETS)
        assert {c[4] for c in cases if c[0] == ch} == {False, True}
    assert {c[5] for c in cases} == {2, 3, 4, 5}


@pytest.mark.parametrize("case", X.CROSSING, ids=lambda c: "%dch-%d-%dx-%x-%s-%df" % (c[0], c[1], c[2], c[3] >> 16, "trailing" if c[4] else "leading", c[5]))
def test_muxed_streams_come_back(oracle, case):
    s, frames, pcm, sectors, rows, K, budgets = X.stream(case)
    ch, options, n_frames = s.audio_channels, s.strspu_options, frames.shape[0]
    B = 126 // ch
    d = 0 if options & M.NO_LEADING_DUMMY else 1
    stride = int(budgets.max()) + 2016
    got = X.run_statement(s, sectors, 1, n_frames, stride, K + 1, fill=0xA5)
    # ---- video: the oracle's bitstreams, every frame whole
    bs, res, rc = O.mdec_encode(s.video_codec, X.W, X.H, frames, budgets, stride=int(budgets.max()))
    assert rc == 0
    for f in range(n_frames):
        assert np.array_equal(got["bs"][f, :budgets[f]], bs[f, :budgets[f]]), f
        assert (got["bs"][f, budgets[f]:] == 0xA5).all()
    assert np.array_equal(got["sizes"], budgets)
    assert (got["info"][:, 7] == 0).all() and np.array_equal(got["info"][:, 0], np.arange(1, n_frames + 1))
    # ---- audio: G_c exactly; the chunk without an owner keeps the fill
    G = X.expected_lanes(pcm, ch, K, options)
    assert np.array_equal(R.lane_streams(got["units"][:K * 126], ch), G)
    assert (got["units"][K * 126:] == 0xA5).all()
    if K:
        assert not d or not G[:, 0].any()                            # the dummy block is silent
        last = G[:, K * B - 1]
        assert (last[:, 1] == (3 if options & M.LOOP else 5)).all()
    info = got["chunk_info"]
    assert (info[:K, 1] == 0).all() and info[K].tolist() == [-1, R.MISSING, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(info[:K, 0], X.audio_positions(rows))
    assert (info[:K, 2] == ch).all() and (info[:K, 3] == 16 * B).all() and (info[:K, 4] == s.audio_frequency).all()
    assert info[:K, 5].tolist() == [0 if k == 0 else 28 * (k * B - d) for k in range(K)]
    assert got["audio_summary"].tolist() == [K, K, K - 1 if K else -1, 0]
    # ---- the table is the schedule; the summary counts by kind
    assert np.array_equal(got["table"], rows)
    n_video = int((rows[:, 0] == M.KIND_VIDEO).sum())
    assert got["summary"].tolist() == [n_video, K, 0, 1, n_frames, n_frames, 0, 0]
    # ---- decoding G_c[d:] is the PCM the device tests expect
    want_pcm = X.expected_pcm(case)
    assert want_pcm.size == 28 * max(K * B - d, 0) * ch


def test_recorded_reference_lanes_come_back():
    """the lanes the reference build's psx_audio_spu_encode gave (tests/golden/strspu_ref.npz), placed by the muxer's statement: the
    reader's statement returns dummy, blocks, and loop flag or trap block"""
    for case, pcm, blocks in M.golden_cases():
        ch, K, options = case["channels"], case["K"], case["options"]
        B = 126 // ch
        d = 0 if options & M.NO_LEADING_DUMMY else 1
        sectors = M.audio_sectors(blocks, K, ch, 44100, options)
        s = X.settings(ch, 44100, 2, options & ~0xFFFF, audio_id=options & 0xFFFF)
        got = X.run_statement(s, sectors, -1, 0, 2016, K)
        G = R.lane_streams(got["units"], ch)
        for c in range(ch):
            if d:
                assert not G[c, 0].any()
            want = blocks[c][:K * B - d].copy()
            for k in range(K):
                g = k * B + B - 1 - d
                if options & M.LOOP:
                    want[g, 1] = 3
                elif k == K - 1:
                    want[g] = [0, 5] + [0] * 14
            assert np.array_equal(G[c, d:], want), (case, c)
        assert (got["chunk_info"][:, 1] == 0).all() and got["audio_summary"].tolist() == [K, K, K - 1, 0]
        assert got["summary"].tolist() == [0, K, 0, 0, 0, 0, 0, 0]


def test_without_audio_the_result_is_format_9s(oracle):
    import str_demux_ref as V
    import types
    s, frames, pcm, sectors, rows, K, budgets = X.stream(X.CROSSING[7])
    s0 = X.settings(0, 0, s.str_cd_speed, 0, video_id=s.str_video_id)
    stride = int(budgets.max())
    got = X.run_statement(s0, sectors, -1, frames.shape[0], stride, 3, fill=0x11)
    v = types.SimpleNamespace(format=9, str_video_id=s.str_video_id, audio_channels=0, audio_xa_file=-1, audio_xa_channel=-1, video_width=X.W,
                              video_height=X.H)
    bs = np.full((frames.shape[0], stride), 0x11, np.uint8)
    want = V.demux(v, sectors, -1, frames.shape[0], bs, np.zeros((0, 2048), np.uint8))
    for name in ("sizes", "info", "table", "summary"):
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(got["bs"], bs) and (got["units"] == 0x11).all()
    assert (got["chunk_info"] == [-1, R.MISSING, 0, 0, 0, 0, 0, 0]).all() and got["audio_summary"].tolist() == [0, 0, -1, 0]
    assert got["summary"][2] == K


def test_damage_gives_the_status_bits_it_should(oracle):
    case = next(c for c in X.CROSSING if c[0] == 2 and X.stream(c)[5] >= 4)
    s, frames, pcm, sectors, rows, K, budgets = X.stream(case)
    rng = np.random.default_rng(5)
    clean = X.run_statement(s, sectors, 1, frames.shape[0], int(budgets.max()), K, fill=0xEE)
    a = X.audio_positions(rows)

    def run(name, capacity=K):
        return X.run_statement(s, X.damaged(name, sectors, rows, rng), 1, frames.shape[0], int(budgets.max()), capacity, fill=0xEE)

    got = run("removed")
    assert got["chunk_info"][:, 1].tolist() == [0, R.MISSING] + [0] * (K - 2)
    assert (got["units"][126:252] == 0xEE).all() and np.array_equal(got["units"][252:], clean["units"][252:])
    assert got["audio_summary"].tolist() == [K, K - 1, K - 1, 0]
    got = run("duplicated")
    assert got["chunk_info"][:, 1].tolist() == [0, 0, R.DUPLICATE] + [0] * (K - 3)
    assert np.array_equal(got["units"], clean["units"]) and got["summary"][1] == K + 1
    got = run("reordered")
    assert (got["chunk_info"][:, 1] == 0).all() and np.array_equal(got["units"], clean["units"])
    assert got["chunk_info"][:4, 0].tolist() == [a[2], a[3], a[0], a[1]]
    for name in ("number-0", "number-max"):
        got = run(name)
        assert got["chunk_info"][1].tolist() == [-1, R.MISSING, 0, 0, 0, 0, 0, 0] and got["summary"][7] == 1 and got["summary"][1] == K
        assert got["table"][a[1]].tolist() == [1, -1, -1, 0]
    for name in X.MISMATCH_EDITS:
        got = run(name)
        assert got["chunk_info"][:, 1].tolist() == [0, 0, R.MISMATCH] + [0] * (K - 3), name
        assert R.mismatch_clauses(X.damaged(name, sectors, rows, rng)[a[2]], 2, 2, s.audio_frequency, s.strspu_options) == [name]
    # frequency 0 in the settings: the rate is not compared
    s_any = X.settings(2, 0, s.str_cd_speed, s.strspu_options & ~0xFFFF, audio_id=s.strspu_options & 0xFFFF, video_id=s.str_video_id)
    got = X.run_statement(s_any, X.damaged("frequency", sectors, rows, rng), 1, frames.shape[0], int(budgets.max()), K)
    assert (got["chunk_info"][:, 1] == 0).all()
    # capacity below K: the overflow is dropped
    got = X.run_statement(s, sectors, 1, frames.shape[0], int(budgets.max()), K - 2, fill=0xEE)
    assert got["summary"][7] == 2 and got["audio_summary"].tolist() == [K - 2, K - 2, -1, 0]
    assert np.array_equal(got["units"], clean["units"][:(K - 2) * 126])
