"""psxhip_strspu_demux_device / psxhip_spu_deinterleave_device / psxhip_strspu_read_host against 'psxhip STRSPU demux v1'
(tests/strspu_demux_ref.py): every output -- rows, sizes, frame records, unit records, chunk records, sector table, both summaries --
byte for byte, into buffers with canary margins before, after and between streams, which must come back untouched.  The streams: this
library's own format 8 (StrMuxer.encode_device) over the crossing of tests/strspu_demux_cases.py, long ones, damaged ones, seeded random
bytes.  Then the decoders behind the reader on the device, the de-interleave alone over SPUI / VAGI files, and the whole reader."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import strspu_demux_cases as X
import strspu_demux_ref as R
import strspu_ref as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W, H = X.W, X.H
_cache = {}


def _reader():
    from psxavenc_amd import StrReader
    if "reader" not in _cache:
        _cache["reader"] = StrReader(0)
    return _cache["reader"]


def _settings(ns, fmt=8):
    """the ctypes settings of a statement's stand-in (tests/strspu_demux_cases.py: settings)"""
    from psxavenc_amd import strmux
    options = ns.strspu_options
    return strmux.settings(fmt=fmt, codec=ns.video_codec, width=ns.video_width, height=ns.video_height, fps_num=ns.str_fps_num,
                           fps_den=ns.str_fps_den, cd_speed=ns.str_cd_speed, video_id=ns.str_video_id, trailing_audio=bool(ns.trailing_audio),
                           channels=ns.audio_channels if fmt == 8 else 0, frequency=ns.audio_frequency, tail=strmux.TAIL_COMPLETE,
                           audio_id=options & 0xFFFF, spu_loop=bool(options & M.LOOP), spu_no_leading_dummy=bool(options & M.NO_LEADING_DUMMY))


def muxed(case):
    """one case muxed on the device: (ctypes settings, d_sectors (n, 2048) CUDA tensor, frames, K); the bytes are the muxer's statement's"""
    import torch
    from psxavenc_amd import strmux
    if ("muxed", case) not in _cache:
        ns, frames, pcm, want, rows, K, budgets = X.stream(case)
        s = _settings(ns)
        mux = strmux.StrMuxer((0,))
        d_out, p = mux.encode_device(s, torch.from_numpy(frames).to(DEV), torch.from_numpy(pcm).to(DEV) if pcm.size else None)
        mux.close()
        d_sectors = d_out[0].clone()
        assert p.sector_size == 2048 and np.array_equal(d_sectors.cpu().numpy(), want), case
        _cache[("muxed", case)] = (s, d_sectors, frames, K)
    return _cache[("muxed", case)]


def device_vs_statement(s, streams, first_frame, max_frames, bs_stride, capacity=None, table=True, in_offset=0, in_pad=2048):
    """streams: list of (n, 2048) uint8 arrays of one length -> one psxhip_strspu_demux_device call over all of them through the raw
    binding: the source in_offset bytes behind a 16-byte boundary, the streams n * 2048 + in_pad bytes apart, every output between
    canaries; every stream's outputs against the statement's.  Returns the device outputs as numpy (per stream)."""
    import torch
    from psxavenc_amd import _lib, strdemux
    L = strdemux._bind()
    S, n = len(streams), streams[0].shape[0]
    cap = n if capacity is None else capacity
    rng = np.random.default_rng(7)

    def noise(shape, dtype=np.uint8):
        return rng.integers(0, 256, shape, dtype=np.uint8).astype(dtype) if dtype == np.uint8 else rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)

    in_stride = n * 2048 + in_pad
    h_in = noise(16 + S * in_stride + 16)
    for i, st in enumerate(streams):
        h_in[in_offset + i * in_stride: in_offset + i * in_stride + n * 2048] = np.ascontiguousarray(st).reshape(-1)
    d_in = torch.from_numpy(h_in).to(DEV)
    assert d_in.data_ptr() % 16 == 0
    bs0, units0 = noise((S, max_frames + 2, bs_stride)), noise((S, (cap + 2) * 126, 16))
    bs_all, units_all = torch.from_numpy(bs0).to(DEV), torch.from_numpy(units0).to(DEV)
    assert units_all.data_ptr() % 16 == 0
    Mg = 64
    counts = dict(sizes=max_frames, info=max_frames * 8, table=n * 4, summary=8, chunk_info=cap * 8, audio_summary=4)
    before = {k: noise(2 * Mg + S * c, np.int32) for k, c in counts.items()}
    flat = {k: torch.from_numpy(v).to(DEV) for k, v in before.items()}
    at = {k: v.data_ptr() + 4 * Mg for k, v in flat.items()}
    rc = L.psxhip_strspu_demux_device(
        _reader()._h, C.byref(s), S, d_in.data_ptr() + in_offset, in_stride, n, int(first_frame), max_frames, bs_all.data_ptr() + bs_stride,
        bs_stride, (max_frames + 2) * bs_stride, at["sizes"], at["info"], units_all.data_ptr() + 126 * 16 if cap else None, cap,
        (cap + 2) * 126 * 16, at["chunk_info"] if cap else None, at["table"] if table else None, at["summary"], at["audio_summary"],
        torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    _lib.check(rc)
    assert np.array_equal(d_in.cpu().numpy(), h_in), "the source was written"
    after = {k: v.cpu().numpy() for k, v in flat.items()}
    for k in counts:          # the margins of the record buffers
        assert np.array_equal(after[k][:Mg], before[k][:Mg]) and np.array_equal(after[k][-Mg:], before[k][-Mg:]), k
    if not table:
        assert np.array_equal(after["table"], before["table"])
    bs1, units1 = bs_all.cpu().numpy(), units_all.cpu().numpy()
    shapes = dict(sizes=(max_frames,), info=(max_frames, 8), table=(n, 4), summary=(8,), chunk_info=(cap, 8), audio_summary=(4,))
    got = []
    for i, st in enumerate(streams):
        want_bs, want_units = bs0[i].copy(), units0[i].copy()
        want = R.demux(s, st, first_frame, max_frames, want_bs[1:-1], want_units[126:len(want_units) - 126])
        assert np.array_equal(bs1[i], want_bs), ("rows or their margins", i, np.nonzero((bs1[i] != want_bs).any(axis=1))[0][:8])
        bad = np.nonzero((units1[i] != want_units).any(axis=1))[0]
        assert bad.size == 0, ("unit records or their margins", i, bad[:8] - 126)
        mine = dict(bs=bs1[i][1:-1], units=units1[i][126:len(want_units) - 126], units_before=units0[i][126:len(want_units) - 126])
        for k, c in counts.items():
            if k == "table" and not table:
                continue
            mine[k] = after[k][Mg + i * c: Mg + (i + 1) * c].reshape(shapes[k])
            assert mine[k].shape == want[k].shape, (k, mine[k].shape, want[k].shape)
            if not mine[k].size:
                continue
            bad = np.nonzero(mine[k].reshape(len(mine[k]), -1) != want[k].reshape(len(mine[k]), -1))[0]
            assert bad.size == 0, (k, i, bad[:8], mine[k][bad[:4]], want[k][bad[:4]])
        got.append(mine)
    return got


def _chains(ch, n_units):
    from psxavenc_amd.adpcm import CHAIN_DTYPE
    chains = np.zeros(ch, CHAIN_DTYPE)
    for c in range(ch):
        chains[c] = (c, ch, 28 * n_units, n_units, ch)
    return chains


def composition(s, d_sectors, n_frames, stride, capacity):
    """the reader, the BS decoder and the ADPCM decoder behind one another on the device, nothing copied to the host in between:
    dict(out = the reader's tensors, frames, decoded, pcm as numpy)"""
    import torch
    from psxavenc_amd import MdecDecoder, decode_chains_device
    out = _reader().demux_strspu_device(s, d_sectors, n_frames, stride, first_frame=1, audio_capacity=capacity)
    dec = MdecDecoder(s.video_width, s.video_height, dc_wrap=s.video_codec == 2, device=0)
    _, d_frames, d_decoded = dec.decode_frames_device(out["bs"][0], out["sizes"][0], levels=False, frames=True)
    ch = s.audio_channels
    d = 0 if s.strspu_options & M.NO_LEADING_DUMMY else 1
    n_units = capacity * (126 // ch) - d if ch and capacity else 0
    pcm = np.zeros(0, np.int16)
    if n_units > 0:
        d_pcm = torch.zeros(28 * n_units * ch, dtype=torch.int16, device=DEV)
        decode_chains_device(out["units"][0], _chains(ch, n_units), np.arange(ch, dtype=np.int32) + d * ch, 5, 4, d_pcm)
        pcm = d_pcm.cpu().numpy()
    torch.cuda.synchronize()
    res = dict(out=out, frames=d_frames.cpu().numpy(), decoded=d_decoded.cpu().numpy(), pcm=pcm)
    dec.close()
    return res


# ---------------------------------------------------------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("case", X.CROSSING + X.EDGES, ids=lambda c: "%dch-%d-%dx-%x-%s-%df" % (c[0], c[1], c[2], c[3] >> 16, "trailing" if c[4] else "leading", c[5]))
def test_round_trip_on_the_device(case):
    """encode_device in format 8 -> demux_strspu_device -> BS decode and ADPCM decode: every reader output is the statement's, the table
    the plan's, the pictures those of the existing reader over the stream as format 9, the PCM the statement decoder's"""
    from psxavenc_amd import strmux
    ns, frames, pcm, want_sectors, rows, K, budgets = X.stream(case)
    s, d_sectors, _, _ = muxed(case)
    n_frames, stride = frames.shape[0], int(budgets.max())
    got = device_vs_statement(s, [want_sectors], 1, n_frames, stride, capacity=K + 1)[0]
    assert np.array_equal(got["table"], strmux.plan_sectors(s, n_frames)) and np.array_equal(got["table"], rows)
    assert not got["info"][:, 7].any() and not got["chunk_info"][:K, 1].any()
    assert got["chunk_info"][K].tolist() == [-1, R.MISSING, 0, 0, 0, 0, 0, 0]
    assert got["audio_summary"].tolist() == [K, K, K - 1 if K else -1, 0]
    assert got["summary"].tolist() == [int((rows[:, 0] == 0).sum()), K, 0, 1, n_frames, n_frames, 0, 0]
    assert np.array_equal(got["units"][K * 126:], got["units_before"][K * 126:])
    if K:
        assert np.array_equal(R.lane_streams(got["units"][:K * 126], s.audio_channels), X.expected_lanes(pcm, s.audio_channels, K, s.strspu_options))
    # ---- the decoders behind it, through the Python mirror, from the device-resident stream
    comp = composition(s, d_sectors, n_frames, stride, K)
    for name in ("sizes", "info", "table", "summary", "audio_summary"):
        assert np.array_equal(comp["out"][name][0].cpu().numpy(), got[name]), name
    assert np.array_equal(comp["out"]["chunk_info"][0].cpu().numpy(), got["chunk_info"][:K])
    s9 = _settings(ns, fmt=9)
    old = _reader().read(s9, want_sectors, n_frames, first_frame=1, pcm_sectors=0)
    assert (comp["decoded"][:, 0] == 0).all() and np.array_equal(comp["decoded"], old["decoded"])
    assert np.array_equal(comp["frames"], old["frames"]) and comp["frames"].any()
    assert np.array_equal(comp["pcm"], X.expected_pcm(case))


def test_no_sectors_is_valid():
    ns = X.settings(2, 44100, 2)
    got = device_vs_statement(_settings(ns), [np.zeros((0, 2048), np.uint8)], -1, 2, 2016, capacity=2)[0]
    assert (got["info"][:, 7] == 1).all() and (got["chunk_info"][:, 1] == R.MISSING).all() and not got["summary"].any()
    assert got["audio_summary"].tolist() == [0, 0, -1, 0]


# ---------------------------------------------------------------------------------------------------------------- 2. long streams
def _long(seed):
    """more than 513 sectors of 44100 Hz stereo at 2x, muxed on the device"""
    import torch
    from psxavenc_amd import strmux
    if ("long", seed) not in _cache:
        ns = X.settings(2, 44100, 2, options=M.LOOP if seed & 1 else 0)
        s = _settings(ns)
        n_frames = 56
        pl = strmux.plan(s, n_frames)
        pcm = X.pcm_for(2, (pl.n_audio_sectors + 1) * pl.audio_samples_per_sector, seed, kind=seed % 3)
        mux = strmux.StrMuxer((0,))
        d_out, p = mux.encode_device(s, torch.from_numpy(O.synth_frames(W, H, n_frames, seed=seed, amp=5)).to(DEV), torch.from_numpy(pcm).to(DEV))
        mux.close()
        assert p.n_sectors > 513
        _cache[("long", seed)] = (s, d_out[0].cpu().numpy(), n_frames, p.max_frame_size)
    return _cache[("long", seed)]


@pytest.mark.parametrize("length", [255, 256, 257, 513, None])
def test_streams_longer_than_one_scan_block(length):
    s, sectors, n_frames, stride = _long(40)
    n = sectors.shape[0] if length is None else length
    got = device_vs_statement(s, [sectors[:n]], 1, n_frames, stride)[0]
    n_audio = int(got["summary"][1])
    assert n_audio == -(-n // 6) and got["audio_summary"][:2].tolist() == [n_audio, n_audio] and not got["chunk_info"][:n_audio, 1].any()
    assert int(got["summary"][:3].sum()) == n


def test_two_streams_with_padded_strides_and_different_content():
    s, a, n_frames, stride = _long(40)
    _, b, _, _ = _long(42)
    n = 513
    together = device_vs_statement(s, [a[:n], b[:n]], 1, n_frames, stride, capacity=90, in_pad=3 * 2048)
    for i, st in enumerate((a, b)):
        alone = device_vs_statement(s, [st[:n]], 1, n_frames, stride, capacity=90)[0]
        for k in ("sizes", "info", "summary", "table", "chunk_info", "audio_summary"):
            assert np.array_equal(alone[k], together[i][k]), (i, k)
        K = int(alone["audio_summary"][0])
        assert K == 86 and np.array_equal(alone["units"][:K * 126], together[i]["units"][:K * 126])
    assert not np.array_equal(together[0]["units"][:86 * 126], together[1]["units"][:86 * 126])


# ---------------------------------------------------------------------------------------------------------------- 3. load paths
@pytest.mark.parametrize("in_offset,in_pad,S", [(0, 2048, 1), (4, 2048, 1), (8, 2048, 1), (12, 2048, 1), (0, 2048, 2), (0, 2048 + 4, 2), (0, 2048 + 8, 2),
                                                (4, 2048 + 12, 2), (0, 4096, 3)])
def test_both_load_paths(in_offset, in_pad, S):
    """the de-interleave loads 16 bytes at once when the source base and the stream stride are 16-byte aligned, else four dwords: bases
    0, 4, 8 and 12 bytes behind a 16-byte boundary, stream strides that are and are not multiples of 16"""
    streams = [X.stream(X.CROSSING[i])[3] for i in (7, 11, 7)][:S]
    ns = X.stream(X.CROSSING[7])[0]
    # (streams of one length and the same ids; the second is 11025 Hz: its chunks disagree with the settings' rate)
    assert len({st.shape[0] for st in streams}) == 1
    got = device_vs_statement(_settings(ns), streams, 1, 5, 10 * 2016, capacity=10, in_offset=in_offset, in_pad=in_pad)
    assert got[0]["audio_summary"].tolist() == [9, 9, 8, 0] and not got[0]["chunk_info"][:9, 1].any()
    if S > 1:
        assert got[1]["audio_summary"].tolist() == [3, 3, 2, 0] and got[1]["chunk_info"][:, 1].tolist() == [R.MISMATCH] * 3 + [R.MISSING] * 7


# ---------------------------------------------------------------------------------------------------------------- 4. capacity
def test_capacity_below_the_chunks_and_capacity_zero():
    ns, frames, pcm, sectors, rows, K, budgets = X.stream(X.CROSSING[6])
    s = _settings(ns)
    full = device_vs_statement(s, [sectors], 1, frames.shape[0], int(budgets.max()), capacity=K)[0]
    got = device_vs_statement(s, [sectors], 1, frames.shape[0], int(budgets.max()), capacity=K - 2)[0]
    assert got["summary"][1] == K and got["summary"][7] == 2 and got["audio_summary"].tolist() == [K - 2, K - 2, -1, 0]
    assert np.array_equal(got["units"], full["units"][:(K - 2) * 126]) and (got["table"][X.audio_positions(rows)[-2:], 2] == -1).all()
    got = device_vs_statement(s, [sectors], 1, frames.shape[0], int(budgets.max()), capacity=0)[0]           # d_units NULL
    assert got["summary"][1] == K and got["summary"][7] == K and got["audio_summary"].tolist() == [0, 0, -1, 0]
    assert np.array_equal(got["bs"], full["bs"]) and np.array_equal(got["info"], full["info"])


# ---------------------------------------------------------------------------------------------------------------- 5. damage
DAMAGE = ("removed", "duplicated", "reordered", "number-0", "number-max") + tuple(X.MISMATCH_EDITS)


@pytest.mark.parametrize("name", DAMAGE)
def test_damage_gives_status_bits(name):
    """a stream with a non-default audio id and a non-default video id, damaged: held to the statement, unowned records keep the canary"""
    case = X.CROSSING[6]
    ns, frames, pcm, sectors, rows, K, budgets = X.stream(case)
    assert ns.strspu_options & 0xFFFF != 1 and ns.str_video_id != 0x8001 and K >= 4
    s = _settings(ns)
    bad = X.damaged(name, sectors, rows, np.random.default_rng(5))
    got = device_vs_statement(s, [bad], 1, frames.shape[0], int(budgets.max()), capacity=K)[0]
    status = got["chunk_info"][:, 1].tolist()
    if name in ("removed", "number-0", "number-max"):
        assert status == [0, R.MISSING] + [0] * (K - 2) and np.array_equal(got["units"][126:252], got["units_before"][126:252])
        assert got["summary"][7] == (0 if name == "removed" else 1)
    elif name == "duplicated":
        assert status == [0, 0, R.DUPLICATE] + [0] * (K - 3) and got["summary"][1] == K + 1
        assert np.array_equal(got["units"][252:378].reshape(-1), np.concatenate([sectors[X.audio_positions(rows)[2], 0x20 + c * 1008:][:1008].reshape(63, 16) for c in (0, 1)], axis=1).reshape(-1))
    elif name == "reordered":
        assert not any(status)
    else:
        assert status == [0, 0, R.MISMATCH] + [0] * (K - 3)
    assert not got["info"][:, 7].any()                   # the video rows do not notice


@pytest.mark.parametrize("seed", [1, 2])
def test_seeded_random_sectors(seed):
    """64 sectors of random bytes given 60 01 and the audio or the video id at random: status bits, never a fault"""
    ns = X.settings(1 + seed % 2, 44100, 2, options=X.OPTION_SETS[seed], audio_id=0x0002, video_id=0x8001, width=0, height=0)
    s = _settings(ns)
    sectors = X.random_sectors(seed, 64, 0x0002, 0x8001)
    got = device_vs_statement(s, [sectors], 2, 6, 3 * 2016 + 8, capacity=8)[0]
    assert got["summary"][1] > 8 and got["summary"][7] > 0 and got["summary"][0] > 0
    reached = int(np.bitwise_or.reduce(got["chunk_info"][:, 1]))
    assert reached & R.MISMATCH and reached & R.DUPLICATE
    device_vs_statement(s, [sectors, sectors[::-1]], -1, 12, 2016, capacity=13, in_pad=2048 + 4)


# ---------------------------------------------------------------------------------------------------------------- 6. the de-interleave alone
def _deinterleave_vs_statement(body, chunk_stride, lane_offset, lane_bytes, channels, src=None, in_offset=0):
    """psxhip_spu_deinterleave_device over one stream through the raw binding, between canaries, against the statement"""
    import torch
    from psxavenc_amd import _lib, strdemux
    L = strdemux._bind()
    rng = np.random.default_rng(11)
    chunks = np.ascontiguousarray(body).reshape(-1, chunk_stride)
    n = len(src) if src is not None else chunks.shape[0]
    per = channels * (lane_bytes // 16)
    h_in = rng.integers(0, 256, 16 + chunks.size + 16, dtype=np.uint8)
    h_in[in_offset: in_offset + chunks.size] = chunks.reshape(-1)
    units0 = rng.integers(0, 256, ((n + 2) * per, 16), dtype=np.uint8)
    d_in, d_units = torch.from_numpy(h_in).to(DEV), torch.from_numpy(units0).to(DEV)
    d_src = torch.from_numpy(np.asarray(src, np.int32)).to(DEV) if src is not None else None
    rc = L.psxhip_spu_deinterleave_device(0, d_in.data_ptr() + in_offset, n, chunk_stride, lane_offset, lane_bytes, channels,
                                          d_src.data_ptr() if d_src is not None else None, 1, 0, d_units.data_ptr() + per * 16, 0,
                                          torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    _lib.check(rc)
    want = units0.copy()
    R.deinterleave(chunks, lane_offset, lane_bytes, channels, want[per:len(want) - per], src)
    got = d_units.cpu().numpy()
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, bad[:8] - per
    return d_units[per:len(want) - per], got[per:len(want) - per]


@pytest.mark.parametrize("fmt_name,channels,interleave,alignment", [("SPUI", 2, 2048, 2048), ("VAGI", 2, 2048, 2048), ("SPUI", 1, 32, 64), ("VAGI", 1, 32, 64)])
def test_spui_and_vagi_bodies(fmt_name, channels, interleave, alignment):
    """a file from psxhip_spu_file_encode_host, de-interleaved and decoded on the device: the PCM is the statement decode of the file's
    lanes"""
    import torch
    from psxavenc_amd import decode_chains_device, spufile, strdemux
    fmt = spufile.FORMAT_SPUI if fmt_name == "SPUI" else spufile.FORMAT_VAGI
    B = interleave // 16
    pcm = X.pcm_for(channels, 28 * (2 * B + B // 2) if interleave == 2048 else 28 * 37, 60 + channels, kind=1)
    fs = spufile.settings(fmt, channels=channels, freq=22050, interleave=interleave, alignment=alignment)
    data = spufile.encode(fs, pcm, device=0)
    header = -(-48 // alignment) * alignment if fmt_name == "VAGI" else 0
    chunk_stride = -(-channels * interleave // alignment) * alignment
    body = data[header:]
    assert body.size % chunk_stride == 0 and body.size // chunk_stride >= 3
    n = body.size // chunk_stride
    d_units, units = _deinterleave_vs_statement(body, chunk_stride, 0, interleave, channels)
    d_pcm = torch.zeros(28 * n * B * channels, dtype=torch.int16, device=DEV)
    decode_chains_device(d_units, _chains(channels, n * B), np.arange(channels, dtype=np.int32), 5, 4, d_pcm)
    lanes = np.stack([body.reshape(n, chunk_stride)[:, c * interleave:(c + 1) * interleave].reshape(-1, 16) for c in range(channels)])
    assert np.array_equal(d_pcm.cpu().numpy(), X.decode_lanes(lanes, 0))
    # ... and through the Python mirror
    mirror = strdemux.spu_deinterleave_device(torch.from_numpy(np.ascontiguousarray(body.reshape(n, chunk_stride))).to(DEV), interleave, channels)
    torch.cuda.synchronize()
    assert np.array_equal(mirror[0].cpu().numpy(), units)


def test_source_table_and_the_smallest_odd_shape():
    """d_src_chunk with a permutation and negative entries; three channels of one block each; sources off a 16-byte boundary"""
    rng = np.random.default_rng(12)
    body = rng.integers(0, 256, 7 * 64, dtype=np.uint8)
    for in_offset in (0, 4, 8, 12):
        _deinterleave_vs_statement(body, 64, 8, 16, 3, in_offset=in_offset)                     # lanes at 8, 24, 40 of a 64-byte chunk
        _deinterleave_vs_statement(body, 64, 8, 16, 3, src=[6, -1, 0, 3, 3, -5, 1, 2, 5], in_offset=in_offset)
    _deinterleave_vs_statement(body[:6 * 48], 48, 0, 16, 3)                                      # the 16-byte loads, a dense odd shape
    big = rng.integers(0, 256, 5 * 2048, dtype=np.uint8)
    _deinterleave_vs_statement(big, 2048, 0x20, 1008, 2, src=[4, 3, -1, 1, 0])
    _deinterleave_vs_statement(big, 2048, 0x20, 2016, 1, src=[-1, -1])


# ---------------------------------------------------------------------------------------------------------------- 7. the whole reader
@pytest.mark.parametrize("case", [X.CROSSING[7], X.CROSSING[1], X.EDGES[1], X.EDGES[2]], ids=["stereo", "mono-loop", "K1", "no-audio"])
def test_read_strspu_is_the_device_composition(case):
    ns, frames, pcm, sectors, rows, K, budgets = X.stream(case)
    s, d_sectors, _, _ = muxed(case)
    n_frames, ch = frames.shape[0], s.audio_channels
    comp = composition(s, d_sectors, n_frames, int(budgets.max()), K)
    got = _reader().read_strspu(s, sectors, n_frames, first_frame=1)
    assert np.array_equal(got["frames"], comp["frames"]) and np.array_equal(got["decoded"], comp["decoded"])
    assert np.array_equal(got["info"], comp["out"]["info"][0].cpu().numpy())
    assert np.array_equal(got["summary"], comp["out"]["summary"][0].cpu().numpy())
    assert np.array_equal(got["audio_summary"], comp["out"]["audio_summary"][0].cpu().numpy())
    assert np.array_equal(got["pcm"], comp["pcm"]) and np.array_equal(got["pcm"], X.expected_pcm(case))
    assert np.array_equal(got["chunk_info"][:K], comp["out"]["chunk_info"][0].cpu().numpy()) and (got["chunk_info"][K:, 1] == R.MISSING).all()
    if K < 2:
        return
    # ---- a PCM buffer that cuts whole chunks, and none at all
    B = 126 // ch
    d = 0 if s.strspu_options & M.NO_LEADING_DUMMY else 1
    cut = _reader().read_strspu(s, sectors, n_frames, first_frame=1, pcm_capacity=28 * (2 * B - d) * ch + 5)
    assert cut["pcm"].size == 28 * (2 * B - d) * ch and np.array_equal(cut["pcm"], comp["pcm"][:cut["pcm"].size])
    assert cut["summary"][7] == K - 2 and cut["audio_summary"].tolist() == [2, 2, -1, 0] and cut["chunk_info"].shape[0] == 2
    assert np.array_equal(cut["frames"], comp["frames"])
    none = _reader().read_strspu(s, sectors, n_frames, first_frame=1, pcm_capacity=0)
    assert none["pcm"].size == 0 and none["summary"][7] == K and none["summary"][1] == K and np.array_equal(none["frames"], comp["frames"])


def test_read_strspu_decodes_a_missing_chunk_as_silence():
    case = X.CROSSING[6]
    ns, frames, pcm, sectors, rows, K, budgets = X.stream(case)
    s = _settings(ns)
    bad = X.damaged("removed", sectors, rows, np.random.default_rng(5))
    got = _reader().read_strspu(s, bad, frames.shape[0], first_frame=1)
    units = np.zeros((K * 126, 16), np.uint8)
    R.demux(s, bad, 1, 0, np.zeros((0, 2016), np.uint8), units)
    d = 0 if s.strspu_options & M.NO_LEADING_DUMMY else 1
    assert np.array_equal(got["pcm"], X.decode_lanes(R.lane_streams(units, 2), d)) and got["chunk_info"][1, 1] == R.MISSING
    assert not got["pcm"].reshape(-1, 2)[28 * (63 - d):28 * (126 - d)].any() and got["pcm"].reshape(-1, 2)[28 * (126 - d):].any()


def test_one_reader_strcd_then_strspu_then_strcd(monkeypatch):
    """both _host readers on ONE fresh handle in turns -- about 8 sectors and 1 frame of an STRCD stream, the smallest STRSPU case (one
    audio chunk), the STRCD piece again: they share the handle's staging buffer and its keyed BS decoder, and the STRCD pictures are
    64 x 48 where the STRSPU stream's are 48 x 32, so the decoder is rebuilt for the second and again for the third call.  Every call
    against the expectation of its own file: _expected_read (tests/test_gpu_str_demux.py) and composition"""
    import test_gpu_str_demux as T
    from psxavenc_amd import MdecDecoder, StrReader, strmux
    monkeypatch.setattr(T, "W", 64)          # clean_stream and _expected_read build pictures of the module's size
    monkeypatch.setattr(T, "H", 48)
    s7, _, d7, p7, _ = T.clean_stream(7, 0, 2, 15, 4, seed=11)          # (a seed no other test muxes: the cache is keyed without the size)
    cd = d7.cpu().numpy()[:8]
    assert cd.shape[0] == 8 and (s7.video_width, s7.video_height) == (64, 48) != (W, H)
    stride = int(strmux.frame_budgets(s7, 0, p7.n_frames_encoded).max())
    dec = MdecDecoder(64, 48, dc_wrap=False, device=0)
    want, px, decoded, pcm, status = T._expected_read(s7, dec, cd, 1, stride)
    dec.close()
    assert want["summary"][0] > 0 and pcm.size > 0
    case = X.EDGES[1]
    ns, frames, _, sectors, rows, K, budgets = X.stream(case)
    s8, d8, _, _ = muxed(case)
    assert K == 1
    comp = composition(s8, d8, frames.shape[0], int(budgets.max()), K)
    reader = StrReader(0)
    for turn in ("strcd", "strspu", "strcd"):
        if turn == "strcd":
            got = reader.read(s7, cd, 1, first_frame=1, frames=np.full((1, 64 * 48 * 3 // 2), 0x55, np.uint8))
            assert np.array_equal(got["info"], want["info"]) and np.array_equal(got["summary"], want["summary"])
            assert np.array_equal(got["decoded"], decoded) and np.array_equal(got["frames"], px)
            assert got["pcm"].size == pcm.size and np.array_equal(got["pcm"], pcm)
            assert np.array_equal(got["xa_status"], status) and not status.any()
        else:
            got = reader.read_strspu(s8, sectors, frames.shape[0], first_frame=1)
            assert np.array_equal(got["frames"], comp["frames"]) and np.array_equal(got["decoded"], comp["decoded"])
            assert np.array_equal(got["info"], comp["out"]["info"][0].cpu().numpy())
            assert np.array_equal(got["summary"], comp["out"]["summary"][0].cpu().numpy())
            assert np.array_equal(got["audio_summary"], comp["out"]["audio_summary"][0].cpu().numpy())
            assert got["pcm"].size > 0 and np.array_equal(got["pcm"], comp["pcm"]) and np.array_equal(got["pcm"], X.expected_pcm(case))
            assert np.array_equal(got["chunk_info"][:K], comp["out"]["chunk_info"][0].cpu().numpy())
    reader.close()
