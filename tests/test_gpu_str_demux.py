"""psxhip_str_demux_device / psxhip_str_read_host against 'psxhip STR demux v1' (tests/str_demux_ref.py): every output -- rows, sizes,
frame records, compacted XA sectors, sector table, summary -- bit for bit, into buffers with canary margins before, after and between
streams (and behind the last whole chunk of every row when bs_stride is no multiple of 2016), which must come back untouched.  The
streams: this library's own (StrMuxer.encode_device, never leaving the device), truncated ones, a seeded synthetic corpus, targeted
edits.  Then the whole reader and the verify loop the reader exists for."""
import copy

import numpy as np
import pytest

import oracle_lib as O
import str_demux_corpus as K
import str_demux_ref as D

pytestmark = pytest.mark.gpu

W, H = 48, 32
DEV = "cuda:0"
_cache = {}


def _reader():
    from psxavenc_amd import StrReader
    if "reader" not in _cache:
        _cache["reader"] = StrReader(0)
    return _cache["reader"]


def clean_stream(fmt, codec, channels, fps, n_frames, trailing=False, seed=3):
    """this library's own stream, muxed on the device: (settings, d_frames, d_sectors as the file holds them, plan).  An STRV sector
    lies in a 2336-byte row of the muxer's output; the file -- and the reader -- take its first 2048 bytes (filefmt.c:575,613)."""
    import torch
    from psxavenc_amd import strmux
    key = (fmt, codec, channels, fps, n_frames, trailing, seed)
    if key not in _cache:
        s = strmux.settings(fmt=fmt, codec=codec, width=W, height=H, fps_num=fps, channels=channels, trailing_audio=trailing)
        d_frames = torch.from_numpy(O.synth_frames(W, H, n_frames, seed=seed, amp=6)).to(DEV)
        d_pcm, n_pcm = None, 0
        if channels:
            pl = strmux.plan(s, n_frames)
            n_pcm = pl.audio_samples_per_sector * (pl.n_audio_sectors + 2) + 100
            d_pcm = torch.from_numpy(K.pcm_for(channels, n_pcm, seed + 1)).to(DEV)
        mux = strmux.StrMuxer((0,))
        d_out, p = mux.encode_device(s, d_frames, d_pcm)
        d_sectors = d_out[0, :, :2048].contiguous() if fmt == 9 else d_out[0].clone()
        mux.close()
        _cache[key] = (s, d_frames, d_sectors, p, n_pcm)
    return _cache[key]


def device_vs_statement(s, streams, first_frame, max_frames, bs_stride, xa_capacity=None, table=True):
    """streams: list of (n, sector size) uint8 arrays or CUDA tensors of one length -> one psxhip_str_demux_device call over all of them,
    with padded strides and canaries; every stream's outputs against the statement's.  Returns the device outputs as numpy (per stream)."""
    import torch
    ssz = D.GEOMETRY_OF[s.format][0]
    S, n = len(streams), streams[0].shape[0]
    cap = n if xa_capacity is None else xa_capacity
    g = torch.Generator(device="cpu").manual_seed(7)

    def noise(shape, dtype=torch.uint8):
        return torch.randint(0, 256, shape, generator=g, dtype=torch.int32).to(dtype).to(DEV)

    d_in = torch.zeros((S, n + 1, ssz), dtype=torch.uint8, device=DEV)
    for i, st in enumerate(streams):
        d_in[i, :n] = st if torch.is_tensor(st) else torch.from_numpy(np.ascontiguousarray(st)).to(DEV)
    bs_all, xa_all = noise((S, max_frames + 2, bs_stride)), noise((S, cap + 2, ssz))
    M = 64
    flat = {k: noise((2 * M + S * c,), torch.int32) for k, c in (("sizes", max_frames), ("info", max_frames * 8), ("table", n * 4), ("summary", 8))}
    before = {k: v.clone() for k, v in flat.items()}
    bs0, xa0 = bs_all.cpu().numpy(), xa_all.cpu().numpy()
    view = {k: v[M:v.numel() - M] for k, v in flat.items()}
    out = _reader().demux_device(s, d_in[:, :n], max_frames, bs_stride, first_frame=first_frame, xa_capacity=cap, d_bs=bs_all[:, 1:-1],
                                 d_sizes=view["sizes"].view(S, max_frames), d_info=view["info"].view(S, max_frames, 8), d_xa=xa_all[:, 1:-1],
                                 d_table=view["table"].view(S, n, 4) if table else None, d_summary=view["summary"].view(S, 8), table=table)
    torch.cuda.synchronize()
    for k, v in flat.items():          # the margins of the record buffers
        assert torch.equal(v[:M], before[k][:M]) and torch.equal(v[-M:], before[k][-M:]), k
    if not table:
        assert torch.equal(flat["table"], before["table"])
    bs1, xa1 = bs_all.cpu().numpy(), xa_all.cpu().numpy()
    got = []
    for i, st in enumerate(streams):
        host = st.cpu().numpy() if torch.is_tensor(st) else st
        want_bs, want_xa = bs0[i].copy(), xa0[i].copy()
        want = D.demux(s, host, first_frame, max_frames, want_bs[1:-1], want_xa[1:-1])
        assert np.array_equal(bs1[i], want_bs), ("rows or their margins", i, np.nonzero((bs1[i] != want_bs).any(axis=1))[0][:8])
        assert np.array_equal(xa1[i], want_xa), ("XA sectors or their margins", i)
        mine = dict(bs=bs1[i][1:-1], xa=xa1[i][1:-1], bs_before=bs0[i][1:-1])
        for k in ("sizes", "info", "table", "summary"):
            if k == "table" and not table:
                continue
            mine[k] = out[k][i].cpu().numpy()
            assert mine[k].shape == want[k].shape, (k, mine[k].shape, want[k].shape)
            bad = np.nonzero((mine[k] != want[k]).any(axis=tuple(range(1, mine[k].ndim))))[0] if mine[k].ndim > 1 else np.nonzero(mine[k] != want[k])[0]
            assert bad.size == 0, (k, i, bad[:8], mine[k][bad[:4]], want[k][bad[:4]])
        got.append(mine)
    return got


CLEAN = [(7, 0, 2, 15, False), (6, 1, 1, 15, False), (9, 2, 0, 15, False), (7, 1, 2, 25, True), (6, 2, 2, 60, False), (7, 2, 1, 15, True),
         (6, 0, 0, 25, False)]


@pytest.mark.parametrize("fmt,codec,channels,fps,trailing", CLEAN)
def test_clean_streams_never_leave_the_device(fmt, codec, channels, fps, trailing):
    import torch
    from psxavenc_amd import strmux
    from psxavenc_amd.mdec import MdecEncoder
    n_frames = 20
    s, d_frames, d_sectors, p, n_pcm = clean_stream(fmt, codec, channels, fps, n_frames, trailing)
    nf = p.n_frames_encoded
    assert nf >= 14
    budgets = strmux.frame_budgets(s, 0, nf)
    stride = int(budgets.max())
    got = device_vs_statement(s, [d_sectors], 1, nf + 1, stride)[0]
    assert np.array_equal(got["table"], strmux.plan_sectors(s, n_frames, n_pcm))
    assert not got["info"][:nf, 7].any() and got["info"][nf].tolist() == [0, 0, 0, 0, 0, 0, 0, D.MISSING]
    assert np.array_equal(got["sizes"][:nf], budgets) and got["sizes"][nf] == 0
    enc = MdecEncoder(codec, W, H, max_frame_size=stride, device=0)
    d_rows, d_res = enc.encode_frames_device(d_frames[:nf].contiguous(), torch.from_numpy(budgets).to(DEV))
    rows, res = d_rows.cpu().numpy(), d_res.cpu().numpy()
    enc.close()
    for f in range(nf):
        assert np.array_equal(got["bs"][f, :budgets[f]], rows[f, :budgets[f]]), f
        assert np.array_equal(got["bs"][f, budgets[f]:], got["bs_before"][f, budgets[f]:]), f
        assert got["info"][f, 3] == res[f, 1] and got["info"][f, 0] == f + 1
    summary = dict(zip(D.SUMMARY_FIELDS, got["summary"]))
    assert (summary["n_video"], summary["n_rows"], summary["n_complete"], summary["first_frame"]) == (p.n_video_sectors, nf, nf, 1)
    auto = device_vs_statement(s, [d_sectors], -1, nf + 1, stride, table=False)[0]
    for k in ("bs", "sizes", "info", "summary", "xa"):
        assert np.array_equal(auto[k], got[k]), k


def test_three_streams_in_one_call_with_padded_strides():
    streams = [clean_stream(7, 0, 2, 15, 20, False, seed=3 + 10 * i) for i in range(3)]
    s, nf = streams[0][0], streams[0][3].n_frames_encoded
    together = device_vs_statement(s, [st[2] for st in streams], 1, nf, 10 * 2016)
    for i, st in enumerate(streams):
        alone = device_vs_statement(s, [st[2]], 1, nf, 10 * 2016)[0]
        for k in ("sizes", "info", "summary", "table"):
            assert np.array_equal(alone[k], together[i][k]), (i, k)
        # (what lies behind a row's chunks and behind the last audio sector is each buffer's own canary)
        assert all(np.array_equal(alone["bs"][f, :size], together[i]["bs"][f, :size]) for f, size in enumerate(alone["sizes"])) and alone["sizes"].all()
        n_audio = int(alone["summary"][1])
        assert n_audio > 0 and np.array_equal(alone["xa"][:n_audio], together[i]["xa"][:n_audio])
    assert not np.array_equal(together[0]["bs"][:, :2016], together[1]["bs"][:, :2016])


@pytest.mark.parametrize("length", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097, None])
def test_lengths_that_cross_the_scan_seams(length):
    """one stream of more than 5000 sectors cut at the block, wavefront and prefix-round boundaries of the scan (None: all of it); the
    last frame of a cut is not whole: MISSING, size 0"""
    s, _, d_sectors, p, _ = clean_stream(7, 0, 2, 15, 512)
    if "long" not in _cache:
        _cache["long"] = d_sectors.cpu().numpy()
    host = _cache["long"]
    n = host.shape[0]
    assert n >= 5000 and p.n_frames_encoded == 510
    length = n if length is None else length
    got = device_vs_statement(s, [host[:length]], 1, 510, 10 * 2016)[0]
    rows = int(got["summary"][4])
    assert int(got["summary"][0] + got["summary"][1] + got["summary"][2]) == length
    if 1 < length < n and got["table"][length - 1, 0] == D.VIDEO and got["table"][length - 1, 2] + 1 < got["info"][rows - 1, 1]:
        assert got["info"][rows - 1, 7] == D.MISSING and got["sizes"][rows - 1] == 0 and got["summary"][5] == rows - 1
    if length == n:
        assert got["summary"][5] == 510 and rows == 510
    assert (length != 4097) or got["summary"][5] == rows - 1       # (4097 sectors end inside a frame)


@pytest.mark.parametrize("fmt", [6, 7, 9])
def test_seeded_synthetic_corpus(fmt):
    from psxavenc_amd import strmux
    sectors, _ = K.synthetic(fmt, seed=fmt)
    s = strmux.settings(fmt=fmt, width=W, height=H, channels=2)
    got = device_vs_statement(s, [sectors], 1000, 200, 8 * 2016 + 32, xa_capacity=900)[0]
    reached = int(np.bitwise_or.reduce(got["info"][:, 7]))
    assert reached == (63 if fmt != 9 else 63 & ~D.EDC)
    device_vs_statement(s, [sectors], -1, 230, 8 * 2016 + 32, xa_capacity=3000)
    any_id = copy.copy(s)
    any_id.str_video_id, any_id.audio_xa_file, any_id.audio_xa_channel, any_id.video_width = -1, -1, -1, 0
    device_vs_statement(any_id, [sectors, sectors[::-1]], 990, 64, 11 * 2016, xa_capacity=10)


@pytest.mark.parametrize("fmt,channels", [(7, 2), (6, 1), (9, 0)])
def test_targeted_edits(fmt, channels):
    s, _, d_sectors, p, _ = clean_stream(fmt, 0, channels, 15, 20)
    sectors, nf = d_sectors.cpu().numpy(), p.n_frames_encoded
    stride = 10 * 2016
    clean = device_vs_statement(s, [sectors], 1, nf, stride)[0]
    assert not clean["info"][:, 7].any()
    names = []
    for name, edited, over in K.edits(fmt, sectors, clean["table"]):
        s2 = copy.copy(s)
        for k, v in over.items():
            setattr(s2, k, v)
        got = device_vs_statement(s2, [edited], 1, nf, stride)[0]
        names.append(name)
        if name == "order_shuffled":       # video rows do not depend on the order; audio follows position
            assert np.array_equal(got["bs"], clean["bs"]) and np.array_equal(got["sizes"], clean["sizes"]) and not got["info"][:, 7].any()
        if name == "payload_bit_flipped":
            assert got["info"][1, 7] == (D.EDC if fmt != 9 else 0)
        if name == "chunk_duplicated_later":
            assert got["info"][1, 7] == D.DUPLICATE and np.array_equal(got["bs"][1], clean["bs"][1])
    assert len(names) == {6: 18, 7: 17, 9: 13}[fmt]
    n_audio = int(clean["summary"][1])
    for rows, cap, stride2 in ((nf, max(n_audio - 1, 0), stride), (nf - 3, 1, stride), (nf, n_audio, 2016), (nf, 0, 4 * 2016), (5, n_audio, 4 * 2016 + 100)):
        got = device_vs_statement(s, [sectors], 1, rows, stride2, xa_capacity=cap)[0]
        assert got["summary"][7] == max(n_audio - cap, 0) and got["summary"][4] == rows
        assert (got["summary"][6] > 0) == (rows < nf)
        if stride2 < stride:
            assert ((got["info"][:, 7] & (D.RANGE | D.MISSING)) == (D.RANGE | D.MISSING)).all() and not got["sizes"].any()


def _expected_read(s, dec, stream, nf, stride):
    """what StrReader.read(s, stream, nf, first_frame=1) over pictures of 0x55 has to return: the statement's demux, then this
    library's BS decoder and XA decoder (each held to its own reference in its own file) over what the statement found"""
    import torch
    from psxavenc_amd import xa_decode_streams
    from psxavenc_amd.adpcm import XaSettings
    bs, xa = np.zeros((nf, stride), np.uint8), np.zeros((stream.shape[0], stream.shape[1]), np.uint8)
    want = D.demux(s, stream, 1, nf, bs, xa)
    canvas = torch.full((nf, W * H * 3 // 2), 0x55, dtype=torch.uint8, device=DEV)
    _, d_px, d_dec = dec.decode_frames_device(torch.from_numpy(bs).to(DEV), torch.from_numpy(want["sizes"]).to(DEV), levels=False, d_frames=canvas)
    torch.cuda.synchronize()
    na = int(want["summary"][1])
    pcm, status = xa_decode_streams(XaSettings(1 if s.format == 7 else 0, s.audio_channels == 2, 37800, 4), xa[:na].reshape(1, -1))
    return want, d_px.cpu().numpy(), d_dec.cpu().numpy(), pcm[0], status[0]


@pytest.mark.parametrize("fmt,channels", [(7, 2), (6, 1)])
def test_whole_reader(fmt, channels):
    from psxavenc_amd import MdecDecoder, strmux
    from psxavenc_amd.decode import DEC_EHEADER
    s, _, d_sectors, p, _ = clean_stream(fmt, 0, channels, 15, 20)
    sectors, nf = d_sectors.cpu().numpy(), p.n_frames_encoded
    stride = int(strmux.frame_budgets(s, 0, nf).max())
    dec = MdecDecoder(W, H, dc_wrap=False, device=0)

    def expected(stream):
        return _expected_read(s, dec, stream, nf, stride)

    reader = _reader()
    want, px, decoded, pcm, status = expected(sectors)
    got = reader.read(s, sectors, nf, first_frame=1, frames=np.full((nf, W * H * 3 // 2), 0x55, np.uint8))
    assert np.array_equal(got["info"], want["info"]) and np.array_equal(got["summary"], want["summary"])
    assert np.array_equal(got["decoded"], decoded) and not decoded[:, 0].any() and np.array_equal(got["frames"], px)
    assert got["pcm"].size == pcm.size > 0 and np.array_equal(got["pcm"], pcm)
    assert got["xa_status"].size == want["summary"][1] and not got["xa_status"].any() and not status.any()
    # the same stream with one chunk gone: that frame does not reach the decoder, the others are as they were
    hit = np.nonzero((want["table"][:, 0] == D.VIDEO) & (want["table"][:, 1] == 4) & (want["table"][:, 2] == 2))[0]
    cut = np.delete(sectors, hit, axis=0)
    want2, px2, decoded2, pcm2, _ = expected(cut)
    got2 = reader.read(s, cut, nf, first_frame=1, frames=np.full((nf, W * H * 3 // 2), 0x55, np.uint8))
    assert np.array_equal(got2["info"], want2["info"]) and np.array_equal(got2["decoded"], decoded2) and np.array_equal(got2["frames"], px2)
    assert got2["decoded"][4, 0] == DEC_EHEADER and (got2["frames"][4] == 0x55).all() and got2["info"][4, 7] == D.MISSING
    others = np.arange(nf) != 4
    assert np.array_equal(got2["frames"][others], got["frames"][others]) and np.array_equal(got2["decoded"][others], got["decoded"][others])
    assert np.array_equal(got2["pcm"], got["pcm"])
    # no room for audio, no pictures asked for
    got3 = reader.read(s, sectors, nf, first_frame=-1, want_frames=False, pcm_sectors=2)
    assert got3["frames"] is None and np.array_equal(got3["decoded"], decoded) and np.array_equal(got3["pcm"], pcm[:got3["pcm"].size])
    assert got3["xa_status"].size == 2 and got3["summary"][7] == want["summary"][1] - 2
    dec.close()


def test_whole_reader_small_larger_small_on_one_handle():
    """about 8, then about 64, then about 8 sectors of an STRCD stream with stereo 4-bit audio through read() of ONE fresh reader: its
    workspace and staging buffers are allocated, outgrown and reused; every call against the same references as test_whole_reader"""
    from psxavenc_amd import MdecDecoder, StrReader, strmux
    s, _, d_sectors, p, _ = clean_stream(7, 0, 2, 15, 20)
    sectors = d_sectors.cpu().numpy()
    stride = int(strmux.frame_budgets(s, 0, p.n_frames_encoded).max())
    assert sectors.shape[0] >= 64
    dec = MdecDecoder(W, H, dc_wrap=False, device=0)
    reader = StrReader(0)
    for n, nf in ((8, 1), (64, 7), (9, 1)):
        want, px, decoded, pcm, status = _expected_read(s, dec, sectors[:n], nf, stride)
        got = reader.read(s, sectors[:n], nf, first_frame=1, frames=np.full((nf, W * H * 3 // 2), 0x55, np.uint8))
        assert np.array_equal(got["info"], want["info"]) and np.array_equal(got["summary"], want["summary"]), n
        assert np.array_equal(got["decoded"], decoded) and np.array_equal(got["frames"], px), n
        assert got["pcm"].size == pcm.size > 0 and np.array_equal(got["pcm"], pcm), n
        assert np.array_equal(got["xa_status"], status) and not status.any(), n
        assert want["summary"][0] > 0 and (n < 64 or (decoded[:, 0] == 0).sum() >= 5), n      # video sectors; the long piece holds whole frames
    reader.close()
    dec.close()


def test_verify_loop_on_the_device():
    """encode -> mux -> demux -> decode -> SSE against the encoder's input, all in HBM: the figures are those of decoding the encoder's
    own rows"""
    import torch
    from psxavenc_amd import MdecDecoder, strmux
    from psxavenc_amd.decode import sse_device
    from psxavenc_amd.mdec import MdecEncoder
    s, d_frames, d_sectors, p, _ = clean_stream(7, 1, 2, 15, 20)
    nf = p.n_frames_encoded
    budgets = strmux.frame_budgets(s, 0, nf)
    stride = int(budgets.max())
    out = _reader().demux_device(s, d_sectors, nf, stride, first_frame=1, table=False)
    dec = MdecDecoder(W, H, dc_wrap=False, device=0)
    _, d_px, d_dec = dec.decode_frames_device(out["bs"][0], out["sizes"][0], levels=False)
    enc = MdecEncoder(1, W, H, max_frame_size=stride, device=0)
    d_rows, _ = enc.encode_frames_device(d_frames[:nf].contiguous(), torch.from_numpy(budgets).to(DEV))
    _, d_px2, d_dec2 = dec.decode_frames_device(d_rows, torch.from_numpy(budgets).to(DEV), levels=False)
    a = sse_device(d_px, d_frames[:nf].contiguous(), W, H)
    b = sse_device(d_px2, d_frames[:nf].contiguous(), W, H)
    torch.cuda.synchronize()
    assert not d_dec[:, 0].any().item() and torch.equal(d_dec, d_dec2)
    assert torch.equal(a, b) and (a.sum(dim=1) > 0).all().item()
    enc.close()
    dec.close()
