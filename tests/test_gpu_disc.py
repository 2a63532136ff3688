"""psxhip_disc_finish_device / psxhip_disc_check_device / psxhip_disc_finish_host against "psxhip disc finish v1" and "psxhip disc
check v1" (tests/disc_ref.py), byte for byte: every source size, forms mixed inside a source, padded strides with junk, guard bytes
round the image, interleaves with gaps and multi-slot sources, images made in pieces, the check kernel on clean, edited and random
sectors -- and the composition the finisher exists for: what it writes goes back through the STR reader and the XA disassembler."""
import numpy as np
import pytest

import disc_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096


def _sectors(rng, n, size, pad=0, forms=None):
    """n random sectors of `size` bytes in rows of size + pad; forms: per sector 1 / 2 (None: random), ignored by 2048-byte sources"""
    data = rng.integers(0, 256, (n, size + pad)).astype(np.uint8)
    at = {2352: 0x12, 2336: 2}.get(size)
    if at is not None and forms is not None:
        for k, f in enumerate(forms):
            data[k, at] = (data[k, at] & 0xDF) | (0x20 if f == 2 else 0)
    return data


def _finish(slots, start_lba, srcs, first_out=0, n_out=None):
    """the device's image for R.Source sources (uploaded as they are, padding and junk included), written between guard bytes"""
    import torch
    from psxavenc_amd import disc
    keep = [disc.source(torch.from_numpy(s.data).to(DEV), s.size, s.file, s.channel, s.data_subheader) for s in srcs]
    lay = disc.layout(slots, start_lba)
    if n_out is None:
        n_out = disc.disc_plan(lay, keep) - first_out
        assert n_out + first_out == R.plan(slots, srcs)
    g = torch.Generator(device="cpu").manual_seed(11)
    buf = torch.randint(0, 256, (2 * GUARD + n_out * 2352,), generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
    before = buf.clone()
    d_out = buf[GUARD:GUARD + n_out * 2352].view(n_out, 2352)
    assert disc.disc_finish(lay, keep, first_out, n_out, d_out=d_out) is d_out
    torch.cuda.synchronize()
    assert torch.equal(buf[:GUARD], before[:GUARD]) and torch.equal(buf[-GUARD:], before[-GUARD:]), "guard bytes round d_out changed"
    for (s, t), src in zip(keep, srcs):
        assert np.array_equal(t.cpu().numpy(), src.data), "a source changed"
    return d_out


def _same(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        k, at = np.argwhere(got != want)[0]
        raise AssertionError("sector %d differs first at byte 0x%X: %02X, statement %02X (%d bytes in all)"
                             % (k, at, got[k, at], want[k, at], int((got != want).sum())))


def _against_statement(slots, start_lba, srcs, first_out=0, n_out=None):
    d = _finish(slots, start_lba, srcs, first_out, n_out)
    _same(d, R.finish(slots, start_lba, srcs, first_out, n_out))
    return d


@pytest.mark.parametrize("start_lba", [73, 4498])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("size", [2352, 2336, 2048])
def test_one_source(size, n, start_lba):
    """the BCD carries frame -> second (lba + 150 = 225) and second -> minute (4650 = 1:02:00) fall inside the runs"""
    rng = np.random.default_rng(size + 10 * n + start_lba)
    forms = [1, 2, 1][:n] if start_lba == 73 else [2, 1, 2][:n]
    src = R.Source(_sectors(rng, n, size, forms=forms), size, data_subheader=(3, 1, 0x09, 0))
    d = _against_statement([0], start_lba, [src]).cpu().numpy()
    want_forms = [1] * n if size == 2048 else forms
    assert [2 if b & 0x20 else 1 for b in d[:, 0x12]] == want_forms


@pytest.mark.parametrize("size,pad", [(2352, 4), (2336, 16), (2048, 304), (2336, 2352 - 2336 + 2352)])
def test_padded_strides_and_guard_bytes(size, pad):
    """junk between the sectors is never read (the statement does not see it either), nothing outside d_out is written"""
    rng = np.random.default_rng(size + pad)
    src = R.Source(_sectors(rng, 5, size, pad, forms=[1, 2, 2, 1, 1]), size)
    d = _against_statement([0], 0, [src])
    other = src._replace(data=src.data.copy())
    other.data[:, size:] ^= 0xFF
    assert (other.data != src.data).any()
    _same(_finish([0], 0, [other]), d.cpu().numpy())


def _eight_sources(rng):
    counts, sizes = [0, 1, 3, 5, 5, 2, 1, 4], [2336, 2352, 2336, 2048, 2336, 2352, 2048, 2336]
    return [R.Source(_sectors(rng, n, size), size) for n, size in zip(counts, sizes)]


def test_interleave_eight_sources():
    srcs = _eight_sources(np.random.default_rng(8))
    d = _against_statement(list(range(8)), 1000, srcs).cpu().numpy()
    assert d.shape[0] == 40
    null = [j for j in range(40) if R.schedule(list(range(8)), srcs, j) is None]
    assert len(null) == 40 - 21
    for j in null:
        assert list(d[j, 0x10:0x18]) == [0, 0, 0x20, 0] * 2 and not d[j, 0x18:0x92C].any() and d[j, 0x92C:].any()


def test_interleave_gaps_and_a_source_with_two_slots():
    rng = np.random.default_rng(9)
    srcs = [R.Source(_sectors(rng, 7, 2336), 2336), R.Source(_sectors(rng, 2, 2352, 8), 2352)]
    slots = [0, -1, 0, -1]
    with pytest.raises(Exception):
        _finish(slots, 0, srcs)                      # source 1 has sectors and no slot
    slots = [0, -1, 0, 1]
    d = _against_statement(slots, 0, srcs).cpu().numpy()
    assert d.shape[0] == 16
    assert [R.schedule(slots, srcs, j) for j in range(6)] == [(0, 0), None, (0, 1), (1, 0), (0, 2), None]
    slots = [-1, 0, -1, 0]
    srcs = srcs[:1]
    _against_statement(slots, 5, srcs)


def test_file_and_channel_overrides_keep_the_top_bits():
    rng = np.random.default_rng(10)
    a, b, c = _sectors(rng, 3, 2336), _sectors(rng, 3, 2352), _sectors(rng, 3, 2048)
    a[:, 1], b[:, 0x11] = [0xE5, 0x1F, 0x80], [0x00, 0xFF, 0x61]
    srcs = [R.Source(a, 2336, file=200, channel=31), R.Source(b, 2352, file=-1, channel=0), R.Source(c, 2048, 255, 9, (1, 0xC3, 0x08, 0x7F)),
            R.Source(a, 2336, file=0, channel=-1)]
    d = _against_statement([0, 1, 2, 3], 0, srcs).cpu().numpy()
    assert [list(d[4 * k, 0x10:0x12]) for k in range(3)] == [[200, 0xFF], [200, 0x1F], [200, 0x9F]]
    assert [list(d[4 * k + 1, 0x10:0x12]) for k in range(3)] == [[b[0, 0x10], 0x00], [b[1, 0x10], 0xE0], [b[2, 0x10], 0x60]]
    assert list(d[2, 0x10:0x18]) == [255, 0xC9, 0x08, 0x7F] * 2
    assert [list(d[4 * k + 3, 0x10:0x12]) for k in range(3)] == [[0, 0xE5], [0, 0x1F], [0, 0x80]]


def test_image_made_in_two_calls():
    srcs = _eight_sources(np.random.default_rng(12))
    slots = list(range(8))
    whole = R.finish(slots, 4400, srcs)
    a = _finish(slots, 4400, srcs, 0, 13)
    b = _finish(slots, 4400, srcs, 13, 27)
    _same(np.concatenate([a.cpu().numpy(), b.cpu().numpy()]), whole)
    _same(_finish(slots, 4400, srcs, 39, 1), whole[39:])
    assert _finish(slots, 4400, srcs, 40, 0).shape[0] == 0


@pytest.fixture(scope="module")
def big():
    """4 099 output sectors of mixed forms and all three sizes: four times as many workgroups as the GPU has CUs, a count that is a multiple of nothing"""
    rng = np.random.default_rng(4099)
    srcs = [R.Source(_sectors(rng, 2100, 2352), 2352), R.Source(_sectors(rng, 1000, 2336, 16), 2336, channel=3),
            R.Source(_sectors(rng, 1000, 2048), 2048)]
    slots = [0, 1, 0, 2]
    return slots, srcs, R.finish(slots, 20000, srcs, 0, 4099)


def test_4099_sectors(big):
    slots, srcs, want = big
    assert R.plan(slots, srcs) == 4200
    _same(_finish(slots, 20000, srcs, 0, 4099), want)
    forms = (want[:, 0x12] & 0x20) != 0
    assert 1000 < forms.sum() < 3000


# ---- the check kernel
def _check(image, start_lba):
    import torch
    from psxavenc_amd import disc
    d = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image)).to(DEV)
    d_status, d_summary = disc.disc_check(d, start_lba)
    torch.cuda.synchronize()
    return d_status.cpu().numpy(), dict(zip(disc.SUMMARY_FIELDS, d_summary.cpu().tolist()))


def _check_against_statement(image, start_lba):
    st, summary = _check(image, start_lba)
    want_st, want_summary = R.check(image, start_lba)
    assert np.array_equal(st, want_st), (np.argwhere(st != want_st)[:5].ravel(), st[st != want_st][:5], want_st[st != want_st][:5])
    assert summary == want_summary
    return st, summary


def test_check_of_a_finished_image_is_clean(big):
    slots, srcs, want = big
    st, summary = _check(want, 20000)
    assert not st.any()
    n2 = int(((want[:, 0x12] & 0x20) != 0).sum())
    assert summary == dict(R.check(want, 20000)[1]) and (summary["n_sectors"], summary["n_form1"], summary["n_form2"], summary["n_bad"]) == (4099, 4099 - n2, n2, 0)
    st, summary = _check(want[:50], -1)
    assert not st.any() and summary["n_bad"] == 0
    st, summary = _check(want[:50], 20001)
    assert list(st) == [R.HEADER] * 50 and summary["n_header"] == 50
    # without the status array
    import torch
    from psxavenc_amd import disc
    none, d_summary = disc.disc_check(torch.from_numpy(want[:9]).to(DEV), 20000, status=False)
    assert none is None and d_summary.cpu().tolist()[:4] == [9, int(((want[:9, 0x12] & 0x20) == 0).sum()), int(((want[:9, 0x12] & 0x20) != 0).sum()), 0]


def test_check_bits_of_single_flipped_bytes():
    """sync, minute, mode, second subheader copy, data, EDC, P, Q: one byte each; sectors 0, 2, 4 are form 1, sectors 1, 3, 5 form 2"""
    rng = np.random.default_rng(13)
    img = R.finish([0], 7000, [R.Source(_sectors(rng, 6, 2336, forms=[1, 2, 1, 2, 1, 2]), 2336)])
    ecc = R.ECC_P | R.ECC_Q
    edits = [(7, 0, R.SYNC), (12, 1, R.HEADER), (15, 2, R.HEADER), (0x15, 0, R.SUBHEADER | R.EDC | ecc), (0x16, 1, R.SUBHEADER | R.EDC),
             (0x400, 2, R.EDC | ecc), (0x400, 3, R.EDC), (0x81A, 4, R.EDC | ecc), (0x92E, 5, R.EDC), (0x81C + 171, 0, ecc), (0x81C, 2, ecc),
             (0x8C8 + 103, 2, R.ECC_Q), (0x8C8, 4, R.ECC_Q)]
    for at, k, want in edits:
        bad = img.copy()
        bad[k, at] ^= 0x04
        st, summary = _check_against_statement(bad, 7000)
        assert st[k] == want and summary["n_bad"] == 1, (hex(at), k, st[k], want)
    absent = img.copy()
    absent[1, 0x92C:] = 0
    absent[0, 0x818:0x81C] = 0                            # form 1 has no "absent": a zero word is a wrong word
    st, summary = _check_against_statement(absent, 7000)
    assert st[1] == R.EDC_ABSENT and st[0] == R.EDC | ecc and summary["n_edc_absent"] == 1


def test_check_of_512_random_sectors():
    rng = np.random.default_rng(14)
    img = rng.integers(0, 256, (512, 2352)).astype(np.uint8)
    img[::7, :12] = R.SYNC_BYTES
    img[::5, 15] = 2
    img[::3, 12:15] = [0x12, 0x34, 0x56]
    img[::4, 0x14:0x18] = img[::4, 0x10:0x14]
    img[::16, 0x92C:] = 0
    _check_against_statement(img, -1)
    _check_against_statement(img, 300)


# ---- composition
W, H = 64, 48


def _str_stream(fmt):
    import torch
    import oracle_lib as O
    import str_demux_corpus as K
    from psxavenc_amd import strmux
    s = strmux.settings(fmt=fmt, codec=0, width=W, height=H, channels=2 if fmt != 9 else 0, tail=strmux.TAIL_COMPLETE)
    d_frames = torch.from_numpy(O.synth_frames(W, H, 5, seed=3, amp=6)).to(DEV)
    d_pcm = None
    if fmt != 9:
        pl = strmux.plan(s, 5)
        d_pcm = torch.from_numpy(K.pcm_for(2, pl.audio_samples_per_sector * (pl.n_audio_sectors + 2) + 100, 4)).to(DEV)
    mux = strmux.StrMuxer((0,))
    d_out, p = mux.encode_device(s, d_frames, d_pcm)
    d_sectors = d_out[0].clone()
    mux.close()
    return s, d_sectors, p


@pytest.mark.parametrize("fmt", [7, 6])
def test_finished_str_stream_goes_back_through_the_reader(fmt):
    import copy
    import torch
    from psxavenc_amd import StrReader, disc
    s, d_sectors, p = _str_stream(fmt)
    n = d_sectors.shape[0]
    assert n == p.n_sectors and p.n_frames_encoded == 5 and p.n_audio_sectors > 0
    lay = disc.layout([0], 3000)
    d_img = disc.disc_finish(lay, [disc.source(d_sectors)])
    torch.cuda.synchronize()
    assert tuple(d_img.shape) == (n, 2352)
    _same(d_img, R.finish([0], 3000, [R.Source(d_sectors.cpu().numpy(), d_sectors.shape[1])]))
    st, summary = _check(d_img, 3000)
    assert not st.any() and summary["n_form1"] > 0 and summary["n_form2"] == p.n_audio_sectors
    reader = StrReader(0)
    bs_stride = (p.max_frame_size + 2015) // 2016 * 2016
    before = reader.demux_device(s, d_sectors, 5, bs_stride)
    s_cd = copy.copy(s)
    s_cd.format = 7
    after = reader.demux_device(s_cd, d_img, 5, bs_stride)
    torch.cuda.synchronize()
    for k in ("bs", "sizes", "summary", "table"):
        assert torch.equal(before[k], after[k]), k
    info0, info1 = before["info"].cpu().numpy(), after["info"].cpu().numpy()
    assert np.array_equal(info0[..., :7], info1[..., :7])
    assert not (info1[..., 7] & 16).any() and not info1[..., 7].any(), "a finished frame fails the reader's EDC rule"
    assert (after["sizes"] > 0).all()
    # the XA sectors the reader compacts are the finished ones: same sound, EDC right
    na = int(after["summary"][0, 1])
    assert na == p.n_audio_sectors and torch.equal(after["xa"][0, :na, 0x18:0x92C], before["xa"][0, :na, 0x18 - (2352 - d_sectors.shape[1]):d_sectors.shape[1] - 4])
    reader.close()


def test_finished_xacd_sectors_disassemble_to_the_same_units():
    import torch
    import str_demux_corpus as K
    from psxavenc_amd import adpcm, disc, xa_disassemble
    xs = adpcm.XaSettings(format=adpcm.PSX_AUDIO_XA_FORMAT_XACD, stereo=True, frequency=37800, bits_per_sample=4, file_number=1, channel_number=0)
    per = adpcm.xa_get_samples_per_sector(xs)
    pcm = np.stack([K.pcm_for(2, 3 * per, 20 + i) for i in range(2)])
    sectors = adpcm.xa_encode_streams(xs, pcm, 3 * per, finalize=True).reshape(2, -1, 2352)
    n = sectors.shape[1]
    assert n >= 3
    d_src = torch.from_numpy(sectors).to(DEV)
    lay = disc.layout([0, 1], 150)
    d_img = disc.disc_finish(lay, [disc.source(d_src[0]), disc.source(d_src[1], channel=1)])
    torch.cuda.synchronize()
    _same(d_img, R.finish([0, 1], 150, [R.Source(sectors[0], 2352), R.Source(sectors[1], 2352, channel=1)]))
    assert not _check(d_img, 150)[0].any()
    for i in range(2):
        want_units, want_status = xa_disassemble(d_src[i].contiguous(), xs)
        units, status = xa_disassemble(d_img[i::2].contiguous(), xs)
        torch.cuda.synchronize()
        assert torch.equal(units, want_units) and not status.any() and not want_status.any()
    assert d_img[1::2, 0x11].cpu().tolist() == [1] * n and int(d_img[2 * n - 1, 0x12]) & 0x80, "channel override, EOF bit kept"


def test_strv_with_a_data_subheader_checks_clean():
    import torch
    from psxavenc_amd import disc
    s, d_sectors, p = _str_stream(9)
    d_src = d_sectors[:, :2048]                         # an STRV sector lies in a 2336-byte row of the muxer's output
    lay = disc.layout([0], 0)
    d_img = disc.disc_finish(lay, [disc.source(d_src, size=2048, data_subheader=(1, 0, 0x48, 0))])
    torch.cuda.synchronize()
    _same(d_img, R.finish([0], 0, [R.Source(d_sectors.cpu().numpy(), 2048, data_subheader=(1, 0, 0x48, 0))]))
    st, summary = _check(d_img, 0)
    assert not st.any() and summary["n_form1"] == p.n_sectors and summary["n_form2"] == 0
    assert torch.equal(d_img[:, 0x18:0x818], d_src)


def test_host_path_equals_the_device_path():
    from psxavenc_amd import disc
    srcs = _eight_sources(np.random.default_rng(15))
    pad = R.Source(_sectors(np.random.default_rng(16), 4, 2336, 48), 2336, file=9)
    srcs[0] = pad
    slots = list(range(8))
    lay = disc.layout(slots, 100)
    keep = [disc.source(s.data, s.size, s.file, s.channel, s.data_subheader) for s in srcs]
    got = disc.disc_finish_host(lay, keep)
    _same(got, _finish(slots, 100, srcs).cpu().numpy())
    _same(disc.disc_finish_host(lay, keep, 7, 11), got[7:18])
