"""psxhip_disc_read_device / psxhip_disc_read_host against "psxhip disc read v1" (tests/disc_read_ref.py), byte for byte: the tracks
between guard bytes that must come back unchanged, the table, the counts, the summary -- image sizes round the workgroup and the
count pass's span, every track size, padded strides, capacities below the count, first match wins, submode masks, every damage
class, damage that changes the routing key, random bytes -- and the composition the reader exists for: finished STRCD streams and an
XACD track, damaged, go back through the STR reader and the XA disassembler."""
import numpy as np
import pytest

import disc_read_corpus as K
import disc_read_ref as D
import disc_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096
SPAN = 1024            # PSXHIP_DISC_READ_SPAN: the sectors of one wavefront of the count and place passes


@pytest.fixture(scope="module")
def reader():
    from psxavenc_amd import DiscReader
    r = DiscReader(0)
    yield r
    r.close()


def _stride(T):
    return T.size if T.stride is None else T.stride


def _read(reader, image, tracks, table=True, seed=5):
    """the device's answer for D.Track tracks over buffers of junk between guard bytes, compared with the statement's on the same junk;
    returns (statement's Result, the device's track tensors)"""
    import torch
    from psxavenc_amd import discread
    rng = np.random.default_rng(seed)
    d_image = torch.from_numpy(np.ascontiguousarray(image)).to(DEV)
    bufs, views, keep = [], [], []
    for T in tracks:
        body = T.capacity * _stride(T)
        buf = torch.from_numpy(rng.integers(0, 256, 2 * GUARD + body).astype(np.uint8)).to(DEV)
        view = buf[GUARD:GUARD + body].view(T.capacity, _stride(T))
        bufs.append(buf)
        views.append(view)
        keep.append(discread.track(view, T.size, T.file, T.channel, T.mask, T.value))
    before = [b.clone() for b in bufs]
    got = reader.read_device(d_image, keep, table=table)
    torch.cuda.synchronize()
    assert torch.equal(d_image.cpu(), torch.from_numpy(np.ascontiguousarray(image))), "the image changed"
    want = D.read(image, tracks, into=[b[GUARD:len(b) - GUARD].cpu().numpy().reshape(T.capacity, _stride(T)) for b, T in zip(before, tracks)])
    for t, (b, b0) in enumerate(zip(bufs, before)):
        assert torch.equal(b[:GUARD], b0[:GUARD]) and torch.equal(b[-GUARD:], b0[-GUARD:]), "guard bytes round track %d changed" % t
        g = views[t].cpu().numpy()
        if not np.array_equal(g, want.tracks[t]):
            k, at = np.argwhere(g != want.tracks[t])[0]
            raise AssertionError("track %d slot %d differs first at byte 0x%X: %02X, statement %02X" % (t, k, at, g[k, at], want.tracks[t][k, at]))
    assert got["counts"].cpu().tolist() == want.counts.tolist()
    summary = discread.summary_dict(got["summary"].cpu().tolist())
    assert summary == want.summary
    if table:
        tab = got["table"].cpu().numpy()
        if not np.array_equal(tab, want.table):
            k = np.argwhere((tab != want.table).any(axis=1))[0, 0]
            raise AssertionError("record %d: %s, statement %s" % (k, tab[k].tolist(), want.table[k].tolist()))
    else:
        assert got["table"] is None
    return want, views


def _eight_sources(rng, n):
    """eight sources of all three sizes and mixed forms, (file, channel) made the routing key by the overrides"""
    spec = [(2336, 16, 1, 0, 0x08), (2352, 0, 1, 1, 0x04), (2048, 0, 2, 0, 0x08), (2336, 0, 2, 1, 0x02), (2352, 8, 3, 0, 0x08),
            (2336, 0, 3, 5, 0x04), (2048, 304, 4, 0, 0x08), (2352, 0, 4, 31, 0x0A)]
    return [R.Source(K.sectors(rng, n, size, pad, forms=rng.integers(1, 3, n).tolist(), kind=kind), size, file=f, channel=c)
            for size, pad, f, c, kind in spec]


SLOTS = [0, 1, 2, -1, 3, 4, 5, 6, -1, 7]


@pytest.fixture(scope="module")
def big():
    """4 099 sectors of eight sources and gaps, mixed forms, a damaged sector every 97"""
    rng = np.random.default_rng(4099)
    srcs = _eight_sources(rng, 410)
    clean = R.finish(SLOTS, 20000, srcs, 0, 4099)
    image = clean.copy()
    for k in range(5, 4099, 97):
        if image[k, 0x12] & 0x20:
            image[k, 0x500] ^= 0x01
        else:
            image[k] = K.scattered(image[k], 1 + k % 7, rng)
    return srcs, clean, image


def _tracks_of(srcs, capacity):
    return [D.Track(s.size, capacity, s.file, s.channel) for s in srcs]


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, SPAN + 1])
def test_small_images_and_one_past_the_span(reader, big, n):
    """five crosses the four-sector workgroup, 1 025 the count pass's span of 1 024"""
    srcs, clean, image = big
    want, _ = _read(reader, image[:n], _tracks_of(srcs, 120))
    assert want.summary["n_sectors"] == n


def test_4099_sectors_eight_tracks_and_gaps(reader, big):
    srcs, clean, image = big
    tracks = [D.Track(s.size, 420, s.file, s.channel, stride=s.size + (16 if t % 3 == 0 else 0)) for t, s in enumerate(srcs)]
    want, views = _read(reader, image, tracks)
    s = want.summary
    assert s["n_repaired"] > 10 and s["n_edc"] > 5 and s["n_unrepairable"] == 0 and s["n_dropped"] == 0 and s["n_unclaimed"] == 0
    assert s["n_empty"] == sum(R.schedule(SLOTS, srcs, j) is None for j in range(4099))
    # what the repair gives back is the finished image
    assert np.array_equal(want.sectors[want.form == 1], clean[want.form == 1])
    _read(reader, image, tracks, table=False)


def test_capacity_below_the_count_first_match_and_submode_masks(reader, big):
    srcs, clean, image = big
    image = image[:1500]
    tracks = [D.Track(2336, 7, 1, 0, stride=2400),                    # file 1 channel 0: 150 sectors, seven slots
              D.Track(2352, 200, 3, -1, 0x04, 0x04),                 # file 3, any channel: the audio sectors ...
              D.Track(2352, 200, 3, -1, 0x08, 0x08, stride=2360),    # ... and the data sectors of it
              D.Track(2048, 150, 2, 0, 0x2E, 0x08),                  # form-1 data only
              D.Track(2048, 0, 2, 1),                                # no room at all: every sector of it is dropped
              D.Track(2352, 150, 1, -1),                             # behind track 0: file 1's other channels only
              D.Track(2336, 1200, -1, -1),                           # the catch-all behind the specific ones
              D.Track(2352, 10, 1, 0)]                               # never reached
    want, _ = _read(reader, image, tracks)
    c = want.counts.tolist()
    assert c[0] == 150 and c[7] == 0 and c[4] == 150 and c[1] == 150 and c[2] == 150 and c[5] == 150 and c[6] > 150
    assert want.summary["n_dropped"] == 143 + 150 and want.summary["n_unclaimed"] == 0
    assert (want.table[:, 2] & D.FORM).any()                          # form-2 sectors of file 2 channel 1 met a 2048-byte track
    want, _ = _read(reader, image, tracks[:6])
    assert want.summary["n_unclaimed"] > 0


def test_every_damage_class_in_one_image(reader):
    rng = np.random.default_rng(77)
    clean = K.form1_image(rng, 3 * K.N_DAMAGE_CLASSES + 2, start_lba=9000)
    image = clean.copy()
    classes = K.damage_classes(rng, clean[1::3])
    for k, (name, bad, good, repairable) in enumerate(classes):
        image[1 + 3 * k] = bad
    for at in (12, 15):
        image[0, at] ^= 0x10                                          # header bytes: clean and untouched
    want, views = _read(reader, image, [D.Track(2352, len(image), 1, 0)])
    for k, (name, bad, good, repairable) in enumerate(classes):
        j = 1 + 3 * k
        assert (want.table[j, 2] == D.REPAIRED) == repairable and (want.table[j, 2] == D.UNREPAIRABLE) == (not repairable), name
        assert np.array_equal(views[0][j].cpu().numpy(), good if repairable else bad), name
    assert want.summary["n_clean"] == len(image) - len(classes) and want.table[0, 2] == 0


def test_damage_that_changes_the_routing_key(reader):
    """a wrong file or channel byte: the sector lands in the track of its repaired subheader"""
    rng = np.random.default_rng(78)
    srcs = [R.Source(K.sectors(rng, 6, 2336), 2336, file=1, channel=c) for c in (0, 1)]
    clean = R.finish([0, 1], 0, srcs)
    image = clean.copy()
    image[2, 0x11] = 1                      # channel 0 -> 1 in the first copy
    image[3, 0x10] = 9                      # file 1 -> 9
    image[4, 0x12] = 0x20                   # data -> no kind at all, form 2: were it not repaired it would be empty
    image[5, 0x11], image[5, 0x15] = 0, 0   # both copies: two errors in different P columns, channel 1 -> 0
    tracks = [D.Track(2336, 8, 1, 0), D.Track(2336, 8, 1, 1), D.Track(2352, 8, -1, -1)]
    want, views = _read(reader, image, tracks)
    assert want.table[:, 0].tolist() == [0, 1] * 6 and want.counts.tolist() == [6, 6, 0]
    assert (want.table[2:6, 2] == D.REPAIRED).all() and want.table[2:6, 3].tolist() == [1, 1, 1, 2]
    for t in (0, 1):
        assert np.array_equal(views[t][:6].cpu().numpy(), clean[t::2, 0x10:])


def test_512_random_sectors(reader):
    rng = np.random.default_rng(79)
    image = rng.integers(0, 256, (512, 2352)).astype(np.uint8)
    image[::7, :12] = R.SYNC_BYTES
    image[::4, 0x14:0x18] = image[::4, 0x10:0x14]
    image[::16, 0x92C:] = 0
    image[::3, 0x12] |= 0x20
    image[::3, 0x16] |= 0x20
    tracks = [D.Track(2352, 40, -1, 3), D.Track(2048, 64, -1, -1, 0x04, 0x04, stride=2052), D.Track(2336, 300, -1, -1, 0x08, 0x00),
              D.Track(2352, 20, 200, -1)]
    want, _ = _read(reader, image, tracks)
    s = want.summary
    assert s["n_unrepairable"] > 100 and s["n_edc"] > 100 and s["n_edc_absent"] > 10 and s["n_repaired"] == 0 and s["n_dropped"] > 0
    assert s["n_empty"] > 0 and s["n_unclaimed"] > 0


def test_recorded_answers_on_the_device(reader):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disc_read_ref.npz"))
    tracks = [D.Track(*[int(v) for v in row]) for row in g["tracks"]]
    want, _ = _read(reader, g["image"], tracks)
    assert np.array_equal(want.table, g["table"])


def test_host_path_equals_the_device_path(reader, big):
    from psxavenc_amd import discread
    srcs, clean, image = big
    image = image[:333]
    tracks = [D.Track(s.size, 20 + 3 * t, s.file, s.channel, stride=s.size + 4 * (t % 2)) for t, s in enumerate(srcs)]
    want, _ = _read(reader, image, tracks)
    rng = np.random.default_rng(80)
    host = [rng.integers(0, 256, (T.capacity, _stride(T))).astype(np.uint8) for T in tracks]
    expect = D.read(image, tracks, into=host)
    got = reader.read_host(image, [discread.track(h, T.size, T.file, T.channel, T.mask, T.value) for h, T in zip(host, tracks)])
    for t in range(len(tracks)):
        assert np.array_equal(host[t], expect.tracks[t]), t
    assert np.array_equal(got["table"], want.table) and got["counts"].tolist() == want.counts.tolist() and got["summary"] == want.summary
    # a handle made for the call, and no table
    got = discread.disc_read_host(image[:9], [discread.track(np.zeros((9, 2352), np.uint8))], table=False)
    assert got["table"] is None and got["summary"]["n_sectors"] == 9


# ---- composition
W, H = 64, 48


def _str_stream(xa_channel, seed):
    import torch
    import oracle_lib as O
    import str_demux_corpus as C
    from psxavenc_amd import strmux
    s = strmux.settings(fmt=7, codec=0, width=W, height=H, channels=2, xa_channel=xa_channel, tail=strmux.TAIL_COMPLETE)
    d_frames = torch.from_numpy(O.synth_frames(W, H, 5, seed=seed, amp=6)).to(DEV)
    pl = strmux.plan(s, 5)
    d_pcm = torch.from_numpy(C.pcm_for(2, pl.audio_samples_per_sector * (pl.n_audio_sectors + 2) + 100, seed)).to(DEV)
    mux = strmux.StrMuxer((0,))
    d_out, p = mux.encode_device(s, d_frames, d_pcm)
    d_sectors = d_out[0].clone()
    mux.close()
    return s, d_sectors, p


def test_damaged_disc_goes_back_through_the_readers(reader):
    import torch
    import str_demux_corpus as C
    from psxavenc_amd import StrReader, adpcm, disc, discread, xa_disassemble
    streams = [_str_stream(0, 3), _str_stream(2, 4)]
    xs = adpcm.XaSettings(format=adpcm.PSX_AUDIO_XA_FORMAT_XACD, stereo=True, frequency=37800, bits_per_sample=4, file_number=1, channel_number=5)
    per = adpcm.xa_get_samples_per_sector(xs)
    xa = adpcm.xa_encode_streams(xs, C.pcm_for(2, 6 * per, 21)[None], 6 * per, finalize=True).reshape(-1, 2352)
    d_xa = torch.from_numpy(xa).to(DEV)
    lay = disc.layout([0, 1, 2, -1], 3000)
    srcs = [disc.source(streams[0][1], channel=0), disc.source(streams[1][1], channel=2), disc.source(d_xa)]
    d_clean = disc.disc_finish(lay, srcs)
    torch.cuda.synchronize()
    clean = d_clean.cpu().numpy()
    assert not R.check(clean, 3000)[0].any()
    rng = np.random.default_rng(81)
    image = clean.copy()
    form1 = np.flatnonzero((clean[:, 0x12] & 0x20) == 0)
    assert len(form1) >= 10
    for k in rng.choice(form1, 36):
        image[k, rng.integers(0x10, 0x930)] ^= rng.integers(1, 256)
    counts = [st[1].shape[0] for st in streams] + [xa.shape[0]]
    tracks = [D.Track(2352, counts[0], -1, 0), D.Track(2352, counts[1], -1, 2), D.Track(2352, counts[2], 1, 5, 0x04, 0x04)]
    want, views = _read(reader, image, tracks)
    assert want.counts.tolist() == counts and want.summary["n_repaired"] >= 10 and want.summary["n_unrepairable"] == 0
    for t in range(3):
        assert np.array_equal(views[t].cpu().numpy(), clean[t::4][:counts[t]]), t
    str_reader = StrReader(0)
    for t, (s, d_sectors, p) in enumerate(streams):
        bs_stride = (p.max_frame_size + 2015) // 2016 * 2016
        before = str_reader.demux_device(s, d_sectors, 5, bs_stride)
        after = str_reader.demux_device(s, views[t].contiguous(), 5, bs_stride)
        torch.cuda.synchronize()
        for k in ("bs", "sizes", "summary", "table"):
            assert torch.equal(before[k], after[k]), (t, k)
        assert (after["sizes"] > 0).all() and not after["info"][..., 7].any()
    str_reader.close()
    want_units, want_status = xa_disassemble(d_xa, xs)
    units, status = xa_disassemble(views[2].contiguous(), xs)
    torch.cuda.synchronize()
    assert torch.equal(units, want_units) and not status.any() and not want_status.any()
