"""The statement of "psxhip disc read v1" itself (tests/disc_read_ref.py), without a GPU: what it repairs,
what it refuses to touch, that finish -> read gives every source back, and that its answers are the recorded ones."""
import os

import numpy as np
import pytest

import disc_read_corpus as K
import disc_read_ref as D
import disc_ref as R


@pytest.fixture(scope="module")
def clean():
    return K.form1_image(np.random.default_rng(1701), 64, start_lba=500)


def _one(sector):
    out, st, corr, form = D.read_sectors(sector[None])
    return out[0], int(st[0]), int(corr[0]), int(form[0])


def test_every_damage_class_of_the_specification(clean):
    rng = np.random.default_rng(1702)
    classes = K.damage_classes(rng, clean)
    assert len(classes) == K.N_DAMAGE_CLASSES
    for name, bad, good, repairable in classes:
        assert (bad != good).any(), name
        out, st, corr, form = _one(bad)
        if repairable:
            assert np.array_equal(out, good), name
            assert st == D.REPAIRED and corr >= 1 and form == 1, (name, st, corr)
        else:
            assert np.array_equal(out, bad), name
            assert st == D.UNREPAIRABLE and corr == 0 and form == 1, (name, st, corr)


def test_single_byte_takes_one_correction_per_code(clean):
    """a wrong data byte lies in one P and one Q codeword: the P pass corrects it, the Q pass finds nothing left"""
    rng = np.random.default_rng(1703)
    out, st, corr, form = _one(K.flip(clean[0], [0x400], rng))
    assert np.array_equal(out, clean[0]) and (st, corr) == (D.REPAIRED, 1)
    out, st, corr, form = _one(K.flip(clean[0], [0x8C8 + 7], rng))          # a Q parity byte: in no P codeword
    assert np.array_equal(out, clean[0]) and (st, corr) == (D.REPAIRED, 1)


def test_rounds_are_at_most_four(clean):
    rng = np.random.default_rng(1704)
    for k in range(20):
        bad = K.scattered(clean[k], int(rng.integers(2, 33)), rng)
        calls = []
        orig = D._pass

        def counting(w, syn, at):
            calls.append(1)
            return orig(w, syn, at)
        D._pass = counting
        try:
            w, total = D.repair(bad)
        finally:
            D._pass = orig
        assert len(calls) <= 2 * D.ROUNDS and np.array_equal(w, clean[k]), k


def test_header_bytes_are_outside_the_code(clean):
    for at in (12, 13, 14, 15):
        bad = clean[3].copy()
        bad[at] ^= 0x55
        out, st, corr, form = _one(bad)
        assert np.array_equal(out, bad) and (st, corr, form) == (0, 0, 1), at
    bad = clean[3].copy()
    bad[5] = 0
    out, st, corr, form = _one(bad)
    assert np.array_equal(out, bad) and (st, corr, form) == (D.SYNC, 0, 1)


def test_the_derived_guarantee(clean):
    """200 patterns inside 0x10 .. 0x8C7 with at most one P column holding more than one wrong byte: all repaired"""
    rng = np.random.default_rng(1705)
    for k in range(200):
        good = clean[k % len(clean)]
        bad = K.one_bad_column(good, rng)
        places = np.flatnonzero(bad != good)
        assert len(places) >= 2 and places.min() >= 0x10 and places.max() <= 0x8C7
        cols = np.bincount((places - 12) % 86, minlength=86)
        assert (cols > 1).sum() <= 1
        out, st, corr, form = _one(bad)
        assert np.array_equal(out, good) and st == D.REPAIRED, (k, len(places))


def test_two_bytes_of_a_p_column_never_share_a_q_codeword():
    """the derivation behind the guarantee, on the codeword tables themselves"""
    q_of = np.full(2236, -1)
    for m in range(52):
        q_of[R.Q_DATA_IDX[m]] = m
    assert (q_of >= 0).all()
    for m in range(86):
        col = q_of[R.P_IDX[m]]
        assert len(set(col.tolist())) == 26, m


def test_form2_is_never_altered():
    rng = np.random.default_rng(1706)
    img = R.finish([0], 0, [R.Source(K.sectors(rng, 6, 2336, forms=[2] * 6, kind=0x04), 2336)])
    out, st, corr, form = D.read_sectors(img)
    assert np.array_equal(out, img) and not st.any() and (form == 2).all()
    bad = img.copy()
    bad[0, 0x400] ^= 1
    bad[1, 0x92C:] = 0
    bad[2] = K.burst(img[2], 300, 0x100, rng)
    bad[3, 0x92D] ^= 0x80
    out, st, corr, form = D.read_sectors(bad)
    assert np.array_equal(out, bad) and not corr.any() and (form == 2).all()
    assert st.tolist() == [D.EDC, D.EDC_ABSENT, D.EDC, D.EDC, 0, 0]


def test_copies_that_disagree_about_the_form(clean):
    rng = np.random.default_rng(1707)
    # a form-1 sector whose byte 0x12 says form 2: a candidate (byte 0x16 does not), repaired, form 1
    bad = clean[5].copy()
    bad[0x12] ^= 0x20
    out, st, corr, form = _one(bad)
    assert np.array_equal(out, clean[5]) and (st, form) == (D.REPAIRED, 1)
    # ... and with more damage than the code repairs: the form is byte 0x12's, so it is a form-2 sector with a wrong EDC, untouched
    worse = K.burst(bad, 400, 0x100, rng)
    out, st, corr, form = _one(worse)
    assert np.array_equal(out, worse) and (st & ~D.EDC_ABSENT, corr, form) == (D.EDC | D.SUBHEADER, 0, 2)
    f2 = R.finish([0], 0, [R.Source(K.sectors(rng, 2, 2336, forms=[2, 2], kind=0x04), 2336)])
    # a form-2 sector whose byte 0x16 says form 1: a candidate, not repairable, form 2 by byte 0x12, EDC wrong (byte 0x16 is under it)
    a = f2[0].copy()
    a[0x16] ^= 0x20
    out, st, corr, form = _one(a)
    assert np.array_equal(out, a) and (st, corr, form) == (D.EDC | D.SUBHEADER, 0, 2)
    # a form-2 sector whose byte 0x12 says form 1: unrepairable, untouched
    b = f2[1].copy()
    b[0x12] ^= 0x20
    out, st, corr, form = _one(b)
    assert np.array_equal(out, b) and (st, corr, form) == (D.UNREPAIRABLE | D.SUBHEADER, 0, 1)


def _sources(rng):
    """all three sizes, mixed forms, padded rows, overrides that make (file, channel) the routing key"""
    return [R.Source(K.sectors(rng, 7, 2336, 16, forms=[1, 2, 1, 1, 2, 2, 1]), 2336, file=1, channel=0),
            R.Source(K.sectors(rng, 5, 2352, forms=[2, 1, 2, 1, 1], kind=0x04), 2352, file=1, channel=1),
            R.Source(K.sectors(rng, 4, 2048), 2048, file=2, channel=0, data_subheader=(0, 0, 0x08, 0)),
            R.Source(K.sectors(rng, 3, 2352, forms=[1, 1, 2], kind=0x02), 2352, file=2, channel=31)]


def _tracks(srcs, extra=0):
    return [D.Track(s.size, s.data.shape[0] + extra, s.file, s.channel) for s in srcs]


def _data_of(src, k):
    """(first, last + 1) of the data bytes the finisher takes from sector k of the source, in the source's own layout"""
    lead = 2352 - src.size if src.size != 2048 else 0x18
    sub = src.data_subheader[2] if src.size == 2048 else src.data[k, 0x12 - lead]
    return 0x18 - lead, (0x92C if sub & 0x20 else 0x818) - lead


def test_finish_then_read_returns_every_source():
    rng = np.random.default_rng(1708)
    srcs = _sources(rng)
    slots = [0, 1, -1, 2, 0, 3]                       # a gap, source 0 in two slots
    img = R.finish(slots, 1000, srcs)
    res = D.read(img, _tracks(srcs, extra=2))
    assert res.counts.tolist() == [s.data.shape[0] for s in srcs]
    for t, src in enumerate(srcs):
        for k in range(src.data.shape[0]):
            a, b = _data_of(src, k)
            assert np.array_equal(res.tracks[t][k, a:b], src.data[k, a:b]), (t, k)
        assert not res.tracks[t][src.data.shape[0]:].any(), "slots past the count are untouched"
    s = res.summary
    n = img.shape[0]
    n_null = sum(R.schedule(slots, srcs, j) is None for j in range(n))
    assert s["n_sectors"] == n and s["n_empty"] == n_null and s["n_unclaimed"] == 0 and s["n_dropped"] == 0
    assert s["n_clean"] == s["n_form1"] and s["n_repaired"] == s["n_unrepairable"] == s["n_corrections"] == 0
    assert (res.table[:, 2] & ~D.EMPTY).any() == 0


def test_table_counts_and_summary_add_up():
    rng = np.random.default_rng(1709)
    srcs = _sources(rng)
    slots = [0, 1, -1, 2, 0, 3]
    img = R.finish(slots, 0, srcs)
    good = img.copy()
    f1 = np.flatnonzero((img[:, 0x12] & 0x20) == 0)
    img[f1[0]] = K.scattered(img[f1[0]], 5, rng)
    img[f1[1]] = K.burst(img[f1[1]], 300, 0x40, rng)
    img[f1[2]] = K.flip(img[f1[2]], [0x11], rng)          # the channel byte: routed by the repaired one
    tracks = [D.Track(2336, 3, 1, 0, stride=2400), D.Track(2352, 9, 1, -1), D.Track(2048, 2, -1, -1, 0x08, 0x08)]
    res = D.read(img, tracks)
    tab, s = res.table, res.summary
    n = img.shape[0]
    assert np.array_equal(res.sectors[f1[0]], good[f1[0]]) and np.array_equal(res.sectors[f1[2]], good[f1[2]])
    assert np.array_equal(res.sectors[f1[1]], img[f1[1]])
    for t in range(len(tracks)):
        mine = tab[tab[:, 0] == t]
        assert res.counts[t] == len(mine) and mine[:, 1].tolist() == list(range(len(mine)))
        assert ((mine[:, 2] & D.DROPPED) != 0).tolist() == [o >= tracks[t].capacity for o in range(len(mine))]
    none = tab[tab[:, 0] < 0]
    assert (none[:, 1] == -1).all() and (((none[:, 2] & D.EMPTY) != 0) ^ ((none[:, 2] & D.UNCLAIMED) != 0)).all()
    assert s["n_sectors"] == n == s["n_form1"] + s["n_form2"]
    assert s["n_form1"] == s["n_clean"] + s["n_repaired"] + s["n_unrepairable"]
    assert (s["n_repaired"], s["n_unrepairable"]) == (2, 1) and s["n_corrections"] == int(tab[:, 3].sum()) >= 6
    assert s["n_empty"] + s["n_unclaimed"] + int(res.counts.sum()) == n
    assert s["n_dropped"] == sum(max(0, int(c) - T.capacity) for c, T in zip(res.counts, tracks)) > 0
    assert s["n_unclaimed"] > 0                           # file 2, channel 31, video: no data bit, no file 1
    # a form-2 sector of file 1 / channel 1 went to no 2048-byte track; the 2048-byte track took file 2's data sectors only
    assert not (tab[:, 2] & D.FORM).any()
    res2 = D.read(img, [D.Track(2048, 40)])               # a catch-all 2048-byte track: mask 0 matches everything not empty
    form2 = (res.form == 2) & ((tab[:, 2] & D.EMPTY) == 0)
    assert np.array_equal((res2.table[:, 2] & D.FORM) != 0, form2) and form2.any()
    # stride wider than the sector: bytes between size and stride are never touched
    into = [np.full((T.capacity, T.size if T.stride is None else T.stride), 0xEE, np.uint8) for T in tracks]
    res3 = D.read(img, tracks, into=into)
    assert (res3.tracks[0][:, 2336:] == 0xEE).all() and np.array_equal(res3.tracks[0][:, :2336], res.tracks[0][:, :2336])


def test_refusals_of_the_track_list():
    for bad in (D.Track(2340, 1), D.Track(2336, -1), D.Track(2336, 1, 256), D.Track(2336, 1, -2), D.Track(2336, 1, 0, 32),
                D.Track(2336, 1, 0, -2), D.Track(2336, 1, stride=2332), D.Track(2336, 1, stride=2338)):
        with pytest.raises(R.Invalid):
            D.read(np.zeros((0, 2352), np.uint8), [bad])
    with pytest.raises(R.Invalid):
        D.read(np.zeros((0, 2352), np.uint8), [D.Track(2336, 0)] * 65)
    res = D.read(np.zeros((0, 2352), np.uint8), [D.Track(2336, 0)] * 64)
    assert res.counts.tolist() == [0] * 64 and res.summary["n_sectors"] == 0


def test_recorded_answers():
    """tests/golden/disc_read_ref.npz (make_disc_read_golden.py): a dozen damaged sectors and what the statement said of them"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disc_read_ref.npz"))
    image = g["image"]
    assert image.shape == (12, 2352)
    tracks = [D.Track(*[int(v) for v in row]) for row in g["tracks"]]
    res = D.read(image, tracks)
    assert np.array_equal(res.sectors, g["sectors"]) and np.array_equal(res.table, g["table"]) and np.array_equal(res.counts, g["counts"])
    assert [res.summary[k] for k in D.SUMMARY_FIELDS] == g["summary"].tolist()
    for t in range(len(tracks)):
        assert np.array_equal(res.tracks[t], g["track%d" % t]), t
    assert (g["table"][:, 2] & D.REPAIRED).any() and (g["table"][:, 2] & D.UNREPAIRABLE).any() and (g["table"][:, 2] & D.EDC).any()
