"""The disc reader's kernel file (psxavenc_amd/csrc/disc_read_kernels.hip) and its host layer (psxhip_disc_read.cpp), their own
text, on the CPU under the host sanitizers: tests/cpu/disc_read_lanes.cpp behind the stand-in's wavefront model
(tests/cpu/hip_lanes/hip_lanes_waves.h), against "psxhip disc read v1" (tests/disc_read_ref.py) byte for byte.

What the GPU tests cannot see and this does: a read outside the image, the records, the span counts or an LDS array (the image
and every output are heap blocks that end where include/psxav_hip.h says the call may reach; LDS arrays stand between red zones);
a barrier, shuffle, ballot or DPP step that not every lane reaches (repair_rounds' round loop must leave workgroup-uniformly);
LDS traffic between wavefronts without a barrier (the three orders -- of workgroups, of wavefronts between barriers, of lanes
between collectives -- must give equal bytes); undefined behaviour the device forgives.

Every case runs through psxhip_disc_read_host (the host layer's staging and workspace layout) and through psxhip_disc_read_device
on blocks of the program's own (padded strides, a table of the caller's).  The last test reads gcov: every line of the kernel file
ran."""
import numpy as np
import pytest

import disc_read_corpus as K
import disc_read_ref as D
import disc_ref as R
import lanes_cpu as L

FILL = 0xA7
KERNEL_FILE = "disc_read_kernels.hip"
# lines of the kernel file that hold code and cannot run from a valid call, with the reason
NOT_REACHED = {}


def _stride(T):
    return T.size if T.stride is None else T.stride


def _record(mode, image, tracks, table=True):
    return dict(mode=mode, image=np.ascontiguousarray(image, dtype=np.uint8).reshape(-1, 2352), tracks=tracks, table=table)


def _write(path, records):
    with open(path, "wb") as f:
        for r in records:
            f.write(np.array([r["mode"], len(r["image"]), len(r["tracks"]), int(r["table"]), FILL], np.int32).tobytes())
            for T in r["tracks"]:
                f.write(np.array([T.size, T.capacity, T.file, T.channel, T.mask, T.value, _stride(T)], np.int32).tobytes())
            f.write(r["image"].tobytes())


_answers = {}


def _want(r):
    """the statement's bytes for one record, in the program's order; computed once per (image, tracks)"""
    key = (r["image"].tobytes(), tuple(r["tracks"]))
    if key not in _answers:
        into = [np.full((T.capacity, _stride(T)), FILL, np.uint8) for T in r["tracks"]]
        _answers[key] = D.read(r["image"], r["tracks"], into=into)
    w = _answers[key]
    parts = []
    for T, buf in zip(r["tracks"], w.tracks):
        if T.capacity:
            parts.append(buf.reshape(-1)[:(T.capacity - 1) * _stride(T) + T.size].tobytes())
    if r["table"]:
        parts.append(w.table.astype(np.int32).tobytes())
    parts.append(w.counts.astype(np.int32).tobytes())
    s = w.summary
    parts.append(np.array([s[k] for k in D.SUMMARY_FIELDS[:-1]], np.int32).tobytes() + np.array([s["n_corrections"]], np.int64).tobytes())
    return parts, w


def _both(image, tracks, table=True):
    return [_record(0, image, tracks, table), _record(1, image, tracks, table)]


# ---- the corpus
def _eight_sources(rng, n):
    spec = [(2336, 16, 1, 0, 0x08), (2352, 0, 1, 1, 0x04), (2048, 0, 2, 0, 0x08), (2336, 0, 2, 1, 0x02), (2352, 8, 3, 0, 0x08),
            (2336, 0, 3, 5, 0x04), (2048, 304, 4, 0, 0x08), (2352, 0, 4, 31, 0x0A)]
    return [R.Source(K.sectors(rng, n, size, pad, forms=rng.integers(1, 3, n).tolist(), kind=kind), size, file=f, channel=c)
            for size, pad, f, c, kind in spec]


SLOTS = [0, 1, 2, -1, 3, 4, 5, 6, -1, 7]


@pytest.fixture(scope="module")
def big():
    """1 025 sectors of eight sources and gaps, mixed forms, a damaged sector every 41"""
    rng = np.random.default_rng(1025)
    srcs = _eight_sources(rng, 103)
    image = R.finish(SLOTS, 20000, srcs, 0, 1025).copy()
    for k in range(5, 1025, 41):
        if image[k, 0x12] & 0x20:
            image[k, 0x500] ^= 0x01
        else:
            image[k] = K.scattered(image[k], 1 + k % 7, rng)
    return srcs, image


def size_records(big):
    """0, 1, 3 and 5 sectors (5 crosses the four-sector workgroup) and 1 025 (one past the count pass's span), every track size with
    padded strides; the largest once per entry point, with a table on the device path and without on the host path"""
    srcs, image = big
    tracks = [D.Track(s.size, 12 if n_t % 2 else 140, s.file, s.channel, stride=s.size + (16 if n_t % 3 == 0 else 0)) for n_t, s in enumerate(srcs)]
    out = []
    for n in (0, 1, 3, 5):
        out += _both(image[:n], tracks) + _both(image[:n], tracks, table=False)
    out += _both(image[:n], [])                                       # no track at all: classify only
    out += [_record(0, image, tracks, table=False), _record(1, image, tracks, table=True)]
    return out


def header_trap(sector, m, e1):
    """two wrong bytes in P column m < 4, rows 1 and 2, whose syndromes name row 0 -- header byte 12 + m, which the rules read as zero
    and never alter: the P pass must leave the column alone (the Q pass then mends both bytes)"""
    a24, a23, a25 = (int(R.GF_EXP[k]) for k in (24, 23, 25))
    e2 = R.gf_div(R.gf_mul(e1, a24 ^ a25), a25 ^ a23)
    bad = sector.copy()
    bad[12 + m + 86] ^= e1
    bad[12 + m + 2 * 86] ^= e2
    s0, s1 = e1 ^ e2, R.gf_mul(a24, e1) ^ R.gf_mul(a23, e2)
    assert s0 and s1 and (int(R.GF_LOG[s1]) - int(R.GF_LOG[s0])) % 255 == 25
    return bad


def damage_records():
    """every damage class in one image, one_bad_column damage, damage that changes the routing key"""
    rng = np.random.default_rng(77)
    clean = K.form1_image(rng, 3 * K.N_DAMAGE_CLASSES + 12, start_lba=9000)
    image = clean.copy()
    classes = K.damage_classes(rng, clean[1::3])
    for k, (name, bad, good, repairable) in enumerate(classes):
        image[1 + 3 * k] = bad
    for k in range(3 * K.N_DAMAGE_CLASSES + 1, 3 * K.N_DAMAGE_CLASSES + 8, 2):
        image[k] = K.one_bad_column(clean[k], rng)
    for m in range(4):
        image[3 * K.N_DAMAGE_CLASSES + 8 + m] = header_trap(clean[3 * K.N_DAMAGE_CLASSES + 8 + m], m, 0x21 + 0x35 * m)
    for at in (12, 15):
        image[0, at] ^= 0x10
    out = _both(image, [D.Track(2352, len(image), 1, 0)])
    rng = np.random.default_rng(78)
    srcs = [R.Source(K.sectors(rng, 6, 2336), 2336, file=1, channel=c) for c in (0, 1)]
    image = R.finish([0, 1], 0, srcs).copy()
    image[2, 0x11] = 1
    image[3, 0x10] = 9
    image[4, 0x12] = 0x20
    image[5, 0x11], image[5, 0x15] = 0, 0
    out += _both(image, [D.Track(2336, 8, 1, 0), D.Track(2336, 8, 1, 1), D.Track(2352, 8, -1, -1)])
    return out, classes


def random_records():
    """64 random sectors; capacities below the count and of zero, first match, submode masks, a 2048-byte track that meets form 2"""
    rng = np.random.default_rng(79)
    image = rng.integers(0, 256, (64, 2352)).astype(np.uint8)
    image[::7, :12] = R.SYNC_BYTES
    image[::4, 0x14:0x18] = image[::4, 0x10:0x14]
    image[::16, 0x92C:] = 0
    image[::3, 0x12] |= 0x20
    image[::3, 0x16] |= 0x20
    tracks = [D.Track(2352, 3, -1, 3), D.Track(2048, 9, -1, -1, 0x04, 0x04, stride=2052), D.Track(2048, 0, -1, -1, 0x02, 0x02),
              D.Track(2336, 40, -1, -1, 0x08, 0x00, stride=2340), D.Track(2352, 2, 200, -1)]
    return _both(image, tracks)


def _check(folder, exe, records):
    src, dst = str(folder / "in.bin"), str(folder / "out.bin")
    _write(src, records)
    raw, at = L.run_orders(exe, src, dst, fibers=True), 0
    for k, r in enumerate(records):
        parts, w = _want(r)
        for p, part in enumerate(parts):
            got = raw[at:at + len(part)]
            if got != part:
                first = next(i for i, (a, b) in enumerate(zip(got, part)) if a != b) if len(got) == len(part) else -1
                raise AssertionError("record %d (mode %d, %d sectors), part %d of %d differs from the statement first at byte %d" % (
                    k, r["mode"], len(r["image"]), p, len(parts), first))
            at += len(part)
    assert at == len(raw)


@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    d = tmp_path_factory.mktemp("disc_read_lanes")
    return d, L.build(d, "disc_read_lanes", L.SANITIZE)


def test_sizes_round_the_workgroup_and_the_span(lanes, big):
    _check(*lanes, size_records(big))


def test_every_damage_class_and_damage_that_changes_the_routing_key(lanes):
    records, classes = damage_records()
    _check(*lanes, records)
    _, w = _want(records[0])
    for k, (name, bad, good, repairable) in enumerate(classes):
        assert (w.table[1 + 3 * k, 2] == D.REPAIRED) == repairable, name
    n3 = 3 * K.N_DAMAGE_CLASSES
    assert (w.table[n3 + 1:n3 + 8:2, 2] == D.REPAIRED).all(), "one_bad_column damage is always repaired"
    assert (w.table[n3 + 8:n3 + 12, 2] == D.REPAIRED).all() and (w.table[n3 + 8:n3 + 12, 3] == 2).all(), "the header traps: two corrections, by Q"
    assert (w.sectors[n3 + 8:n3 + 12, :16] == records[0]["image"][n3 + 8:n3 + 12, :16]).all()
    _, w = _want(records[2])
    assert w.table[:, 0].tolist() == [0, 1] * 6 and w.table[2:6, 3].tolist() == [1, 1, 1, 2]


def test_random_sectors_small_and_zero_capacities(lanes):
    records = random_records()
    _check(*lanes, records)
    s = _want(records[0])[1].summary
    assert s["n_unrepairable"] > 10 and s["n_edc"] > 10 and s["n_dropped"] > 0 and s["n_unclaimed"] > 0 and s["n_empty"] > 0


def test_the_records_reach_every_line(tmp_path, big):
    exe = L.build(tmp_path, "disc_read_lanes", L.COVERAGE)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write(src, size_records(big)[:-2] + damage_records()[0] + random_records())
    L.run(exe, src, dst, sanitized=False)
    cov = L.Coverage(tmp_path, "disc_read_lanes", KERNEL_FILE)
    unvisited = cov.unvisited()
    print("lines that hold code and did not run:", unvisited)
    assert not [x for x in unvisited if x[1] not in NOT_REACHED], [x for x in unvisited if x[1] not in NOT_REACHED]
    assert len(cov.lines) > 150
