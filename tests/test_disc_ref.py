"""The numpy statement of the disc finisher (tests/disc_ref.py) against itself, against the reference-pinned
oracle where the reference has the arithmetic (header bytes, EDC), and psxhip_disc_plan (host-only) against the statement.  No GPU."""
import os

import numpy as np
import pytest

import disc_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disc_ref.npz")


def _form1_sectors(n, seed):
    s = np.random.default_rng(seed).integers(0, 256, (n, 2352)).astype(np.uint8)
    s[:, 0x12] &= 0xDF
    return s


def test_gf_tables():
    """alpha = 2 generates the field under 0x11D; 3^-1 is 0xF4; the table product is the shift-and-reduce product"""
    assert sorted(R.GF_EXP[:255]) == list(range(1, 256))
    assert R.GF_INV3 == 0xF4 and R.gf_mul(3, 0xF4) == 1

    def slow(a, b):
        r = 0
        while b:
            if b & 1:
                r ^= a
            a = (a << 1) ^ (0x11D if a & 0x80 else 0)
            b >>= 1
        return r
    rng = np.random.default_rng(0)
    for a, b in rng.integers(0, 256, (500, 2)):
        assert R.gf_mul(int(a), int(b)) == slow(int(a), int(b))


def test_closed_form_equals_per_codeword_solve():
    s = _form1_sectors(12, 1)
    closed = R.ecc_closed(s.copy())
    for k in range(len(s)):
        assert np.array_equal(R.ecc_solve(s[k].copy()), closed[k]), k
    assert not np.array_equal(closed[:, 0x81C:], s[:, 0x81C:])
    assert np.array_equal(closed[:, :0x81C], s[:, :0x81C])


def test_all_codewords_of_200_sectors_have_zero_syndromes():
    """86 P + 52 Q codewords each, the header taken as zero; one flipped bit anywhere in the ECC's reach shows in both codes"""
    s = R.ecc_closed(_form1_sectors(200, 2))
    sp, sq = R.syndromes(s)
    assert sp.shape == (200, 86, 2) and sq.shape == (200, 52, 2)
    assert not sp.any() and not sq.any()
    rng = np.random.default_rng(3)
    for k in range(50):
        t = s[k:k + 1].copy()
        at = int(rng.integers(0x10, 0x81C))
        t[0, at] ^= 1 << int(rng.integers(0, 8))
        sp, sq = R.syndromes(t)
        assert (sp.reshape(-1, 2).any(axis=1).sum(), sq.reshape(-1, 2).any(axis=1).sum()) == (1, 1), at
    # the header is outside: Mode 2 takes it as zero
    t = s[:1].copy()
    t[0, 12:16] ^= 0xFF
    sp, sq = R.syndromes(t)
    assert not sp.any() and not sq.any()


def test_codeword_indices_cover_what_they_should():
    """P: every d[0..2063] once; Q: every d[0..2235] once"""
    assert sorted(R.P_IDX[:, :24].ravel()) == list(range(2064))
    assert sorted(R.P_IDX[:, 24:].ravel()) == list(range(2064, 2236))
    assert sorted(R.Q_DATA_IDX.ravel()) == list(range(2236))


@pytest.mark.parametrize("lba", [0, 74, 75, 4349, 4350, 449849])
def test_header_bytes_equal_the_reference(oracle, lba):
    O = oracle
    sec = np.zeros(2352, np.uint8)
    O.lib().orc_cdrom_init_sector(O.ptr(sec, O.u8p), lba, 1)
    assert list(sec[:12]) == list(R.SYNC_BYTES)
    assert list(sec[12:16]) == R.header(lba)
    src = R.Source(np.zeros((1, 2336), np.uint8), 2336)
    out = R.finish([0], lba, [src])
    assert np.array_equal(out[0, :16], sec[:16])


def test_header_limit():
    src = R.Source(np.zeros((2, 2336), np.uint8), 2336)
    R.finish([0], R.LBA_LIMIT - 150 - 2, [src])
    for lba in (R.LBA_LIMIT - 150 - 1, -1):
        with pytest.raises(R.Invalid):
            R.finish([0], lba, [src])


@pytest.mark.parametrize("typ", [1, 2])
def test_edc_words_equal_the_reference(oracle, typ):
    O = oracle
    rng = np.random.default_rng(10 + typ)
    raw = rng.integers(0, 256, (3, 2352)).astype(np.uint8)
    raw[:, 0x12] = (raw[:, 0x12] & 0xDF) | (0x20 if typ == 2 else 0)
    raw[:, 0x14:0x18] = raw[:, 0x10:0x14]
    out = R.finish([0], 1000, [R.Source(raw, 2352)])
    at, end = (0x818, 0x818) if typ == 1 else (0x92C, 0x92C)
    for k in range(3):
        want = raw[k].copy()
        O.lib().orc_cdrom_calculate_checksums(O.ptr(want, O.u8p), typ)
        assert np.array_equal(out[k, at:at + 4], want[at:at + 4]), k
        assert np.array_equal(out[k, 0x10:end], raw[k, 0x10:end])


def test_finish_rules():
    """subheader sources and overrides, the form from the submode bit alone, nothing read past the form-1 data, null sectors"""
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, (3, 2400)).astype(np.uint8)          # 2336-byte sectors with junk behind them
    a[0, 2] |= 0x20
    a[1, 2] &= 0xDF
    a[2, 2] |= 0x20
    b = rng.integers(0, 256, (1, 2048)).astype(np.uint8)
    srcs = [R.Source(a, 2336, file=7, channel=33 & 31), R.Source(b, 2048, data_subheader=(1, 2, 0x08, 0))]
    out = R.finish([0, -1, 1], 0, srcs)
    assert out.shape == (9, 2352)
    assert [R.schedule([0, -1, 1], srcs, j) for j in range(9)] == [(0, 0), None, (1, 0), (0, 1), None, None, (0, 2), None, None]
    assert list(out[0, 0x10:0x14]) == [7, (a[0, 1] & 0xE0) | 1, a[0, 2], a[0, 3]] and np.array_equal(out[0, 0x10:0x14], out[0, 0x14:0x18])
    assert np.array_equal(out[0, 0x18:0x92C], a[0, 8:2332])
    assert np.array_equal(out[3, 0x18:0x818], a[1, 8:0x808])
    changed = a.copy()
    changed[1, 0x808:] ^= 0xFF             # a form-1 sector's bytes past its data (the reference's misplaced .str EDC lies there)
    assert np.array_equal(R.finish([0, -1, 1], 0, [srcs[0]._replace(data=changed), srcs[1]])[3], out[3])
    assert list(out[2, 0x10:0x18]) == [1, 2, 8, 0] * 2 and np.array_equal(out[2, 0x18:0x818], b[0])
    for j in (1, 4, 5, 7, 8):
        assert list(out[j, 0x10:0x18]) == [0, 0, 0x20, 0] * 2 and not out[j, 0x18:0x92C].any() and out[j, 0x92C:].any()
    st, summary = R.check(out, 0)
    assert not st.any() and (summary["n_form1"], summary["n_form2"], summary["n_bad"]) == (2, 7, 0)
    # in pieces
    assert np.array_equal(np.concatenate([R.finish([0, -1, 1], 0, srcs, 0, 5), R.finish([0, -1, 1], 0, srcs, 5, 4)]), out)


def test_check_bits():
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, (4, 2336)).astype(np.uint8)
    raw[:2, 2] &= 0xDF
    raw[2:, 2] |= 0x20
    img = R.finish([0], 500, [R.Source(raw, 2336)])
    assert not R.check(img, 500)[0].any() and not R.check(img, -1)[0].any()
    assert list(R.check(img, 501)[0]) == [R.HEADER] * 4
    for at, k, want in ((5, 0, R.SYNC), (12, 0, R.HEADER), (15, 1, R.HEADER), (0x15, 0, R.SUBHEADER | R.EDC | R.ECC_P | R.ECC_Q), (0x16, 2, R.SUBHEADER | R.EDC), (0x100, 0, R.EDC | R.ECC_P | R.ECC_Q),
                        (0x100, 2, R.EDC), (0x819, 1, R.EDC | R.ECC_P | R.ECC_Q), (0x81C + 100, 0, R.ECC_P | R.ECC_Q), (0x8C8 + 7, 1, R.ECC_Q),
                        (0x92D, 3, R.EDC)):
        bad = img.copy()
        bad[k, at] ^= 0x10
        st, summary = R.check(bad, 500)
        assert st[k] == want and summary["n_bad"] == 1, (at, k, st[k], want)
    bad = img.copy()
    bad[2, 0x92C:] = 0
    assert R.check(bad, 500)[0][2] == R.EDC_ABSENT
    bad[0, 12] = 0x1A                  # not BCD
    assert R.check(bad, -1)[0][0] == R.HEADER


def _c_table(srcs, slot_source, start_lba=0):
    from psxavenc_amd import disc
    keep = [disc.source(s.data, s.size, s.file, s.channel, s.data_subheader) for s in srcs]
    return disc.layout(slot_source, start_lba), keep


@pytest.mark.parametrize("period", [1, 4, 8, 64])
def test_plan_against_the_statement(period):
    from psxavenc_amd import disc
    rng = np.random.default_rng(period)
    for trial in range(30):
        n_src = int(rng.integers(1, min(period, 9) + 1))
        slots = [int(rng.integers(-1, n_src)) for _ in range(period)]
        counts = [slots.count(s) for s in range(n_src)]
        srcs = [R.Source(np.zeros((int(rng.integers(0, 40)) if counts[s] and rng.integers(0, 4) else 0, 2336), np.uint8), 2336) for s in range(n_src)]
        lay, keep = _c_table(srcs, slots)
        assert disc.disc_plan(lay, keep) == R.plan(slots, srcs), (slots, [s.data.shape[0] for s in srcs])
    srcs = [R.Source(np.zeros((5, 2336), np.uint8), 2336), R.Source(np.zeros((0, 2352), np.uint8), 2352)]
    lay, keep = _c_table(srcs, [0] + [-1] * (period - 1))
    assert disc.disc_plan(lay, keep) == 5 * period == R.plan([0] + [-1] * (period - 1), srcs)
    lay, keep = _c_table(srcs, [0] * period)
    assert disc.disc_plan(lay, keep) == period * -(-5 // period)
    lay, keep = _c_table([], [-1] * period)
    assert disc.disc_plan(lay, keep) == 0


def test_plan_refuses_a_source_without_a_slot():
    from psxavenc_amd import _lib, disc
    srcs = [R.Source(np.zeros((5, 2336), np.uint8), 2336), R.Source(np.zeros((1, 2352), np.uint8), 2352)]
    lay, keep = _c_table(srcs, [0, 0, -1])
    with pytest.raises(_lib.PsxHipError) as e:
        disc.disc_plan(lay, keep)
    assert e.value.code == _lib.PSXHIP_EINVAL
    with pytest.raises(R.Invalid):
        R.plan([0, 0, -1], srcs)


def test_golden_fixture_is_the_statement():
    """tests/golden/disc_ref.npz (make_disc_golden.py): a dozen sectors and their finished bytes, recorded"""
    g = np.load(GOLDEN)
    srcs = [R.Source(g["xa"], 2336, file=1, channel=2), R.Source(g["strcd"], 2352), R.Source(g["strv"], 2048, data_subheader=(1, 0, 0x48, 0))]
    slots = [int(x) for x in g["slot_source"]]
    out = R.finish(slots, int(g["start_lba"]), srcs)
    assert out.shape[0] == 12 and np.array_equal(out, g["image"])
    st, summary = R.check(g["image"], int(g["start_lba"]))
    assert not st.any() and summary["n_form1"] + summary["n_form2"] == 12
