"""Streams of an independent BS writer (tests/mdec_foreign_streams.py) through the three CPU readers: the oracle's
(oracle/mdec_decode.c) and the product's parse core (psxavenc_amd/csrc/mdec_parse.h under the host sanitizers) one peek per step and
on the kernel's window schedule.  The writer is pinned first, by frames written out by hand; the corpus is held to its coverage
conditions; and the numpy statement of the reconstruction is compared with a float64 IDCT where coefficients saturate, which no
stream of this project's encoder ever made them do."""
import numpy as np
import pytest

import mdec_decode_corpus as DC
import mdec_foreign_streams as FS
import mdec_recon_ref as R
from test_mdec_parse_cpu import sim  # noqa: F401  (the sanitizer build of the parse core)


# ---------------------------------------------------------------- the writer, against frames written out by hand
def _pack(bits):
    """a bit string -> bytes, by the rule alone: sixteen bits make a word, first bit highest, stored low byte first"""
    bits = bits.replace(" ", "")
    bits += "0" * (-len(bits) % 16)
    out = bytearray()
    for i in range(0, len(bits), 16):
        word = int(bits[i:i + 16], 2)
        out += bytes([word & 255, word >> 8])
    return bytes(out)


def _frame(levels):
    lv = np.zeros((6, 64), np.int64)
    for b, row in enumerate(levels):
        for k, v in row.items():
            lv[b, k] = v
    return lv


HAND_V2 = (      # 16x16, quant scale 5: DCs 5, -1 (0x3FF), -512, 510, 0, 1; +1 at position 1 of block 2 (code 11, sign 0); -2 at
                 # position 2 of block 3 (run 1 level 2: 000110, sign 1); end code 0x1FF
    "0000000101 10"
    "1111111111 10"
    "1000000000 110 10"
    "0111111110 0001101 10"
    "0000000000 10"
    "0000000001 10"
    "0111111111",
    92,
    bytes.fromhex("2000 0038 0500 0200".replace(" ", "")) + bytes.fromhex("6F0180FEFF34800D0108F09F"))

HAND_V3 = (      # 16x16, quant scale 1, deltas Cr +5 (chroma class 3: 110, sign 1, 01), Cb -3 (chroma class 2: 10, sign 0, 0),
                 # Y +200 (luma class 8: 1111110, sign 1, 1001000), -1 (luma class 1: 00, sign 0), 0 (luma zero: 100),
                 # -100 (luma class 7: 111110, sign 0, 011011); end code 0x3FF
    "110 1 01 10"
    "10 0 0 10"
    "1111110 1 1001000 10"
    "00 0 10"
    "100 10"
    "111110 0 011011 10"
    "1111111111",
    66,
    bytes.fromhex("2000003801000300") + bytes.fromhex("8BD644F67C29FF6E00C0"))

HAND_ESCAPE = (  # 16x16 v2, quant scale 65535, block 0: DC 0, -1 at position 3 (run 2 level 1: 0101, sign 1), -300 at position 9
                 # (run 5, no table code: 000001 000101 1011010100), end of block; five empty blocks
    "0000000000 01011 000001 000101 1011010100 10"
    "0000000000 10" "0000000000 10" "0000000000 10" "0000000000 10" "0000000000 10"
    "0111111111",
    109,
    bytes.fromhex("20000038FFFF0200") + bytes.fromhex("1600B60800A40440400000 04F84F".replace(" ", "")))


def test_the_hand_written_frames_are_consistent():
    """the literal bit strings pack, by the word rule alone, to the literal bytes"""
    for bits, nbits, want in (HAND_V2, HAND_V3, HAND_ESCAPE):
        assert len(bits.replace(" ", "")) == nbits
        assert _pack(bits) == want[8:]


def test_writer_produces_the_hand_written_v2_frame():
    lv = _frame([{0: 5}, {0: -1}, {0: -512, 1: 1}, {0: 510, 2: -2}, {0: 0}, {0: 1}])
    assert FS.write(lv, 2, 5) == (HAND_V2[2], HAND_V2[1])
    assert np.array_equal(FS.expected_levels(lv, 2, False)[0], lv)


def test_writer_produces_the_hand_written_v3_frame():
    lv = _frame([{0: 5}, {0: -3}, {0: 200}, {0: -1}, {0: 0}, {0: -100}])
    for wrap in (False, True):
        assert FS.write(lv, 3, 1, wrap) == (HAND_V3[2], HAND_V3[1])
    # the DCs the syntax defines, worked out by hand: 4 * the running sum per component; with the wrap 800 is -224 and -628 is 396
    assert FS.expected_levels(lv, 3, False)[0][:, 0].tolist() == [20, -12, 800, 796, 796, 396]
    assert FS.expected_levels(lv, 3, True)[0][:, 0].tolist() == [20, -12, -224, -228, -228, 396]
    far = _frame([{0: 0}, {0: 0}, {0: 255}, {0: 255}, {0: 255}, {0: 255}])
    far = np.concatenate([far] * 9)                                 # 36 luma blocks of +1020: 32640 after the 32nd, then past int16
    got, running = FS.expected_levels(far, 3, False)
    luma = [b for b in range(54) if b % 6 >= 2]
    assert running[luma].tolist() == [1020 * (i + 1) for i in range(36)]
    assert got[luma, 0].tolist() == [1020 * (i + 1) if i < 32 else 1020 * (i + 1) - 65536 for i in range(36)]


def test_writer_produces_the_hand_written_block_with_a_table_code_an_escape_and_an_eob():
    lv = _frame([{3: -1, 9: -300}, {}, {}, {}, {}, {}])
    assert FS.write(lv, 2, 65535) == (HAND_ESCAPE[2], HAND_ESCAPE[1])
    # the same pairs, both as escapes: 000001 000010 1111111111 and the escape as before
    data, nbits = FS.write(lv, 2, 65535, escape_policy="always")
    bits = ("0000000000 000001 000010 1111111111 000001 000101 1011010100 10"
            "0000000000 10" "0000000000 10" "0000000000 10" "0000000000 10" "0000000000 10" "0111111111")
    assert nbits == 109 + 17 and data[8:] == _pack(bits)
    # and an escape of level 0 at a chosen position: 000001 000000 0000000000 at position 1; the -1 is then two positions on
    data, nbits = FS.write(lv, 2, 65535, escape_policy={(0, 1)})
    bits = ("0000000000 000001 000000 0000000000 011 1 000001 000101 1011010100 10"
            "0000000000 10" "0000000000 10" "0000000000 10" "0000000000 10" "0000000000 10" "0111111111")
    assert nbits == 109 + 22 - 1 and data[8:] == _pack(bits)                  # (run 1 level 1 is 011: one bit shorter than 0101)


# ---------------------------------------------------------------- the writer against the readers
def _check_readers(oracle, sim, pairs):
    cases = [c for c, _ in pairs]
    step, windowed = sim(cases, True), sim(cases, True, windowed=True)
    for (c, want), a, b in zip(pairs, step, windowed):
        got = {"oracle": DC.oracle_decode(c), "step": a, "windowed": b}
        for name, g in got.items():
            assert g[0] == want[0] == 0, (c.name, name, g[0])
            assert (g[2], g[3], g[4]) == want[2:], (c.name, name, g[2:], want[2:])
            assert np.array_equal(g[1], want[1]), (c.name, name)
    return len(cases)


def test_every_foreign_stream_decodes_to_what_was_written(oracle, sim):  # noqa: F811
    pairs = FS.clean_cases()
    assert _check_readers(oracle, sim, pairs) == len(pairs) == 1260


def test_the_larger_frames_decode_to_what_was_written(oracle, sim):  # noqa: F811
    pairs = FS.large_cases()
    assert _check_readers(oracle, sim, pairs) == 3
    bits = {c.name: want[4] for c, want in pairs}
    assert bits["v2 320x240 dense always"] == 1800 * (10 + 63 * 22 + 2) + 10 and bits["v2 320x240 empty"] == 1800 * 12 + 10
    assert bits["v3dc 320x240 dense always"] == 600 * 1404 + 1200 * 1403 + 10         # 16-bit chroma DCs, 15-bit luma DCs


def test_negative_cases_give_their_status_from_all_three_readers(oracle, sim):  # noqa: F811
    pairs = FS.negative_cases()
    cases = [c for c, _ in pairs]
    step, windowed = sim(cases, True), sim(cases, True, windowed=True)
    seen, cut = set(), set()
    for (c, want), a, b in zip(pairs, step, windowed):
        o = DC.oracle_decode(c)
        if want is None:                                 # a frame cut before its end code: whatever the oracle says
            want = o[0]
            cut.add(want)
        assert o[0] == a[0] == b[0] == want != 0, (c.name, o[0], a[0], b[0], want)
        assert (o[2], o[3]) == (a[2], a[3]) == (b[2], b[3]) == (7, 2 if c.name.startswith("v2") else 3), c.name
        seen.add(want)
    assert {-3, -6, -7} <= seen and cut
    assert -8 not in seen                                # mdec_decode_corpus.REACHABLE's note: the end code cannot lie past the end
    assert seen <= DC.REACHABLE[2] | DC.REACHABLE[3]


# ---------------------------------------------------------------- coverage: what a later edit of a generator must not thin
def test_the_corpus_covers_what_it_is_for():
    pairs = FS.clean_cases()
    ac = FS.books()[0]
    table, esc_runs, esc_coded, esc_zero = set(), set(), 0, 0
    pos63 = {(2, 0): 0, (3, 0): 0, (3, 1): 0}
    dc_classes = set()
    outside, cast, wraps, below, above = 0, 0, 0, 0, 0
    by = {}
    sizes = set()
    for c, want in pairs:
        wr = c.written
        table |= set(wr.table_codes)
        esc_runs |= {e[2] for e in wr.escapes}
        esc_coded += sum(1 for e in wr.escapes if e[4])
        esc_zero += sum(1 for e in wr.escapes if e[3] == 0)
        assert all(want[1][e[0], e[1]] == e[3] for e in wr.escapes)
        pos63[(wr.version, wr.wrap)] += int((want[1][:, 63] != 0).sum()) + sum(1 for e in wr.escapes if e[1] == 63 and e[3] == 0)
        dc_classes |= set(wr.dc_classes)
        if wr.version == 3 and not wr.wrap:
            outside += bool((np.abs(wr.running) > 512).any())
            cast += bool((wr.running != want[1][:, 0]).any())
            below += bool((wr.running < -32768).any())
            above += bool((wr.running > 32767).any())
            assert np.array_equal(wr.running.astype(np.int16), want[1][:, 0])
        if wr.version == 3 and wr.wrap:
            unwrapped = FS.expected_levels(wr.given, 3, False)[1]
            wraps += bool((unwrapped != want[1][:, 0]).any())
            assert (want[1][:, 0] >= -512).all() and (want[1][:, 0] <= 511).all()
        by.setdefault((wr.version, wr.wrap, c.w, c.h, wr.cls, wr.policy), set()).add(want[2])
        sizes.add((c.size - 8) % 4 if c.size % 2 == 0 else -1)
        assert (want[1][:, 1:] >= -512).all() and (want[1][:, 1:] <= 511).all()
    assert table == {(r, l, neg) for (r, l) in ac for neg in (False, True)} and len(table) == 222
    assert esc_coded >= 50, esc_coded
    assert esc_runs >= set(range(63)), sorted(set(range(63)) - esc_runs)
    assert esc_zero >= 20, esc_zero
    assert min(pos63.values()) >= 10, pos63
    assert dc_classes == {(luma, cls, sign) for luma in (False, True) for cls in range(1, 9) for sign in (-1, 1)} | {(False, 0, 0), (True, 0, 0)}
    assert outside >= 1 and cast >= 1 and wraps >= 1, (outside, cast, wraps)
    assert below >= 1 and above >= 1, (below, above)     # the int16 cast in either direction
    # every codec x size x class x policy with every header scale
    want_keys = {(v, wr, w, h, cls, pol) for (v, wr) in FS.CODECS for (w, h) in FS.SIZES for cls in FS.BLOCK_CLASSES
                 for pol in (("needed",) if cls == "empty" else ("at",) if cls == "zeros" else FS.POLICIES)}
    assert set(by) == want_keys and all(v == set(FS.SCALES) for v in by.values())
    assert sizes == {-1, 0, 2}                           # odd; a multiple of 4; even and not a multiple of 4
    how = {}
    for c, _ in pairs:                                   # each of the three sizings really happens, zero fill included
        wr = c.written
        how[wr.sizing] = how.get(wr.sizing, 0) + 1
        extra = c.data[wr.bytes_written:c.size]
        assert {"exact": c.size == wr.bytes_written, "junk": c.size == wr.bytes_written + 1 and extra.tolist() == [0xFF],
                "fill": c.size == wr.bytes_written + 2 and c.size % 4 == 0 and extra.tolist() == [0, 0],
                "no fill": c.size == wr.bytes_written and c.size % 4 == 0}[wr.sizing], c.name
    assert min(how.get(k, 0) for k in ("exact", "junk", "fill")) >= 100, how
    # v2 DCs: the named ones, 0x3FF = -1 among them; v3 deltas: the named ones
    v2 = np.concatenate([want[1][:, 0] for c, want in pairs if c.written.version == 2])
    assert set(FS.V2_DC_SET) <= set(v2.tolist()) and v2.min() == -512 and v2.max() == 510
    v3 = np.concatenate([c.written.given[:, 0] for c, _ in pairs if c.written.version == 3])
    assert {-255, -128, -1, 0, 1, 128, 255} <= set(FS.V3_DELTA_SET) <= set(v3.tolist())
    # both densities: 12 bits per block, 1404 bits per block
    for group in (pairs, FS.large_cases()):
        per_block = {n for c, _ in group for n in c.written.block_bits}
        assert 12 in per_block and max(per_block) == 16 + 63 * 22 + 2 == 1404
    assert {(c.w, c.h, c.written.cls) for c, _ in FS.large_cases()} == {(320, 240, "dense"), (320, 240, "empty")}


# ---------------------------------------------------------------- the statement where coefficients saturate
STATEMENT_SCALES = (0, 1, 2, 8, 63, 64, 200, 16383, 16384, 65535)


@pytest.fixture(scope="module")
def statement_levels():
    """the levels of every case of the corpus, the 320x240 frames included, and blocks whose DC goes over the whole int16 range"""
    rows = [want[1] for _, want in FS.clean_cases() + FS.large_cases()]
    assert len(rows) == 1263 and sum(r.shape[0] for r in rows) == 57960 + 3 * 1800
    edge = np.array([-32768, -32767, -1025, -1024, -1023, -513, -512, -1, 0, 1, 511, 512, 1023, 1024, 1025, 32766, 32767])
    sweep = np.concatenate([np.arange(-32768, 32768, 16), edge])
    dc = np.zeros((sweep.size * 2, 64), np.int16)
    dc[:sweep.size, 0] = sweep                           # the DC alone
    dc[sweep.size:, 0] = sweep                           # the DC beside a few coefficients
    dc[sweep.size:, 1:6] = np.random.default_rng(5).integers(-6, 7, (sweep.size, 5))
    return np.concatenate(rows + [dc])


def test_statement_is_within_its_bound_of_float64_where_coefficients_saturate(oracle, statement_levels):
    lv = statement_levels
    worst, largest = 0, 0
    for qs in STATEMENT_SCALES:
        f8 = R.dequantise(lv, qs)
        got = R.idct_blocks(f8).astype(np.int64)
        bound = R.pixel_bound(f8)
        d = np.abs(got - R.real_pixels(f8)).max(axis=(1, 2))
        assert (d <= bound).all(), (qs, int(d.max()), int(bound[d > bound].min()))
        worst, largest = max(worst, int(d.max())), max(largest, int(bound.max()))
        sat = R.saturating_blocks(lv, qs)
        if qs >= 63:
            assert sat.any(), qs
        if qs in (1, 2):
            assert (~sat).any(), qs
        if qs:                                           # both references are in use at every scale that scales anything
            assert sat.any() and (~sat).any(), qs
        # where nothing saturates the oracle's float reconstruction (which has no clamp) is the reference, as in test_mdec_recon_ref.py
        keep = np.flatnonzero(~sat)
        assert keep.size
        pad = np.zeros(((-keep.size) % 6, 64), np.int16)
        sub = np.concatenate([lv[keep], pad])
        hh = 16 * (sub.shape[0] // 6)                    # the oracle reconstructs frames: one column of macroblocks holds the blocks
        want = oracle.mdec_reconstruct(16, hh, np.ascontiguousarray(sub, np.int16), qs).astype(np.int64)
        f8s = R.dequantise(sub, qs)
        mine = R.place(16, hh, R.idct_blocks(f8s)).astype(np.int64)
        b = R.place(16, hh, np.minimum(np.broadcast_to(R.pixel_bound(f8s)[:, None, None], f8s.shape), 255)).astype(np.int64)
        assert (np.abs(mine - want) <= b).all(), (qs, int(np.abs(mine - want).max()))
    print("statement vs float64 over %d blocks x %d scales: worst |difference| %d, largest bound %d" % (lv.shape[0], len(STATEMENT_SCALES), worst, largest))
