"""The sound bank's kernel file (psxavenc_amd/csrc/spu_bank_kernels.hip), its own text, on the CPU under the host sanitizers:
tests/cpu/spu_bank_lanes.cpp behind the stand-in's wavefront model (tests/cpu/hip_lanes/hip_lanes_waves.h; the check kernel reduces a
wavefront's bits with wave_ops.h), the rows and tiles built by the plan module's own text, in three lane orders, and once under gcov.

The bank is tests/spu_bank_corpus.py's: about 40 entries mixing every length of the sweep with loop points at 0, inside, on the last
block and beyond the end, loops on and off, empty entries, names of 0, 5 and 16 characters and three rates, framed under both
formats, with and without the dummy block, alignments 16 / 64 / 2048 and bank alignments 16 / 2048.  The data blocks come from the
reference build; the expected bytes are ref_spu_file of tests/golden/make_spufile_golden.py per entry, placed by the restated plan.
The frame kernel is handed a buffer of 0xA5 that holds the data blocks alone, between guards.  What the GPU tests cannot see: a word
read or written outside the bank (the blocks here end with their last byte), a cross-lane operation not every lane reaches, undefined
behaviour in the index arithmetic."""
import ctypes as C

import numpy as np
import pytest

import lanes_cpu as L
import spu_bank_corpus as B

FILL, GUARD = 0xA5, 64
KERNEL_FILE = "spu_bank_kernels.hip"


class Entry(C.Structure):
    """psxhip_spu_bank_entry_t"""
    _fields_ = [("pcm_offset", C.c_int64), ("samples", C.c_int64), ("audio_frequency", C.c_int32), ("audio_loop_point", C.c_int32),
                ("enable_loop", C.c_int32), ("name", C.c_char * 16)]


def record(kind, s, entries, bank):
    head = np.array([kind, s["fmt"], s["alignment"], int(s["no_dummy"]), s["bank_alignment"], len(entries), GUARD, FILL], np.int32)
    arr = (Entry * len(entries))(*[Entry(e["pcm_offset"], e["samples"], e["freq"], e["loop"], int(e["enable_loop"]), e["name"].encode()[:16])
                                   for e in entries])
    assert C.sizeof(Entry) == 48
    return head.tobytes() + bytes(arr) + bank.tobytes()


def tiled_banks():
    """two small banks whose tiles are more than one per part: 4100 data blocks, and padding of more than 4096 words"""
    long = B.placed([B.entry(1, 22050, 0, False, "a"), B.entry(4100 * 28 - 5, 44100, B.loop_ms("last", 4100 * 28 - 5, 44100), True, "long"),
                     B.entry(29, 11025, -1, False, "z")])
    return [(B.settings(B.VAG, 64, False, 16), long), (B.settings(B.SPU, 1 << 17, False, 2048), B.placed([B.entry(57, 22050, 1, False), B.entry(0)]))]


@pytest.fixture(scope="module")
def banks():
    """[(settings, entries, expected bank, restated plan)]"""
    out = []
    mixed = B.mixed_entries()
    for s, entries in [(s, mixed) for s in B.MIXED_SETTINGS] + tiled_banks():
        bank, p = B.ref_bank(s, entries, B.synth(entries))
        out.append((s, entries, bank, p))
    return out


@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    d = tmp_path_factory.mktemp("spu_bank_lanes")
    return d, L.build(d, "spu_bank_lanes", L.SANITIZE)


def frame_records(banks):
    return [record(0, s, entries, B.data_only(bank, p, FILL)) for s, entries, bank, p in banks]


def check_records(banks):
    """per bank the clean bank, then one corrupted copy per kind; and what the statuses must be"""
    src, want = [], []
    for s, entries, bank, p in banks:
        src.append(record(1, s, entries, bank))
        want.append(np.zeros(len(entries), np.int32))
        for what, i, at, mask, bit in B.corruptions(s, entries, p):
            bad = bank.copy()
            bad[at] ^= mask
            w = np.zeros(len(entries), np.int32)
            w[i] = bit
            src.append(record(1, s, entries, bad))
            want.append(w)
    return src, want


def test_the_mixed_bank_mixes_what_it_says(banks):
    s, entries, bank, p = banks[1]
    rows = p["rows"]
    assert 38 <= len(entries) <= 45
    assert {e["samples"] for e in entries} >= {0, 1, 27, 28, 29, 56, 1125}
    assert any(r[6] == 0 and r[3] > 1 for r in rows) and any(0 < r[6] < r[3] - 1 for r in rows) and any(r[6] == r[3] - 1 and r[3] > 1 for r in rows)
    assert any(e["loop"] >= 0 and r[6] < 0 and r[3] > 0 for e, r in zip(entries, rows)), "a loop point beyond the end"
    assert any(r[3] == 0 and r[4] == 0 for r in rows) and any(r[3] == 0 and r[4] == 1 for r in rows)
    assert {len(e["name"]) for e in entries} >= {0, 5, 16} and {e["freq"] for e in entries} == {11025, 22050, 44100}
    # an empty SPU file and a header-only VAG: no dummy, a loop, no samples
    for (s2, _, _, p2), size in ((banks[2], 0), (banks[3], 48)):
        assert s2["no_dummy"] and any(r[3] == 0 and r[4] == 0 and z == size for r, z in zip(p2["rows"], p2["sizes"]))
    kinds = [{c[0] for c in B.corruptions(s_, e_, p_)} for s_, e_, _, p_ in banks[:4]]
    assert set.union(*kinds) == {"header byte", "frequency field", "dummy byte", "stray flag on a middle block", "missing LOOP_START", "trap byte",
                                 "pad byte", "gap byte"}
    assert sum(t[1] == 0 for t in banks[5][3]["tiles"]) > 2 and sum(t[1] == 1 for t in banks[4][3]["tiles"]) == 4


def test_frame_kernel_writes_the_reference_files_between_the_guards(lanes, banks):
    folder, exe = lanes
    src, dst = str(folder / "frame_in.bin"), str(folder / "frame_out.bin")
    with open(src, "wb") as f:
        f.write(b"".join(frame_records(banks)))
    raw, at = np.frombuffer(L.run_orders(exe, src, dst, fibers=True), np.uint8), 0
    for k, (s, entries, bank, p) in enumerate(banks):
        got = raw[at:at + bank.size + 2 * GUARD]
        at += got.size
        assert (got[:GUARD] == FILL).all() and (got[GUARD + bank.size:] == FILL).all(), "bank %d: a guard byte was written" % k
        body = got[GUARD:GUARD + bank.size]
        if not np.array_equal(body, bank):
            first = int(np.flatnonzero(body != bank)[0])
            entry = max(i for i, o in enumerate(p["offsets"]) if o <= first)
            raise AssertionError("bank %d differs from the reference's files first at byte %d (entry %d, its byte %d)" % (
                k, first, entry, first - p["offsets"][entry]))
    assert at == raw.size


def test_check_kernel_names_each_corruption_and_nothing_else(lanes, banks):
    folder, exe = lanes
    src, dst = str(folder / "check_in.bin"), str(folder / "check_out.bin")
    records, want = check_records(banks)
    with open(src, "wb") as f:
        f.write(b"".join(records))
    raw, at = np.frombuffer(L.run_orders(exe, src, dst, fibers=True), np.int32), 0
    for k, w in enumerate(want):
        got = raw[at:at + w.size]
        at += w.size
        assert np.array_equal(got, w), "check record %d: status %s at entries %s, wanted %s" % (
            k, got[np.flatnonzero(got != w)].tolist(), np.flatnonzero(got != w).tolist(), w[np.flatnonzero(got != w)].tolist())
    assert at == raw.size


def test_the_records_reach_every_line(tmp_path, banks):
    exe = L.build(tmp_path, "spu_bank_lanes", L.COVERAGE)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(b"".join(frame_records(banks[:4]) + check_records(banks[:2])[0]))
    L.run(exe, src, dst, sanitized=False)
    cov = L.Coverage(tmp_path, "spu_bank_lanes", KERNEL_FILE)
    unvisited = cov.unvisited()
    print("lines that hold code and did not run:", unvisited)
    assert not unvisited, unvisited
    assert len(cov.lines) > 40
