"""The seam kernels' file (psxavenc_amd/csrc/spu_seam_kernels.hip, and with it spu_seam_core.h), its own text, on the CPU under the
host sanitizers: tests/cpu/spu_seam_lanes.cpp behind the stand-in's wavefront model, in three lane orders, and once under gcov.

The step kernel is driven through whole encodes of the corpus bank (tests/spu_seam_corpus.py) with the statement's encoder between
its launches -- the reference's, or the beam statement -- and must arrive at the statement's outcomes, retire exactly the fixed
entries and re-arm the others with s_0.  The report kernel judges the reference's banks, the statement's STEADY banks and one
hand-made bank that never settles, with and without PCM, against the statement's two whole decodes.  What the GPU tests cannot see:
a block or a sample read outside its buffer (every table here ends with its last element), undefined behaviour in the arithmetic."""
import ctypes as C

import numpy as np
import pytest

import lanes_cpu as L
import spu_bank_corpus as B
import spu_seam_corpus as K
import spu_seam_ref as S
from test_spu_bank_lanes_cpu import Entry

KERNEL_FILE, CORE_FILE = "spu_seam_kernels.hip", "spu_seam_core.h"
SEAM_DTYPE = np.dtype([("seam_block", "<i4"), ("first_units", "<i4"), ("first_peak", "<i4"), ("settled", "<i4"), ("first_sse", "<u8"),
                       ("pass1_err", "<u8"), ("pass2_err", "<u8")])


def step_record(s, ents, pcm, beam):
    """-> (the record, the statement's outcomes, the units a body keeps in the device table: 0 once fixed)"""
    p = B.plan(s, ents)
    t = S.seam_tables(s, ents, p)
    trace = []
    _, outcome = S.encode_entries([S.padded(e, pcm) for e in ents], t["seams"], beam, S.STEADY, trace)
    # the states of the chains encoded once: an intro's is s_0 of its entry, the others are never looked at
    first = np.full((t["first"], 2), 0x3C3C, np.int32)
    for entry, intro in t["bodies"]:
        if intro >= 0:
            first[intro] = trace[0][entry]
    bodies = [entry for entry, _ in t["bodies"]]
    tables = []
    for k in range(S.PASSES):
        sk, ek = np.full((len(bodies), 2), 0x7777, np.int32), np.full((len(bodies), 2), 0x7777, np.int32)
        for j, entry in enumerate(bodies):
            if entry in trace[1 + k]:
                sk[j], ek[j] = trace[1 + k][entry]
        tables += [sk, ek]
    head = np.array([0, len(bodies), t["first"], len(ents), S.PASSES, 0, 0, 0], np.int32)
    parts = [head, np.array([i for _, i in t["bodies"]], np.int32), np.array(bodies, np.int32),
             np.array([c[3] for c in t["chains"][t["first"]:]], np.int32), first] + tables
    left = [0 if outcome[entry] < S.PASSES else t["chains"][t["first"] + j][3] for j, entry in enumerate(bodies)]
    return b"".join(a.tobytes() for a in parts), np.array(outcome, np.int32), np.array(left, np.int32)


def report_record(s, ents, bank, pcm):
    n = B.pcm_elements(ents)
    head = np.array([1, s["fmt"], s["alignment"], int(s["no_dummy"]), s["bank_alignment"], len(ents), int(pcm is not None), n if pcm is not None else 0],
                    np.int32)
    arr = (Entry * len(ents))(*[Entry(e["pcm_offset"], e["samples"], e["freq"], e["loop"], int(e["enable_loop"]), e["name"].encode()[:16])
                                for e in ents])
    return head.tobytes() + bytes(arr) + bank.tobytes() + (pcm[:n].tobytes() if pcm is not None else b"")


def statement_report(s, ents, bank, pcm):
    p = B.plan(s, ents)
    want = np.zeros(len(ents), SEAM_DTYPE)
    for i, (e, base, row) in enumerate(zip(ents, p["unit_base"], p["rows"])):
        r = S.report(bank[16 * base:16 * (base + row[3])].reshape(-1, 16), S.seam_block(s, e), None if pcm is None else S.padded(e, pcm))
        want[i] = tuple(r[f] for f in S.FIELDS)
    return want


def never_settles():
    """one entry of three blocks, the loop at block 0: filter 1, shift 12, the first code +1 and nothing else.  Every value 0 .. 8 is
    a fixed point of (60 p + 32) >> 6, so pass 1 sits at 1, pass 2 at 2, pass 3 at 3: the passes never meet and b2 != b"""
    s = B.settings(B.SPU, 16, True, 16)
    ents = B.placed([B.entry(84, 22050, 0, True, "climb"), B.entry(30, 22050, -1, False, "other")])
    pcm = np.zeros(B.pcm_elements(ents) + 2, np.int16)
    bank, p = B.ref_bank(s, ents, pcm)
    bank = bank.copy()
    for u in range(3):
        at = 16 * (p["unit_base"][0] + u)
        bank[at], bank[at + 2:at + 16] = 0x1C, 0
    bank[16 * p["unit_base"][0] + 2] = 0x01
    return s, ents, bank, pcm


@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    d = tmp_path_factory.mktemp("spu_seam_lanes")
    return d, L.build(d, "spu_seam_lanes", L.SANITIZE)


def step_cases():
    ents, pcm = K.bank()
    return [step_record(K.MIXED_SETTINGS[k], ents, pcm, beam) for k, beam in ((0, 0), (2, 0), (3, 2))]


def report_cases():
    """[(record, the statement's report)]"""
    ents, pcm = K.bank()
    out = []
    for k, mode, with_pcm in ((0, S.OFF, True), (0, S.STEADY, True), (2, S.STEADY, False), (3, S.OFF, False), (2, S.OFF, True)):
        bank = K.expected(k, 0, mode)[0]
        x = pcm if with_pcm else None
        out.append((report_record(K.MIXED_SETTINGS[k], ents, bank, x), statement_report(K.MIXED_SETTINGS[k], ents, bank, x)))
    s, e2, bank, x = never_settles()
    for with_pcm in (True, False):
        out.append((report_record(s, e2, bank, x if with_pcm else None), statement_report(s, e2, bank, x if with_pcm else None)))
    return out


def test_the_step_sequence_arrives_at_the_statement_s_outcomes(lanes):
    folder, exe = lanes
    cases = step_cases()
    src, dst = str(folder / "step_in.bin"), str(folder / "step_out.bin")
    with open(src, "wb") as f:
        f.write(b"".join(c[0] for c in cases))
    raw, at = np.frombuffer(L.run_orders(exe, src, dst, fibers=True), np.int32), 0
    for k, (_, outcome, left) in enumerate(cases):
        got = raw[at:at + outcome.size + left.size]
        at += got.size
        assert np.array_equal(got[:outcome.size], outcome), (k, got[:outcome.size].tolist(), outcome.tolist())
        assert np.array_equal(got[outcome.size:], left), "case %d: the fixed bodies are retired, the others keep their units" % k
        assert (outcome == 0).sum() >= 2 and ((outcome >= 1) & (outcome < S.PASSES)).sum() >= 2 and (outcome == S.PASSES).sum() >= 2
    assert at == raw.size


def test_the_report_is_the_statement_s_two_whole_decodes(lanes):
    folder, exe = lanes
    cases = report_cases()
    src, dst = str(folder / "report_in.bin"), str(folder / "report_out.bin")
    with open(src, "wb") as f:
        f.write(b"".join(c[0] for c in cases))
    raw, at = np.frombuffer(L.run_orders(exe, src, dst, fibers=True), SEAM_DTYPE), 0
    for k, (_, want) in enumerate(cases):
        got = raw[at:at + want.size]
        at += want.size
        bad = np.flatnonzero(got != want)
        assert not bad.size, "report %d, entry %d: %s, the statement has %s" % (k, bad[0], got[bad[0]], want[bad[0]])
    assert at == raw.size
    climb = cases[-2][1][0]
    assert (climb["seam_block"], climb["first_units"], climb["first_peak"], climb["settled"], climb["first_sse"]) == (0, 3, 1, 0, 84)
    assert climb["pass1_err"] == 84 and climb["pass2_err"] == 4 * 84
    assert C.sizeof(C.c_int32) * 4 + 24 == SEAM_DTYPE.itemsize == 40


def test_the_records_reach_every_line(tmp_path):
    exe = L.build(tmp_path, "spu_seam_lanes", L.COVERAGE)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(b"".join([c[0] for c in step_cases()[:1]] + [c[0] for c in report_cases()[1:3]]))
    L.run(exe, src, dst, sanitized=False)
    total = 0
    for name in (KERNEL_FILE, CORE_FILE):
        cov = L.Coverage(tmp_path, "spu_seam_lanes", name)
        unvisited = cov.unvisited()
        print(name, "lines that hold code and did not run:", unvisited)
        assert not unvisited, (name, unvisited)
        total += len(cov.lines)
    assert total > 60
