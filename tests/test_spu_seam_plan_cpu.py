"""The seam tables of the sound bank's plan module (psxavenc_amd/csrc/spu_bank_plan.cpp; "psxhip SPU loop seam v1", DESIGN.md section
24) on the CPU, without HIP and under the host sanitizers, the way tests/test_spu_bank_plan_cpu.py checks the rest of the plan: g++
builds spu_bank_plan.cpp and the driver (tests/cpu/spu_seam_plan_check.cpp) and nothing else.  The expectations are the restatement
of tests/spu_seam_ref.py; what the plan derived before it had seam tables is compared with tests/spu_bank_corpus.py's restatement
once more, through this driver."""
import itertools
import os
import shutil
import subprocess

import pytest

import spu_bank_corpus as B
import spu_seam_corpus as K
import spu_seam_ref as S
from test_spu_bank_plan_cpu import ROOT, bank_lines

MAX_SAMPLES = 0x7FFFFFFF - 28


def run_driver(exe, tmp, banks):
    src = os.path.join(tmp, "banks.txt")
    with open(src, "w") as f:
        for lines in banks:
            f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), "the sanitizer build reported (exit %d):\n%s" % (r.returncode, r.stderr[-4000:])
    out = []
    for line in r.stdout.splitlines():
        kind = line.split(" ", 1)[0]
        if kind in "ecbt":
            out[-1][kind].append(tuple(int(v) for v in line.split()[1:]))
        else:
            rc, rest = line.split(" | ", 1)
            out.append(dict(rc=int(rc), head=[int(v) for v in rest.split()] if rc == "0" else rest, e=[], c=[], b=[], t=[]))
    assert len(out) == len(banks)
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build psxavenc_amd/csrc/spu_bank_plan.cpp and tests/cpu/spu_seam_plan_check.cpp")
    tmp = str(tmp_path_factory.mktemp("spu_seam_plan"))
    exe = os.path.join(tmp, "spu_seam_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe,
                    os.path.join(ROOT, "psxavenc_amd/csrc/spu_bank_plan.cpp"), os.path.join(ROOT, "tests/cpu/spu_seam_plan_check.cpp")], check=True)
    return lambda banks: run_driver(exe, tmp, banks)


def sweep_entries():
    """samples 0, 1, 28, 29, 56, 1125 with loops on and off, a loop point nowhere, at 0, inside, in the last block and behind the end"""
    out = []
    for samples, enable_loop, kind in itertools.product((0, 1, 28, 29, 56, 1125), (False, True), ("none", "zero", "inside", "last", "beyond")):
        out.append(B.entry(samples, 22050, B.loop_ms(kind, samples, 22050), enable_loop, "n%d" % samples))
    return B.placed(out)


SWEEP = [B.settings(fmt, alignment, no_dummy, bank_alignment) for fmt, no_dummy, alignment, bank_alignment in
         itertools.product((B.SPU, B.VAG), (False, True), (16, 2048), (16, 2048))]


def assert_bank(s, entries, g):
    p = B.plan(s, entries)
    t = S.seam_tables(s, entries, p)
    assert g["rc"] == 0, g["head"]
    assert g["head"] == [p["total"], sum(r[3] for r in p["rows"]), len(p["tiles"]), t["first"], t["body"]]
    assert g["t"] == p["tiles"]
    for i, (e, line) in enumerate(zip(entries, g["e"])):
        # what the plan derived before: layout, row, chain, unit base
        assert line[:2] == (p["offsets"][i], p["sizes"][i]) and line[2:10] == p["rows"][i], (s, i)
        assert line[10:16] == (e["pcm_offset"], 1, e["samples"], B.blocks_of(e), 1, p["unit_base"][i]), (s, i)
        # the seam block and the report's row
        assert line[16] == t["seams"][i], (s, i, e)
        assert line[17:] == (e["pcm_offset"], e["samples"], p["unit_base"][i], B.blocks_of(e), t["seams"][i]), (s, i)
    assert g["c"] == t["chains"]
    assert g["b"] == t["bodies"]
    return p, t


def test_the_seam_tables_are_the_restated_rule_over_the_sweep(driver):
    entries = sweep_entries()
    got = driver([bank_lines(s, entries) for s in SWEEP])
    kinds = set()
    for s, g in zip(SWEEP, got):
        p, t = assert_bank(s, entries, g)
        # the properties the host layer relies on
        chains, first = t["chains"], t["first"]
        assert all(c[3] > 0 for c in chains[first:]), "a body has units"
        for (entry, intro), body in zip(t["bodies"], chains[first:]):
            S_, D = t["seams"][entry], B.blocks_of(entries[entry])
            assert body[3] == D - S_ and body[5] == p["unit_base"][entry] + S_
            assert (intro < 0) == (S_ == 0)
            if intro >= 0:
                assert intro < first and chains[intro][3] == S_ and chains[intro][5] == p["unit_base"][entry], "the intro ends where the body begins"
                assert chains[intro][0] + 28 * S_ == body[0] and chains[intro][2] == entries[entry]["samples"]
            kinds.add((S_ == 0, S_ == D - 1, s["no_dummy"]))
        units = sum(c[3] for c in chains)
        assert units == sum(r[3] for r in p["rows"]), "every data block belongs to exactly one chain"
        spans = sorted((c[5], c[5] + c[3]) for c in chains if c[3])
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert len(kinds) >= 6


def test_the_corpus_banks_and_a_bank_without_any_loop(driver):
    ents, _ = K.bank()
    plain = B.placed([B.entry(100, 22050), B.entry(0, 11025, -1, True), B.entry(57, 44100, 1, False)])
    got = driver([bank_lines(s, ents) for s in K.MIXED_SETTINGS] + [bank_lines(K.MIXED_SETTINGS[0], plain)])
    for s, g in zip(K.MIXED_SETTINGS, got):
        assert_bank(s, ents, g)
    p, t = assert_bank(K.MIXED_SETTINGS[0], plain, got[-1])
    assert t["body"] == 0 and t["first"] == 3 and t["seams"] == [-1, -1, -1]


def test_the_largest_entries_keep_their_arithmetic_in_range(driver):
    """the most samples an entry may have, the loop point far inside: the body's sample offset and limit in 64 / 32 bits"""
    e = B.entry(MAX_SAMPLES, 44100, 10 ** 6, True, pcm_offset=5)
    s = B.settings(B.SPU, 16, True, 16)
    g = driver([bank_lines(s, [e], n=3)])[0]
    p, t = assert_bank(s, [e] * 3, g)
    S_ = 10 ** 6 * 44100 // 28000
    assert t["seams"] == [S_] * 3 and g["c"][3] == (5 + 28 * S_, 1, MAX_SAMPLES - 28 * S_, -(-MAX_SAMPLES // 28) - S_, 1, S_)
