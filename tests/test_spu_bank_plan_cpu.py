"""The sound bank's plan module (psxavenc_amd/csrc/spu_bank_plan.cpp) on the CPU, without HIP and under the host sanitizers, the way
tests/test_reader_plan_cpu.py checks the readers': g++ builds spu_bank_plan.cpp and the driver (tests/cpu/spu_bank_plan_check.cpp,
which brings the error sink) and nothing else.  The driver is handed this file's banks and prints what the plan derives; the
expectations are the restatement of tests/spu_bank_corpus.py, and, through ctypes, what the library's psxhip_spu_bank_plan and
psxhip_spu_file_size answer.  Every case is arithmetic only: sample counts may be huge."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import spu_bank_corpus as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
MAX_SAMPLES = 0x7FFFFFFF - 28
NO_THRESHOLD = 0x7FFFFFFF


def bank_lines(s, entries, n=None, threshold=NO_THRESHOLD, has_settings=1, has_entries=1):
    n = len(entries) if n is None else n
    lines = ["%d %d %d %d %d %d %d %d %d %d" % (has_settings, s["fmt"], s["alignment"], int(s["no_dummy"]), s["bank_alignment"], s["beam"],
                                                 has_entries, n, threshold, len(entries))]
    for e in entries:
        lines.append("%d %d %d %d %d %s" % (e["pcm_offset"], e["samples"], e["freq"], e["loop"], int(e["enable_loop"]),
                                            e["name"].encode()[:16].ljust(16, b"\0").hex()))
    return lines


def run_driver(exe, tmp, banks):
    """per bank: (rc, error text) or (0, head numbers, entry lines, tile lines), and the public function's (rc, total)"""
    src = os.path.join(tmp, "banks.txt")
    with open(src, "w") as f:
        for lines in banks:
            f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), "the sanitizer build reported (exit %d):\n%s" % (r.returncode, r.stderr[-4000:])
    out, cur = [], None
    for line in r.stdout.splitlines():
        kind = line.split(" ", 1)[0]
        if kind == "e":
            cur["entries"].append(line.split()[1:])
        elif kind == "t":
            cur["tiles"].append(tuple(int(v) for v in line.split()[1:]))
        elif kind == "p":
            cur["public"] = tuple(int(v) for v in line.split()[1:])
            out.append(cur)
        else:
            rc, rest = line.split(" | ", 1)
            cur = dict(rc=int(rc), entries=[], tiles=[])
            if cur["rc"]:
                cur["error"] = rest
            else:
                cur["head"] = [int(v) for v in rest.split()]
    assert len(out) == len(banks)
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build psxavenc_amd/csrc/spu_bank_plan.cpp and tests/cpu/spu_bank_plan_check.cpp")
    tmp = str(tmp_path_factory.mktemp("spu_bank_plan"))
    exe = os.path.join(tmp, "spu_bank_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe,
                    os.path.join(ROOT, "psxavenc_amd/csrc/spu_bank_plan.cpp"), os.path.join(ROOT, "tests/cpu/spu_bank_plan_check.cpp")], check=True)
    return lambda banks: run_driver(exe, tmp, banks)


def sweep_entries():
    """samples 0, 1, 27, 28, 29, 56, 1125 with loops on and off, each with and without a loop point"""
    out = []
    for samples, enable_loop, loop in itertools.product((0, 1, 27, 28, 29, 56, 1125), (False, True), (-1, 0, 30)):
        out.append(B.entry(samples, 22050, loop, enable_loop, "n%d" % samples))
    return B.placed(out)


SWEEP = [B.settings(fmt, alignment, no_dummy, bank_alignment) for fmt, no_dummy, alignment, bank_alignment in
         itertools.product((B.SPU, B.VAG), (False, True), (16, 64, 2048), (16, 2048))]


def vag_header(s, e, p, i):
    r = p["rows"][i]
    h = np.zeros(48, np.uint8)
    if s["fmt"] != B.VAG:
        return h
    h[0:4] = list(b"VAGp")
    h[4:8] = [0, 0, 0, 0x20]
    h[12:16] = list(((r[2] + r[3] + r[4]) * 16).to_bytes(4, "big"))
    h[16:20] = list(e["freq"].to_bytes(4, "big"))
    h[0x1E] = 1
    name = e["name"].encode()[:16]
    h[0x20:0x20 + len(name)] = list(name)
    return h


def test_the_plan_is_the_restated_rule_over_the_sweep(driver):
    entries = sweep_entries()
    got = driver([bank_lines(s, entries) for s in SWEEP])
    for s, g in zip(SWEEP, got):
        p = B.plan(s, entries)
        assert g["rc"] == 0 and g["public"] == (0, p["total"]), (s, g.get("error"))
        total, chunked, max_units, total_units, pcm_elements, n_tiles = g["head"]
        assert (total, chunked, max_units, total_units, pcm_elements) == (p["total"], 0, 41, sum(r[3] for r in p["rows"]), B.pcm_elements(entries))
        assert g["tiles"] == p["tiles"] and n_tiles == len(p["tiles"])
        assert total % s["bank_alignment"] == 0
        for i, (e, line) in enumerate(zip(entries, g["entries"])):
            offset, size = int(line[0]), int(line[1])
            row, header, chain, base = tuple(int(v) for v in line[2:10]), bytes.fromhex(line[10]), [int(v) for v in line[11:16]], int(line[16])
            assert (offset, size) == (p["offsets"][i], p["sizes"][i]) and offset % s["bank_alignment"] == 0, (s, i)
            assert i == 0 or offset >= p["offsets"][i - 1] + p["sizes"][i - 1] > offset - s["bank_alignment"], "monotone, and no further than it must be"
            assert row == p["rows"][i], (s, i, row, p["rows"][i])
            assert header == vag_header(s, e, p, i).tobytes(), (s, i)
            # the chain reads the entry's samples and writes from the first data block on: behind the header and the dummy block
            assert chain == [e["pcm_offset"], 1, e["samples"], B.blocks_of(e), 1]
            assert base == p["unit_base"][i] == (offset + (48 if s["fmt"] == B.VAG else 0)) // 16 + int(not s["no_dummy"])


def _library():
    from psxavenc_amd import spubank, spufile
    L = spubank._bind()
    spufile._bind()
    return L, spubank, spufile


def test_the_library_plans_without_a_device_and_sizes_are_the_one_file_sizes():
    L, spubank, spufile = _library()
    entries = sweep_entries()
    for s in SWEEP:
        p = B.plan(s, entries)
        offsets, sizes, total = spubank.plan(spubank.settings(s["fmt"], s["alignment"], s["no_dummy"], s["bank_alignment"]),
                                             [spubank.entry(e["pcm_offset"], e["samples"], e["freq"], e["loop"], e["enable_loop"], e["name"]) for e in entries])
        assert offsets.tolist() == p["offsets"] and sizes.tolist() == p["sizes"] and total == p["total"]
        for e, size in zip(entries, sizes):
            one = spufile.settings(s["fmt"], 1, e["freq"], alignment=s["alignment"], loop_point=e["loop"], enable_loop=e["enable_loop"],
                                   no_dummy=s["no_dummy"], name=e["name"])
            assert L.psxhip_spu_file_size(C.byref(one), e["samples"]) == size
        assert np.all(np.diff(offsets) >= 0) and np.all(offsets % s["bank_alignment"] == 0)


OK = B.settings(B.VAG, 64, False, 16)
ONE = [B.entry(100, 22050)]
# (what, the bank's lines, the text's beginning): in the order the plan decides them
REFUSALS = [
    ("n = 0", bank_lines(OK, [], n=0), "psxhip_spu_bank: 0 entries (1 .. 65535)"),
    ("n = 65536", bank_lines(OK, ONE, n=65536), "psxhip_spu_bank: 65536 entries (1 .. 65535)"),
    ("no settings", bank_lines(OK, ONE, has_settings=0), "psxhip_spu_bank: NULL settings or entries"),
    ("no entries", bank_lines(OK, ONE, has_entries=0), "psxhip_spu_bank: NULL settings or entries"),
    ("format 4", bank_lines(dict(OK, fmt=4), ONE), "psxhip_spu_bank: format 4 (2 = SPU, 3 = VAG"),
    ("format 0", bank_lines(dict(OK, fmt=0), ONE), "psxhip_spu_bank: format 0 "),
    ("alignment 24", bank_lines(dict(OK, alignment=24), ONE), "psxhip_spu_bank: alignment 24 is no positive multiple of 16"),
    ("alignment 0", bank_lines(dict(OK, alignment=0), ONE), "psxhip_spu_bank: alignment 0 is no positive multiple of 16"),
    ("bank alignment 8", bank_lines(dict(OK, bank_alignment=8), ONE), "psxhip_spu_bank: bank_alignment 8 (a multiple of 16, 16 .. 65536)"),
    ("bank alignment 40", bank_lines(dict(OK, bank_alignment=40), ONE), "psxhip_spu_bank: bank_alignment 40 "),
    ("bank alignment 131072", bank_lines(dict(OK, bank_alignment=131072), ONE), "psxhip_spu_bank: bank_alignment 131072 "),
    ("beam 5", bank_lines(dict(OK, beam=5), ONE), "psxhip_spu_bank: beam 5 (0 .. 4)"),
    ("beam -1", bank_lines(dict(OK, beam=-1), ONE), "psxhip_spu_bank: beam -1 (0 .. 4)"),
    ("samples -1", bank_lines(OK, ONE + [B.entry(-1, 22050)]), "psxhip_spu_bank: entry 1 has -1 samples (0 .. 2147483619)"),
    ("samples too many", bank_lines(OK, [B.entry(MAX_SAMPLES + 1, 22050)]), "psxhip_spu_bank: entry 0 has 2147483620 samples"),
    ("frequency 0", bank_lines(OK, ONE + ONE + [B.entry(5, 0)]), "psxhip_spu_bank: entry 2 has audio_frequency 0"),
    ("negative offset", bank_lines(OK, [B.entry(5, 22050, pcm_offset=-2)]), "psxhip_spu_bank: entry 0 has pcm_offset -2"),
    ("2^31 records", bank_lines(OK, [B.entry(MAX_SAMPLES, 22050)], n=28), "psxhip_spu_bank: the bank takes "),
    # precedence: the count before the format, the format before the alignments, those before the beam, the settings before the
    # entries, an entry's samples before its frequency, the entries before the bank's size
    ("n before the pointers", bank_lines(OK, ONE, n=-1, has_settings=0), "psxhip_spu_bank: -1 entries"),
    ("n before format", bank_lines(dict(OK, fmt=9, alignment=3), ONE, n=0), "psxhip_spu_bank: 0 entries"),
    ("format before alignment", bank_lines(dict(OK, fmt=9, alignment=3), ONE), "psxhip_spu_bank: format 9"),
    ("alignment before bank alignment", bank_lines(dict(OK, alignment=3, bank_alignment=3, beam=9), ONE), "psxhip_spu_bank: alignment 3"),
    ("bank alignment before beam", bank_lines(dict(OK, bank_alignment=3, beam=9), ONE), "psxhip_spu_bank: bank_alignment 3"),
    ("beam before entries", bank_lines(dict(OK, beam=9), [B.entry(-1, 0)]), "psxhip_spu_bank: beam 9"),
    ("samples before frequency", bank_lines(OK, [B.entry(-1, 0)]), "psxhip_spu_bank: entry 0 has -1 samples"),
    ("entries before the size", bank_lines(OK, [B.entry(MAX_SAMPLES, 22050)] * 27 + [B.entry(5, -1)], n=28), "psxhip_spu_bank: entry 27 has audio_frequency -1"),
]


def test_every_refusal_has_its_text_and_its_place(driver):
    got = driver([lines for _, lines, _ in REFUSALS])
    for (what, _, text), g in zip(REFUSALS, got):
        assert g["rc"] == EINVAL and g["public"][0] == EINVAL, what
        assert g["error"].startswith(text), (what, g["error"])
    assert len({g["error"] for g in got[:18]}) == 17, "the refusals have texts of their own"


def test_the_largest_bank_the_indices_allow_is_planned(driver):
    """27 entries of the most samples: just below 2^31 records; with the 28th the bank is refused (REFUSALS)"""
    g = driver([bank_lines(B.settings(B.SPU, 16, True, 16), [B.entry(MAX_SAMPLES, 44100, 10 ** 6, True)], n=27)])[0]
    assert g["rc"] == 0
    blocks = -(-MAX_SAMPLES // 28)
    assert g["head"][0] == 27 * blocks * 16 and g["head"][0] // 16 < 2 ** 31
    assert int(g["entries"][26][2]) == 26 * blocks and int(g["entries"][26][7]) == 27 * blocks
    assert int(g["entries"][0][8]) == 10 ** 6 * 44100 // 28000, "the loop block in 64-bit arithmetic"


def test_serial_or_chunked_on_both_sides_of_the_threshold(driver):
    """the decision is the longest entry's units against the threshold given: 512 for up to 8 entries, 4096 above (the library's rule,
    asked by the caller: psxhip_adpcm_chunked_threshold)"""
    from psxavenc_amd import _lib
    L = _lib.lib()
    assert (L.psxhip_adpcm_chunked_threshold(8), L.psxhip_adpcm_chunked_threshold(9)) == (512, 4096)
    s = B.settings(B.SPU, 64, False, 16)
    cases = []
    for n, units in ((3, 511), (3, 512), (8, 512), (9, 512), (12, 4095), (12, 4096)):
        entries = B.placed([B.entry(28 * units - 27, 22050)] + [B.entry(100, 22050)] * (n - 1))
        cases.append((n, units, bank_lines(s, entries, threshold=L.psxhip_adpcm_chunked_threshold(n))))
    got = driver([c[2] for c in cases])
    assert [(n, units, g["head"][1], g["head"][2]) for (n, units, _), g in zip(cases, got)] == [
        (3, 511, 0, 511), (3, 512, 1, 512), (8, 512, 1, 512), (9, 512, 0, 512), (12, 4095, 0, 4095), (12, 4096, 1, 4096)]
