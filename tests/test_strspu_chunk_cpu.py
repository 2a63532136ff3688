"""The STRSPU reader's header reading (psxavenc_amd/csrc/strspu_chunk.h: the classification, the chunk number, the MISMATCH rule) on the
CPU, under the host sanitizers, against the statement (tests/strspu_demux_ref.py): clean headers from the muxer's statement, and a
seeded corpus of random and of edited 32-byte headers that is required to reach every MISMATCH clause, alone, and both classifications.
The kernels compile the same text (tests/test_gpu_strspu_demux.py runs them)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import strspu_demux_cases as X
import strspu_demux_ref as R
import strspu_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpu/strspu_chunk_check.cpp")
    d = tmp_path_factory.mktemp("strspu_chunk")
    exe = str(d / "strspu_chunk_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe,
                    os.path.join(ROOT, "tests/cpu/strspu_chunk_check.cpp")], check=True)

    def run(cases):
        """cases: [(ch, id, d, loop, frequency, k, header bytes)] -> [(audio, flags, mismatch, number)]"""
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        with open(src, "wb") as f:
            for ch, audio_id, dd, loop, freq, k, hd in cases:
                f.write(np.array([ch, audio_id, dd, loop, freq], np.int32).tobytes() + np.array([k], np.int64).tobytes())
                f.write(np.asarray(hd, np.uint8)[:32].tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0 and not r.stderr.strip(), "the sanitizer build reported:\n" + r.stderr[-4000:]
        raw = open(dst, "rb").read()
        assert len(raw) == 20 * len(cases)
        out = []
        for i in range(len(cases)):
            a = np.frombuffer(raw, np.int32, 3, 20 * i)
            out.append((int(a[0]), int(a[1]), int(a[2]), int(np.frombuffer(raw, np.int64, 1, 20 * i + 12)[0])))
        return out
    return run


def _want(case):
    ch, audio_id, d, loop, freq, k, hd = case
    options = audio_id | (M.LOOP if loop else 0) | (0 if d else M.NO_LEADING_DUMMY)
    clauses = R.mismatch_clauses(hd, k, ch, freq, options) if ch else None
    return (int(R.is_audio(hd, ch, audio_id)), int(hd[0x1C]) | int(hd[0x1D]) << 8, clauses, R.chunk_number(hd))


def _compare(check, cases):
    got, want = check(cases), [_want(c) for c in cases]
    for c, g, w in zip(cases, got, want):
        assert (g[0], g[1], g[3]) == (w[0], w[1], w[3]), (c[:6], g, w)
        if w[2] is not None:
            assert g[2] == int(bool(w[2])), (c[:6], g, w)
    return want


def test_clean_headers_read_as_the_statement_says(check):
    cases = []
    for ch in (1, 2):
        for options in X.OPTION_SETS:
            for K in (1, 3):
                audio_id = 0x0001 + K
                sectors = M.audio_sectors(np.zeros((ch, K * 126 // ch, 16), np.uint8), K, ch, 32000 + K, audio_id | options)
                for k in range(K):
                    cases.append((ch, audio_id, 0 if options & M.NO_LEADING_DUMMY else 1, int(bool(options & M.LOOP)), 32000 + K, k, sectors[k, :32]))
    want = _compare(check, cases)
    assert all(w[0] == 1 and w[2] == [] and w[3] == c[5] for c, w in zip(cases, want))
    # the same headers under other settings: frequency 0 is not compared; another id is not audio; ch 0 has no audio
    c = cases[-1]
    got = check([c[:4] + (0,) + c[5:], c[:1] + (c[1] + 1,) + c[2:], (0,) + c[1:], c[:4] + (c[4] + 1,) + c[5:]])
    assert [g[0] for g in got] == [1, 0, 0, 1] and got[0][2] == 0 and got[3][2] == 1


def test_seeded_corpus_reaches_every_clause_and_both_classes(check):
    rng = np.random.default_rng(20)
    cases = []
    for i in range(600):                                 # random bytes, half of them with 60 01 and a likely id
        hd = rng.integers(0, 256, 32, dtype=np.uint8)
        if i & 1:
            hd[0:2] = (0x60, 0x01)
            X.poke(hd, 2, 2, int(rng.integers(1, 3)))
        if i % 8 == 3:                                   # the numbers at both ends: k = -1 and k = 2^32 - 2
            X.poke(hd, 8, 4, 0 if i & 8 else 0xFFFFFFFF)
        cases.append((int(rng.integers(0, 3)), int(rng.integers(1, 3)), int(rng.integers(0, 2)), int(rng.integers(0, 2)),
                      int(rng.choice([0, 44100])), int(rng.choice([0, 1, 5, 2 ** 24, 2 ** 32 - 2])), hd))
    fields = [(0x04, 2), (0x06, 2), (0x0C, 4), (0x10, 2), (0x12, 2), (0x14, 4), (0x18, 4), (0x1C, 2)]
    for i in range(1200):                                # clean headers with one field, or a few, replaced
        ch, K, options = int(rng.integers(1, 3)), 4, X.OPTION_SETS[int(rng.integers(0, 4))]
        k = int(rng.integers(0, K))
        hd = M.audio_sectors(np.zeros((ch, K * 126 // ch, 16), np.uint8), K, ch, 44100, 0x0001 | options)[k, :32].copy()
        for _ in range(1 if i % 3 else int(rng.integers(0, 4))):
            at, width = fields[int(rng.integers(0, len(fields)))]
            X.poke(hd, at, width, int(rng.integers(0, 1 << (8 * width))) if rng.integers(0, 2) else
                   int.from_bytes(bytes(hd[at:at + width].tolist()), "little") ^ (1 << int(rng.integers(0, 8 * width))))
        cases.append((ch, 0x0001, 0 if options & M.NO_LEADING_DUMMY else 1, int(bool(options & M.LOOP)), 44100, k, hd))
    want = _compare(check, cases)
    assert {w[0] for w in want} == {0, 1}
    alone = {w[2][0] for w in want if w[2] is not None and len(w[2]) == 1}
    assert alone == set(X.MISMATCH_EDITS), sorted(set(X.MISMATCH_EDITS) - alone)
    assert any(w[2] == [] for w in want) and any(w[2] is not None and len(w[2]) > 3 for w in want)
    assert {w[3] for w in want} >= {-1, 2 ** 32 - 2}
