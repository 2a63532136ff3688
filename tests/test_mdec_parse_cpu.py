"""The decoder's parse core (psxavenc_amd/csrc/mdec_parse.h) on the CPU, under the host sanitizers, against the oracle's reader
(oracle/mdec_decode.c: orc_mdec_decode_frame): status, levels, quant scale, version and bits consumed on clean streams, status on a
seeded corrupted corpus.  The kernel runs the same text; it sees the corpus only after this has passed (tests/test_gpu_mdec_decode.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mdec_decode_corpus as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpu/decode_sim.cpp")
    d = tmp_path_factory.mktemp("decode_sim")
    exe = str(d / "decode_sim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe,
                    os.path.join(ROOT, "tests/cpu/decode_sim.cpp")], check=True)

    def run(cases, want_levels, windowed=False):
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        with open(src, "wb") as f:
            for c in cases:
                f.write(np.array([c.w, c.h, c.size, c.wrap, int(want_levels)], np.int32).tobytes())
                f.write(c.data[:c.size].tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, src, dst] + (["windowed"] if windowed else []), capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0 and not r.stderr.strip(), "the sanitizer build reported:\n" + r.stderr[-4000:]
        raw = open(dst, "rb").read()
        out, at = [], 0
        for c in cases:
            head = np.frombuffer(raw, np.int32, 4, at)
            at += 16
            levels = None
            if want_levels and head[0] == 0:
                levels = np.frombuffer(raw, np.int16, c.nblk * 64, at).reshape(c.nblk, 64)
                at += c.nblk * 128
            out.append((int(head[0]), levels, int(head[1]), int(head[2]), int(head[3])))
        assert at == len(raw)
        return out
    return run


def test_clean_streams_decode_as_the_oracle_says(oracle, sim):
    cases = [c for c, _ in DC.clean_cases()]
    got = sim(cases, True)
    versions = set()
    for c, g in zip(cases, got):
        rc, levels, q, v, nbits = DC.oracle_decode(c)
        assert rc == 0, c.name
        assert g[0] == 0 and (g[2], g[3], g[4]) == (q, v, nbits), (c.name, g[0], g[2:], (q, v, nbits))
        assert np.array_equal(g[1], levels), c.name
        versions.add((v, c.wrap))
    assert versions == {(2, 0), (3, 0), (3, 1)}


def test_corrupted_corpus_gives_the_oracles_status(oracle, sim):
    cases = list(DC.corrupted_cases())
    want = [DC.oracle_decode(c) for c in cases]
    DC.check_corpus_reaches_every_error(cases, [w[0] for w in want])
    got = sim(cases, True)
    bad = [(c.name, g[0], w[0]) for c, g, w in zip(cases, got, want) if g[0] != w[0]]
    assert not bad, bad[:20]
    for c, g, w in zip(cases, got, want):
        if w[0] == 0:                                    # a corrupted stream that still parses: everything else agrees too
            assert (g[2], g[3], g[4]) == (w[2], w[3], w[4]) and np.array_equal(g[1], w[1]), c.name
        elif w[0] <= -2:                                 # past the magic the header fields are set
            assert (g[2], g[3]) == (w[2], w[3]), c.name


def test_truncation_runs_at_every_byte(oracle):
    """the corpus cuts a 16x16 frame of every codec at every byte from 0 to its length"""
    cases = DC.corrupted_cases()
    for codec in (0, 1, 2):
        cuts = sorted(c.size for c in cases if c.name.startswith("c%d 16x16 cut at" % codec))
        assert cuts and cuts == list(range(len(cuts))) and len(cuts) > 40


def test_the_kernels_window_schedule_gives_the_same_answers(oracle, sim):
    """decode_sim's `windowed` mode is the parse kernel's loop with the 64 lanes as arrays: window fetch, per-offset classification,
    the walk, the per-lane block.  Same results as the step-by-step reader, on the clean streams and on the corrupted corpus."""
    for cases in ([c for c, _ in DC.clean_cases()][::3], list(DC.corrupted_cases())):
        a, b = sim(cases, True), sim(cases, True, windowed=True)
        for c, x, y in zip(cases, a, b):
            assert x[0] == y[0] and x[2:] == y[2:], (c.name, x[0], y[0])
            assert (x[1] is None) == (y[1] is None) and (x[1] is None or np.array_equal(x[1], y[1])), c.name
