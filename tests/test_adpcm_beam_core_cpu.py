"""psxavenc_amd/csrc/adpcm_beam_core.h -- the text the beam kernels compile -- behind tests/cpu/adpcm_beam_sim.cpp, a program of its
own built with g++ -fsanitize=address,undefined, against the statement (tests/adpcm_beam_ref.py) on every unit of the corpus
(tests/adpcm_beam_corpus.py): records, errors and states, all three codings, beam 1 .. 4."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adpcm_beam_corpus as BC
import lanes_cpu as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpu/adpcm_beam_sim.cpp")
    d = tmp_path_factory.mktemp("adpcm_beam_sim")
    exe = str(d / "adpcm_beam_sim")
    subprocess.run(["g++", "-std=c++17"] + L.SANITIZE + ["-o", exe, os.path.join(ROOT, "tests/cpu/adpcm_beam_sim.cpp")], check=True)
    return d, exe


@pytest.mark.parametrize("filter_count,bits", BC.CODINGS)
def test_core_equals_the_statement(sim, filter_count, bits):
    d, exe = sim
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    want = b""
    with open(src, "wb") as f:
        for beam in BC.BEAMS:
            rec, err, after, _, _ = BC.expected(filter_count, bits, beam)
            for c in range(BC.N_CHAINS):
                n = BC.unit_count(c)
                f.write(np.array([bits, filter_count, beam, n, *BC.start_state(c)], np.int32).tobytes())
                f.write(BC.samples(c)[:28 * n].tobytes())
                for u in range(n):
                    want += rec[c, u].tobytes() + err[c, u].tobytes() + after[c, u].tobytes()
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, env=L.sanitizer_env(), timeout=600)
    assert p.returncode == 0 and not p.stderr.strip(), p.stderr[-4000:]
    with open(dst, "rb") as f:
        got = f.read()
    assert len(got) == len(want)
    if got != want:
        per = (16 if bits == 4 else 32) + 12
        first = next(i for i in range(len(got)) if got[i] != want[i])
        raise AssertionError("unit %d of the run differs from the statement at byte %d of its output" % (first // per, first % per))
