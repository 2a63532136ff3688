"""The decoder's core (psxavenc_amd/csrc/adpcm_decode_core.h) on the CPU, under the host sanitizers, against the numpy statement
(tests/adpcm_decode_ref.py): the clean corpus, records of seeded random bytes that cover all 256 header values for both record sizes
(flags included), the fixed-point stream.  The same driver (tests/cpu/adpcm_decode_sim.cpp) runs the kernel's chunk / verify
schedule as a host model: its fixpoint equals the serial decode whatever the chunking.  The kernels compile the same text; they see
the corpus only after this has passed (tests/test_gpu_adpcm_decode.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adpcm_decode_corpus as DC
import adpcm_decode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Case:
    def __init__(self, name, records, bits, filter_count, state=(0, 0), chunk_units=0, warmup_units=0, limit=None):
        self.name, self.bits, self.filter_count, self.state = name, bits, filter_count, state
        self.records = np.ascontiguousarray(records, np.uint8).reshape(-1, R.record_bytes(bits))
        self.chunk_units, self.warmup_units = chunk_units, warmup_units
        self.limit = 28 * len(self.records) if limit is None else limit


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpu/adpcm_decode_sim.cpp")
    d = tmp_path_factory.mktemp("adpcm_decode_sim")
    exe = str(d / "adpcm_decode_sim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe,
                    os.path.join(ROOT, "tests/cpu/adpcm_decode_sim.cpp")], check=True)

    def run(cases):
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        with open(src, "wb") as f:
            for c in cases:
                f.write(np.array([c.bits, c.filter_count, len(c.records), c.state[0], c.state[1], c.chunk_units, c.warmup_units, c.limit],
                                 np.int32).tobytes())
                f.write(c.records.tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0 and not r.stderr.strip(), "the sanitizer build reported:\n" + r.stderr[-4000:]
        raw = open(dst, "rb").read()
        out, at = [], 0
        for c in cases:
            n = len(c.records)
            head = np.frombuffer(raw, np.int32, 3, at)
            at += 12
            pcm = np.frombuffer(raw, np.int16, 28 * n, at)
            at += 56 * n
            flags = np.frombuffer(raw, np.uint8, n, at)
            at += n
            out.append(((int(head[0]), int(head[1])), pcm, flags, int(head[2])))
        assert at == len(raw)
        return out
    return run


@pytest.fixture(scope="module")
def spu_blocks():
    return {name: DC.spu_encode_units(DC.signal(name, 28 * DC.SPU_UNITS), False)[0] for name in DC.signal_names()}


def check(case, got):
    pcm, st, flags = R.decode_chain(case.records, case.bits, case.filter_count, case.state)
    want = pcm.copy()
    want[case.limit:] = 0x7777
    assert got[0] == st, (case.name, got[0], st)
    assert np.array_equal(got[1], want), case.name
    assert np.array_equal(got[2], flags), case.name


def test_clean_corpus(sim, spu_blocks):
    cases = [Case(name, b, 4, 5) for name, b in spu_blocks.items()]
    for name in DC.signal_names()[::3]:
        for fmt, stereo, bits in DC.XA_LAYOUTS[:4]:
            sectors, _ = DC.xa_encode_sectors(DC.xa_pcm(name, stereo, bits, 1), fmt, stereo, bits, False, 1)
            rec = R.xa_sector_records(sectors[0], bits)
            for c in range(2 if stereo else 1):
                cases.append(Case("xa %s %d %d %d ch %d" % (name, fmt, stereo, bits, c), rec[c::2 if stereo else 1], bits, 4))
    for c, g in zip(cases, sim(cases)):
        check(c, g)


@pytest.mark.parametrize("bits,filter_count", [(4, 5), (4, 4), (8, 4)])
def test_random_bytes_cover_every_header(sim, bits, filter_count):
    rec = R.random_records(7 + bits, bits, 300)
    assert len(set(rec[:, 0].tolist())) == 256
    cases = [Case("random", rec, bits, filter_count, (-32768, 32767)), Case("random cut", rec[:9], bits, filter_count, (5, -5), limit=28 * 8 + 5)]
    got = sim(cases)
    for c, g in zip(cases, got):
        check(c, g)
    want_flags = set([0, 2] if filter_count == 4 else [0, 1, 2, 3])
    assert set(got[0][2].tolist()) == want_flags


def test_fixed_point_stream(sim):
    rec = R.fixed_point_stream(256)
    cases = [Case("fixed %d" % s, rec, 4, 5, (s, s)) for s in (0, 1000, -1000)]
    cases += [Case("fixed chunked %d" % s, rec, 4, 5, (s, s), chunk_units=4, warmup_units=8) for s in (1000, -1000)]
    got = sim(cases)
    for c, g in zip(cases, got):
        check(c, g)
    assert [g[0] for g in got] == [(0, 0), (8, 8), (-7, -7), (8, 8), (-7, -7)]
    assert (got[3][1][28 * 8:] == 8).all() and got[3][3] >= 2 and got[4][3] >= 2      # the wrong guess was met and repaired


@pytest.mark.parametrize("chunk_units", [1, 2, 5, 64])
def test_chunked_fixpoint_equals_the_serial_decode(sim, spu_blocks, chunk_units):
    cases = []
    for name, b in spu_blocks.items():
        for warm in (0, 1, 8):
            cases.append(Case("%s chunk %d warm %d" % (name, chunk_units, warm), b[:97], 4, 5, (123, -45), chunk_units, warm))
            cases.append(Case("%s chunk %d warm %d cut" % (name, chunk_units, warm), b[:97], 4, 5, (123, -45), chunk_units, warm, limit=28 * 50 + 5))
    got = sim(cases)
    for c, g in zip(cases, got):
        check(c, g)
    if chunk_units < 64:
        tonal = [g[3] for c, g in zip(cases, got) if c.name.startswith("kind4") and " warm 0" in c.name]
        assert tonal and min(tonal) >= 2, "no wrong guess was met: the verify phase is not exercised"
