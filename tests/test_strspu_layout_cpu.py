"""Format 8's arithmetic in the host layer (psxavenc_amd/csrc/host_layout.h: strspu_layout, strspu_audio_before) on the CPU, under the
host sanitizers, the way tests/test_host_layout_cpu.py checks the other layouts: the driver (tests/cpu/strspu_layout_check.cpp) prints
what the header derives, the expectations are the restatement's (tests/strspu_ref.py)."""
import os
import shutil
import subprocess

import pytest

import strspu_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = [1323, 1000000, 2147483646, 2147483647]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpu/strspu_layout_check.cpp")
    exe = str(tmp_path_factory.mktemp("strspu_layout") / "strspu_layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe,
                    os.path.join(ROOT, "tests/cpu/strspu_layout_check.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), "the sanitizer build reported:\n" + r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        out.setdefault(kind, []).append(rest)
    return out


def ints(text):
    return [int(v) for v in text.split()]


def test_layout_is_the_formats(lines):
    seen = {}
    for line in lines["layout"]:
        (freq, ch, speed), got = (ints(part) for part in line.split(":"))
        B, L, spc, p, q = R.layout(ch, freq, speed)
        assert got == [ch, B, L, spc, p, q], line
        assert B * ch == 126 and L * ch == 2016 and p * spc * 75 * speed == q * freq
        seen[(freq, ch, speed)] = (p, q)
    assert len(seen) == 12
    assert [seen[k] for k in ((44100, 2, 2), (44100, 1, 2), (44100, 2, 1), (32000, 2, 2), (48000, 2, 1), (11025, 1, 2))] == [
        (1, 6), (1, 12), (1, 3), (160, 1323), (160, 441), (1, 48)]
    assert seen[(200000, 2, 1)][0] > seen[(200000, 2, 1)][1] and seen[(2147483647, 2, 2)][0] > seen[(2147483647, 2, 2)][1]


def test_audio_before_is_the_schedule(lines):
    seen = set()
    for line in lines["before"]:
        (freq, ch, speed, trailing), got = (ints(part) for part in line.split(":"))
        p, q = R.layout(ch, freq, speed)[3:]
        at = list(range(61)) + FAR
        assert got == [R.audio_before(p, q, bool(trailing), n) for n in at], line
        # whole shares: the reference's modulo schedule, audio first or last in every block of N (filefmt.c:456-461)
        if p == 1:
            for n in range(60):
                audio = got[n + 1] > got[n]
                assert audio == ((n % q) == q - 1 if trailing else (n % q) == 0), (line, n)
        seen.add((freq, ch, speed, trailing))
    assert len(seen) == 20          # the two rates past their CD speed have no schedule
