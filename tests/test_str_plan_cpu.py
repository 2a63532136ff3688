"""The STR muxer's plan module (psxavenc_amd/csrc/str_plan.cpp) on the CPU, without HIP and under the host sanitizers, the way
tests/test_strspu_layout_cpu.py checks the layouts: g++ builds str_plan.cpp and the driver (tests/cpu/str_plan_check.cpp, which brings
the error sink) and nothing else; the driver prints what the module derives, and the expectations are the restatements' -- format 8's
schedule, audio chunks and video chunk header (tests/strspu_ref.py), the reference's sector loop over the oracle
(tests/str_reference_loop.py), and the refusals of tests/test_strspu_plan.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import str_reference_loop
import strspu_ref as R
from test_host_framing import _stream_structure
from test_strspu_plan import FPS, RATES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
VIDEO, AUDIO, EMPTY = 0, 1, 2
REFERENCE, COMPLETE = 0, 1
# the seven parameter sets of test_host_framing.test_str_plan_follows_the_reference_sector_loop: fmt, channels, bits, freq, speed, fps, trailing
REF_CASES = [(7, 2, 4, 37800, 2, (15, 1), False), (7, 2, 4, 37800, 2, (15, 1), True), (6, 1, 4, 37800, 2, (15, 1), False),
             (6, 2, 8, 18900, 1, (10, 1), False), (9, 0, 4, 37800, 2, (15, 1), False), (7, 2, 4, 37800, 2, (30000, 1001), False),
             (6, 1, 8, 37800, 2, (25, 1), True)]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build psxavenc_amd/csrc/str_plan.cpp and tests/cpu/str_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("str_plan") / "str_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe,
                    os.path.join(ROOT, "psxavenc_amd/csrc/str_plan.cpp"), os.path.join(ROOT, "tests/cpu/str_plan_check.cpp")], check=True)
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


def parse_plan(line):
    """(case parameters, rc, error text or None, plan numbers, budgets, rows (n, 4))"""
    head, rest = line.split(" : ", 1)
    parts = rest.split("|")
    rc = int(parts[0])
    if rc:
        return ints(head), rc, "|".join(parts[1:]).strip(), None, None, None
    return ints(head), rc, None, ints(parts[1]), np.array(ints(parts[2]), np.int32), np.array(ints(parts[3]), np.int32).reshape(-1, 4)


def check_counts(numbers, rows, ctx):
    """what every plan says about itself: the counts are the rows', Plan::n_audio counts the audio sectors that hold samples (the
    public n_audio_sectors counts the empty slots too), and those are numbered in stream order"""
    n_sectors, n_video, n_slots, n_audio = numbers[0], numbers[1], numbers[2], numbers[8]
    kinds = rows[:, 0]
    assert rows.shape[0] == n_sectors and int((kinds == VIDEO).sum()) == n_video, ctx
    assert int((kinds == AUDIO).sum()) == n_audio and int((kinds != VIDEO).sum()) == n_slots, ctx
    assert rows[kinds == AUDIO][:, 2].tolist() == list(range(n_audio)), ctx
    assert (rows[kinds == EMPTY][:, 1:] == [-1, -1, 0]).all(), ctx


def test_format_8_plans_against_the_restatement(lines):
    seen = set()
    for line in lines["plan8"]:
        (freq, ch, speed, fnum, fden, trailing, n_frames), rc, _, numbers, budgets, rows = parse_plan(line)
        assert rc == 0, line
        B, L, spc, p, q = R.layout(ch, freq, speed)
        want_rows, want_budgets, K = R.schedule(ch, freq, speed, fnum, fden, bool(trailing), n_frames)
        assert np.array_equal(rows, want_rows) and np.array_equal(budgets, want_budgets), line[:80]
        check_counts(numbers, rows, line[:80])
        base, den = R.budget_terms(ch, freq, speed, fnum, fden)
        assert numbers == [want_rows.shape[0], want_rows.shape[0] - K, K, 2048, q // p if q % p == 0 else 0, spc,
                           int(want_budgets.max()) if n_frames else 0, n_frames, K, 28 * R.units_per_channel(K, ch, 0x0001), base, den], line[:80]
        seen.add(((freq, ch, speed), (fnum, fden), trailing, n_frames))
    assert seen == {(r, f, t, n) for r in RATES for f in FPS for t in (0, 1) for n in range(6)}


def test_reference_tail_plans_follow_the_reference_sector_loop(lines, oracle):
    w, h = 16, 16                              # the structure does not depend on the picture
    frames_of = {n: oracle.synth_frames(w, h, n, seed=3, amp=2) for n in (1, 2, 3, 4, 7, 24)}
    seen = {}
    for line in lines["planref"]:
        (fmt, ch, bits, freq, speed, fnum, fden, trailing, n_frames, n_audio), rc, _, numbers, budgets, rows = parse_plan(line)
        assert rc == 0, line
        pcm = np.zeros(n_audio * max(1, ch), np.int16)
        pcm[:] = (np.arange(pcm.size) * 37 % 2001 - 1000)
        want, _, frames_encoded = str_reference_loop.encode_file_str(fmt, 0, w, h, fnum, fden, speed, frames_of[n_frames], pcm, channels=ch, freq=freq,
                                                                     bits=bits, trailing_audio=bool(trailing))
        ctx = line[:80]
        assert rows.shape[0] == want.shape[0] and numbers[7] == frames_encoded == budgets.size, ctx
        assert np.array_equal(rows, _stream_structure(want, fmt)), ctx
        check_counts(numbers, rows, ctx)
        sps = 18 * (112 * 8 // bits) // ch if ch else 0           # a sector's 18 sound groups hold 112 bytes of codes each
        assert numbers[3:6] == [{6: 2336, 7: 2352, 9: 2336}[fmt], (2 if ch == 2 else 4) * (37800 // freq) * (8 // bits) * speed if ch else 1, sps], ctx
        assert numbers[9] == min(n_audio, numbers[8] * sps), ctx      # every audio sector but the last is full
        seen.setdefault((fmt, ch, bits, freq, speed, (fnum, fden), bool(trailing)), set()).add((n_frames, n_audio))
    assert sorted(seen) == sorted(REF_CASES)
    for (fmt, ch, bits, freq, speed, fps, trailing), got in seen.items():
        sps = 18 * (112 * 8 // bits) // ch if ch else 0
        lengths = [10 ** 6, 0, 1, sps - 1, sps, sps + 1, 2 * sps, 3 * sps + 77, 7 * sps] if ch else [0]
        assert got == {(n, a) for n in (1, 2, 3, 4, 7, 24) for a in lengths}


def test_no_frame_plans_no_video_sector(lines):
    """n_frames = 0 (the reference asserts in its decoder there -- nothing to mirror) never plans frame 0: the stream ends at its first
    video slot.  The COMPLETE tail has nothing to write then; the reference's loop has handed out the audio slot a block of leading
    audio starts with -- at the end of input, so with EOF, and empty when there is no sample"""
    seen = set()
    for line in lines["zero"]:
        (fmt, ch, trailing, tail, pcm), rc, _, numbers, budgets, rows = parse_plan(line)
        assert rc == 0 and numbers[7] == 0 and numbers[1] == 0 and budgets.size == 0 and not (rows[:, 0] == VIDEO).any(), line
        check_counts(numbers, rows, line)
        leading_slot = tail == REFERENCE and ch and not trailing
        assert rows.tolist() == ([[AUDIO, -1, 0, 1] if pcm else [EMPTY, -1, -1, 0]] if leading_slot else []), line
        seen.add((fmt, ch, trailing, tail, pcm))
    assert seen == {(f, c, t, tail, pcm) for (f, c, t) in ((9, 0, 0), (7, 2, 0), (7, 2, 1), (7, 1, 1)) for tail in (REFERENCE, COMPLETE)
                    for pcm in (0, 1000, 5000, 1 << 40)}


def test_every_refusal_with_its_text(lines):
    """the settings of test_strspu_plan.test_every_refusal in its order, what it accepts next to them, and base or den past an int --
    which every format refuses before the sector loop works with them"""
    LOOP, NODUMMY = R.LOOP, R.NO_LEADING_DUMMY

    def s8(freq, ch, speed, fps=(15, 1), tail=COMPLETE, options=0x0001, video_id=0x8001):
        return [8, fps[0], fps[1], speed, ch, freq, 4, tail, options, video_id]

    def terms(fmt, ch, freq, speed, fps):
        if fmt == 8:
            return R.budget_terms(ch, freq, speed, fps[0], fps[1])
        interleave = 4 * speed if ch else 1          # 37800 Hz 4-bit stereo: every fourth sector at 1x
        return 75 * speed * (interleave - 1 if ch else 1) * fps[1], interleave * fps[0]

    def overflow(fmt, ch, freq, speed, fps):
        base, den = terms(fmt, ch, freq, speed, fps)
        assert base > 2 ** 31 - 1 or den > 2 ** 31 - 1
        return "psxhip_str: frame rate and audio rate do not fit the budget arithmetic (base %d, den %d)" % (base, den)

    bad = "psxhip_str: bad settings"
    no_sector = "psxhip_str: a frame would get no sector (frame rate too high for this CD speed)"
    want = [
        (s8(44100, 2, 2, tail=REFERENCE), "psxhip_str: format 8 (STRSPU) defines PSXHIP_STR_TAIL_COMPLETE only: the reference has no strspu loop whose "
                                          "tail could be mirrored"),
        (s8(200000, 2, 1), "psxhip_str: audio rate too high for this CD speed"),
        (s8(132300, 2, 1), "psxhip_str: audio rate too high for this CD speed"),
        (s8(44100, 2, 2, options=0x0001 | 1 << 18), "psxhip_str: unknown bit set in strspu_options"),
        (s8(44100, 2, 2, options=0x0001 | 1 << 24), "psxhip_str: unknown bit set in strspu_options"),
        (s8(44100, 2, 2, options=0x0001 | 1 << 31), "psxhip_str: unknown bit set in strspu_options"),
        (s8(44100, 2, 2, options=0x8001), "psxhip_str: the audio chunk id of strspu_options equals str_video_id"),
        (s8(44100, 2, 2, options=0x0042, video_id=0x0042), "psxhip_str: the audio chunk id of strspu_options equals str_video_id"),
        (s8(44100, 3, 2), bad),
        (s8(0, 2, 2), bad),
        (s8(-44100, 2, 2), bad),
        (s8(32000, 2, 2, fps=(2000000, 1)), overflow(8, 2, 32000, 2, (2000000, 1))),
        (s8(44100, 2, 2, fps=(151, 1)), no_sector),
        (s8(100000, 2, 1), None),
        (s8(44100, 2, 2, options=0xFFFF | LOOP | NODUMMY), None),
        (s8(32000, 2, 2, fps=(1, 2000000)), overflow(8, 2, 32000, 2, (1, 2000000))),
        ([7, 1, 1 << 30, 2, 2, 37800, 4, REFERENCE, 1, 0x8001], overflow(7, 2, 37800, 2, (1, 1 << 30))),
        ([7, 2 ** 31 - 1, 1, 2, 2, 37800, 4, COMPLETE, 1, 0x8001], overflow(7, 2, 37800, 2, (2 ** 31 - 1, 1))),
        ([9, 1, 2 ** 31 - 1, 2, 0, 37800, 4, COMPLETE, 1, 0x8001], overflow(9, 0, 37800, 2, (1, 2 ** 31 - 1))),
        ([9, 2 ** 31 - 1, (2 ** 31 - 1) // 150, 2, 0, 37800, 4, COMPLETE, 1, 0x8001], no_sector),        # base and den both just fit
    ]
    assert len(lines["settings"]) == len(want)
    for line, (params, text) in zip(lines["settings"], want):
        got, rc, error, numbers, _, _ = parse_plan(line)
        assert got == params, line
        if text is None:
            assert rc == 0, line
        else:
            assert rc == EINVAL and error == text, line
    assert parse_plan(lines["settings"][13])[3][4] == 0          # 100000 Hz at 1x: 1000 / 1323 of the sectors, no whole interleave
    assert terms(9, 0, 37800, 2, (2 ** 31 - 1, (2 ** 31 - 1) // 150))[0] > 2 ** 31 - 1 - 150


def recurrence(seed, n):
    """x <- (1103515245 x + 12345) mod 2^31 from x = seed; byte i = bits 16-23 of the i-th x after the seed"""
    out, x = np.zeros(n, np.uint8), seed
    for i in range(n):
        x = (1103515245 * x + 12345) & 0x7FFFFFFF
        out[i] = (x >> 16) & 0xFF
    return out


def test_strspu_place_host_builds_the_audio_chunks(lines):
    seen = set()
    for line in lines["place"]:
        head, text = line.split(" : ")
        ch, K, options = ints(head)
        U = R.units_per_channel(K, ch, options)
        E = recurrence(1 + ch + 10 * K, ch * U * 16).reshape(ch, U, 16)
        want = R.audio_sectors(E, K, ch, 44100, options)
        assert np.array_equal(np.frombuffer(bytes.fromhex(text), np.uint8).reshape(K, 2048), want), head
        seen.add((ch, K, options & ~0xFFFF))
    assert seen == {(c, k, f) for c in (1, 2) for k in (1, 2, 3) for f in (0, R.LOOP, R.NO_LEADING_DUMMY, R.LOOP | R.NO_LEADING_DUMMY)}


def test_video_chunk_header_is_the_restatements(lines):
    seen = set()
    for line in lines["vhdr"]:
        head, text = line.split(" : ")
        video_id, w, h, frame, chunk, budget, bytes_used = ints(head)
        row = np.zeros(budget, np.uint8)
        row[:8] = recurrence(7, 8)
        want = R.video_sector(row, (0, bytes_used), frame, chunk, budget, w, h, video_id)[:32]
        assert np.array_equal(np.frombuffer(bytes.fromhex(text), np.uint8), want), head
        seen.add((chunk, budget // 2016))
    assert seen == {(0, 3), (2, 3)}          # a frame's first and last chunk
