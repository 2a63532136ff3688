"""The audio front-end's plan module (psxavenc_amd/csrc/resample_plan.cpp) on the CPU, without HIP and under the host sanitizers, the
way tests/test_adpcm_plan_cpu.py checks the ADPCM layer's: g++ builds resample_plan.cpp and the driver
(tests/cpu/resample_plan_check.cpp, which brings the error sink) and nothing else.  The expectations are restatements in Python over
the constants the driver prints.

tests/golden/resample_plan_parent.json holds what the library answered before the plan module existed, for CALLS: everything
psxhip_resampler_create decides precedes its device check, and psxhip_resampler_design and _output_count need no device, so all of it
was recorded through ctypes on a machine without one (an accepted create answers "no device"; a table is held as its SHA-256 with P
and T; the host convert's refusal of a NULL handle leaves the error text alone, so only its return code is held):

    [[k, a, answer] for (k, a), answer in zip(CALLS, library_answers(L, CALLS))], the counts of count_calls() gathered a rate pair a row

The plan module and the library as it is built now both have to reproduce the file exactly: the tables of the g++ build, of the
hipcc-built library and of the recording are the same bytes.
"""
import ctypes as C
import hashlib
import json
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE = -1, -2
GPU_TEST_RATES = [(48000, 37800), (44100, 37800), (48000, 18900), (22050, 37800), (32000, 44100), (44100, 44100), (44100, 44099), (192000, 18900)]   # tests/test_gpu_resampler.py
RATES = GPU_TEST_RATES + [(44100, 18900), (37800, 37800), (1000, 16000), (16000, 1000), (384000, 24000)]
BAD_RATES = [(1000, 16001), (16001, 1000), (999, 37800), (37800, 384001), (384001, 384001), (0, 0)]
BIG = 1 << 40


def params(src, dst):
    """design_params restated: L, M, P, T, H, bypass (the cutoff in the double arithmetic of the C text)"""
    g = math.gcd(src, dst)
    L, M = dst // g, src // g
    if src == dst:
        return L, M, 1, 0, 0, True
    factor = min(0.97 * dst / src, 1.0)
    T = math.ceil(32 / factor)
    T += T & 1
    return L, M, min(L, 1024), T, T // 2, False


def avail(src, dst, n):
    L, M, _, _, H, bypass = params(src, dst)
    return n if bypass else 0 if n <= H else -(-(n - H) * L // M)


def total(src, dst, n):
    L, M, _, _, _, bypass = params(src, dst)
    return n if bypass else -(-n * L // M)


def outputs_of(src, dst, consumed, n_in, flush):
    return (total if flush else avail)(src, dst, consumed + n_in) - avail(src, dst, consumed)


def count_calls(src, dst):
    H = params(src, dst)[4]
    points = sorted({0, 1, max(H - 1, 0), H, H + 1, 2 * H + 3, BIG, BIG + 1})
    return [("count", [src, dst, c, n, f]) for c in points for n in points for f in (0, 1)]


def create(**kw):
    d = dict(fmt=0, sch=2, srate=48000, dch=2, drate=37800, have_mix=0)
    assert set(kw) - {"mix"} <= set(d)
    return ("create", [dict(d, **kw)[n] for n in d] + list(kw.get("mix", ())))


CALLS = [("design", [s, d, 1, -1]) for s, d in RATES + BAD_RATES]
CALLS += [("design", [48000, 37800, 0, 0]), ("design", [48000, 37800, 1, 100]), ("design", [44100, 44100, 1, -1])]
CALLS += [c for s, d in RATES for c in count_calls(s, d)]
CALLS += [("count", [s, d, 0, 100, 0]) for s, d in BAD_RATES] + [("count", [48000, 37800, -1, 5, 0]), ("count", [48000, 37800, 5, -1, 1]),
                                                                 ("count", [48000, 37800, (1 << 62) - 5, 6, 0]), ("count", [48000, 37800, (1 << 62) - 6, 5, 0])]
CALLS += [
    create(fmt=-1), create(fmt=6), create(sch=0), create(sch=9), create(dch=0), create(dch=9), create(srate=999), create(drate=384001), create(srate=16001, drate=1000),
    create(fmt=6, sch=9), create(sch=3), create(sch=2, dch=6), create(sch=8, dch=1), create(sch=3, dch=2, have_mix=1, mix=[32767, 32767, 2, 0, 0, 0]),
    create(sch=3, dch=2, have_mix=1, mix=[1, 2, 3, -32768, -32767, -1]), create(sch=9, have_mix=1, mix=[0] * 18), create(sch=3, srate=999),
    create(), create(fmt=5), create(sch=1, dch=1), create(sch=2, dch=1), create(sch=1, dch=2), create(sch=6, dch=2), create(sch=8, dch=8), create(srate=44100, drate=44100),
    create(sch=3, dch=2, have_mix=1, mix=[12000, -7000, 9000, -3000, 15000, 11000]), create(sch=3, dch=2, have_mix=1, mix=[32767, 32767, 1, -32768, -32767, 0]),
    create(srate=1000, drate=16000), create(srate=16000, drate=1000), create(srate=44100, drate=44099),
]
CALLS += [("convdev", [0, 0, 0, 1, -1, 16, 1, 0, 0]), ("convdev", [0, 0, 0, 0, -1, 0, 0, 0, 1]), ("convhost", [0, 0, 0, 1, -1, 16, 1, 64, 0])]


# ------------------------------------------------------------------------------------------------ the library, through ctypes
def bind(L):
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.psxhip_last_error.restype = C.c_char_p
    L.psxhip_resampler_design.argtypes = [i32, i32, vp, vp, vp, i32]
    L.psxhip_resampler_output_count.argtypes = [i32, i32, i64, i64, i32]
    L.psxhip_resampler_output_count.restype = i64
    L.psxhip_resampler_create.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp]
    L.psxhip_resampler_convert_device.argtypes = [vp, vp, i64, vp, vp, i32, vp]
    L.psxhip_resampler_convert_host.argtypes = [vp, vp, i64, vp, i64, vp, i32]
    return L


def library_answers(L, calls):
    out = []
    for kind, a in calls:
        if kind == "design":
            P, T = C.c_int(-1), C.c_int(-1)
            room = 1024 * 600
            coef = (C.c_int16 * room)()
            rc = L.psxhip_resampler_design(a[0], a[1], C.addressof(P), C.addressof(T), C.addressof(coef) if a[2] else None, room if a[3] < 0 else a[3])
            if rc < 0:
                out.append(dict(rc=rc, error=L.psxhip_last_error().decode()))
            else:
                table = bytes(coef)[:P.value * T.value * 2] if a[2] and a[3] < 0 else b""
                out.append(dict(rc=rc, P=P.value, T=T.value, n=len(table), sha256=hashlib.sha256(table).hexdigest()))
        elif kind == "count":
            out.append(dict(value=L.psxhip_resampler_output_count(*a)))
        elif kind == "create":
            handle = C.c_void_p()
            mix = (C.c_int16 * max(len(a) - 6, 1))(*a[6:])
            rc = L.psxhip_resampler_create(C.addressof(handle), 0, *a[:5], C.addressof(mix) if a[5] else None)
            assert not handle.value
            out.append(dict(rc=rc, error=L.psxhip_last_error().decode()))
        else:
            assert not a[0]
            src = (C.c_void_p * 8)(*[0x100000] * 8)
            n_out = C.c_int64(-1)
            if kind == "convdev":
                rc = L.psxhip_resampler_convert_device(None, C.addressof(src) if a[3] else None, a[5], 0x100000 if a[6] else None, C.addressof(n_out), a[8], None)
                out.append(dict(rc=rc, error=L.psxhip_last_error().decode()))
            else:
                rc = L.psxhip_resampler_convert_host(None, C.addressof(src) if a[3] else None, a[5], 0x100000 if a[6] else None, a[7], C.addressof(n_out), a[8])
                out.append(dict(rc=rc))
            assert n_out.value == 0
    return out


@pytest.fixture(scope="module")
def gold():
    """the file as one answer per call of CALLS: "counts" holds a rate pair's count_calls() values on one row, "calls" [kind, args, answer]
    for every other call, in CALLS' order"""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "resample_plan_parent.json")))
    counts = {(s, d, *a[2:]): v for (s, d), values in g["counts"] for (_, a), v in zip(count_calls(s, d), values)}
    assert [tuple(r) for r, _ in g["counts"]] == RATES and all(len(v) == len(count_calls(*r)) for r, v in g["counts"])
    rest = iter(g["calls"])
    out = []
    for kind, a in CALLS:
        if kind == "count" and tuple(a) in counts:
            out.append(dict(value=counts[tuple(a)]))
        else:
            k, args, answer = next(rest)
            assert (k, args) == (kind, list(a))
            out.append(answer)
    assert next(rest, None) is None
    return out


# ------------------------------------------------------------------------------------------------ the driver
def build_driver(tmp, flags):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build psxavenc_amd/csrc/resample_plan.cpp and tests/cpu/resample_plan_check.cpp")
    exe = os.path.join(tmp, "resample_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, "-o", exe, os.path.join(ROOT, "psxavenc_amd/csrc/resample_plan.cpp"),
                    os.path.join(ROOT, "tests/cpu/resample_plan_check.cpp")], check=True)
    return exe


def run_driver(exe, tmp, calls):
    """the driver's constants, (rc, text) per call, and the blob of tables"""
    src, blob = os.path.join(tmp, "calls.txt"), os.path.join(tmp, "tables.bin")
    with open(src, "w") as f:
        for kind, a in calls:
            f.write(" ".join(map(str, [kind, len(a)] + list(a))) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, blob], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), "the driver reported:\n" + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[0].startswith("const ") and len(lines) == len(calls) + 1
    out = []
    for (kind, _), line in zip(calls, lines[1:]):
        head, rest = line.split(" : ", 1)
        rc, text = rest.split(" |", 1)
        assert head == kind
        out.append((int(rc), text.strip()))
    return K([int(v) for v in lines[0].split()[1:]]), out, open(blob, "rb").read()


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("resample_plan"))
    exe = build_driver(tmp, SANITIZE)
    return lambda calls: run_driver(exe, tmp, calls)


class K:
    """the constants, as the driver prints them"""

    def __init__(self, v):
        self.header, self.tile, self.launch_max, self.filter_size, self.max_phases = v


def ints(text):
    return [int(v) for v in text.split()]


def lists(text):
    return [ints(part) for part in text.split("|")]


def plan_answer(call, rc, text, blob):
    """the driver's answer in the recording's terms"""
    kind = call[0]
    if kind == "design":
        if rc:
            return dict(rc=rc, error=text)
        ret, P, T, at, n = ints(text)
        return dict(rc=ret, P=P, T=T, n=n, sha256=hashlib.sha256(blob[at:at + n]).hexdigest())
    if kind == "count":
        return dict(value=int(text))
    if kind == "create":
        return dict(rc=rc, error=text) if rc else dict(rc=EDEVICE, error="no HIP device visible (libpsxav_hip has no CPU fallback)")
    return dict(rc=rc, error=text) if kind == "convdev" else dict(rc=rc)


# ------------------------------------------------------------------------------------------------ against the recording
def test_the_plan_answers_as_the_parent_library_did(driver, gold):
    """refusals with their texts, P and T, the tables bit for bit (g++ designed them here, hipcc's build the recording), the counts"""
    _, got, blob = driver(CALLS)
    for call, (rc, text), want in zip(CALLS, got, gold):
        assert plan_answer(call, rc, text, blob) == want, (call, rc, text[:200], want)
    tables = [g["sha256"] for g in gold if g.get("n", 0) > 0]
    ratios = {params(s, d)[:2] for s, d in RATES if s != d}          # (a table is its ratio's: 16000 -> 1000 and 384000 -> 24000 share one)
    assert len(tables) == sum(1 for s, d in RATES if s != d) and len(set(tables)) == len(ratios)
    assert len({g["error"] for g in gold if g.get("rc") == EINVAL and "error" in g}) >= 6


def test_the_library_answers_as_its_parent_did(gold):
    """the built library through ctypes, unsanitized: the same table, its tables included.  Beside a GPU the creates that went on to
    the device are left out"""
    import torch
    from psxavenc_amd import _lib
    L = bind(C.CDLL(_lib.lib()._name))
    pairs = [(c, g) for c, g in zip(CALLS, gold) if g.get("rc") != EDEVICE or not torch.cuda.is_available()]
    got = library_answers(L, [c for c, _ in pairs])
    for (call, want), answer in zip(pairs, got):
        assert answer == want, (call, answer, want)


def test_counts_are_the_restatement_s(driver):
    """avail, total and outputs_of in exact integers, around H, at 0 and near 2^40"""
    calls = [c for s, d in RATES for c in count_calls(s, d)]
    _, got, _ = driver(calls)
    for (_, (s, d, consumed, n_in, flush)), (rc, text) in zip(calls, got):
        assert rc == 0 and int(text) == outputs_of(s, d, consumed, n_in, flush), (s, d, consumed, n_in, flush)
    _, got, _ = driver([("design", [s, d, 0, 0]) for s, d in RATES])
    for (s, d), (rc, text) in zip(RATES, got):
        assert rc == 0 and ints(text)[:3] == [params(s, d)[2]] + list(params(s, d)[2:4]), (s, d, text)


def test_default_matrices_and_row_sums(driver):
    cases = [(1, 1), (2, 2), (8, 8), (2, 1), (1, 2), (6, 2)]
    _, got, _ = driver([create(sch=s, dch=d) for s, d in cases])
    want = {(2, 1): {(0, 0): 8192, (0, 1): 8192}, (1, 2): {(0, 0): 16384, (1, 0): 16384},
            (6, 2): {(0, 0): 6786, (0, 2): 4799, (0, 4): 4799, (1, 1): 6786, (1, 2): 4799, (1, 5): 4799}}
    for (s, d), (rc, text) in zip(cases, got):
        m = lists(text.replace("device", ""))[1]
        cells = want.get((s, d), {(c, c): 16384 for c in range(d)})
        assert rc == 0 and m == [cells.get((c, k), 0) for c in range(8) for k in range(8)], (s, d)
    # a row of sum |m| = 65535 is the last one taken
    _, got, _ = driver([create(sch=3, dch=1, have_mix=1, mix=[32767, -32768, 0]), create(sch=3, dch=1, have_mix=1, mix=[32767, -32768, 1])])
    assert got[0][0] == 0 and got[1] == (EINVAL, "psxhip_resampler_create: matrix row 0 has sum |m| = 65536 > 65535")


# ------------------------------------------------------------------------------------------------ the launch's shape
def test_span_table_placement_lds_bytes_and_grid(driver):
    """afe_layout.h's carve and the rules on top of it, from the printed constants: dch 1, 2, 8; a full-size and a 64 KiB compute unit
    (the 1024-phase tables are above 48 KiB and stay in memory on both; the smaller one also sends 192000 -> 18900's 42 KiB table back there)"""
    cases = [(s, d, dch, lds, 256) for s, d in RATES for dch in (1, 2, 8) for lds in (163840, 65536)] + [(48000, 37800, 2, 163840, n) for n in (1, 304)]
    k, got, _ = driver([("shape", list(c)) for c in cases])
    assert (k.header, k.tile) == (320, 256)
    seen = set()
    for (s, d, dch, lds_max, n_cu), (rc, text) in zip(cases, got):
        L, M, P, T, H, bypass = params(s, d)
        if bypass:
            assert rc == 0 and lists(text) == [[0, 0, 0, 8 * n_cu], [L, M, P, T, H, 1]]
            continue
        span = (L - 1 + (k.tile - 1) * M) // L + T
        span += span & 1
        spans = dch * 2 * span * 2
        table = P * T * 2
        coef_lds = int(table <= 48 * 1024 and k.header + table + spans <= lds_max)
        lds = k.header + coef_lds * table + spans
        if lds > lds_max:
            assert (rc, text) == (EINVAL, "psxhip_resampler_create: the input span (%d bytes of LDS) does not fit a compute unit" % lds), (s, d, dch, lds_max)
            seen.add("refused")
            continue
        assert rc == 0 and lists(text) == [[span, coef_lds, lds, n_cu * max(1, min(8, lds_max // lds))], [L, M, P, T, H, 0]], (s, d, dch, lds_max, text)
        seen.add((coef_lds, table <= 48 * 1024, P))
    assert {(0, False, 1024), (1, True, 63)} <= seen and any(c == 0 and fits for c, fits, _ in seen - {"refused"}), seen


# ------------------------------------------------------------------------------------------------ the launch cut
def test_a_call_is_cut_into_launches(driver):
    """per-launch outputs sum to outputs_of; i0 and r0 are divmod(avail(consumed) * M, L); only the last launch flushes"""
    N = 1 << 28
    cases = [(s, d, consumed, n_in, flush, grid) for s, d in ((48000, 37800), (44100, 44099), (16000, 1000), (1000, 16000), (44100, 44100)) for consumed in (0, 1234567)
             for n_in in (0, 1, N, N + 1, 3 * N + 5) for flush in (0, 1) for grid in (2048,)] + [(48000, 37800, 0, 1000, 0, 2), (48000, 37800, 0, 100000, 1, 64)]
    k, got, _ = driver([("cut", list(c)) for c in cases])
    assert k.launch_max == N
    counts = set()
    for (s, d, consumed, n_in, flush, grid_max), (rc, text) in zip(cases, got):
        L, M, P, T, H, bypass = params(s, d)
        (outputs, avail0), *launches = lists(text)
        assert rc == 0 and outputs == outputs_of(s, d, consumed, n_in, flush) and avail0 == avail(s, d, consumed)
        assert len(launches) == max(1, -(-n_in // N)) and sum(l[0] for l in launches) == n_in and sum(l[4] for l in launches) == outputs
        at = consumed
        for i, (n, fl, i0, r0, n_out, work, grid) in enumerate(launches):
            last = i == len(launches) - 1
            assert n == (N if not last else n_in - N * i) and fl == int(bool(flush) and last)
            assert n_out == outputs_of(s, d, at, n, fl)
            q, r = (0, 0) if bypass else divmod(avail(s, d, at) * M, L)
            assert (i0, r0) == ((0, 0) if bypass else (q - at, r)) and i0 >= -H
            assert work == -(-n_out // k.tile) + (0 if bypass else 1) and grid == min(work, grid_max)
            at += n
        counts.add(len(launches))
    assert counts == {1, 2, 4}
