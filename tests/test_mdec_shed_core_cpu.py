"""The refinement's plain-C++ core (psxavenc_amd/csrc/mdec_shed_core.h) and its plan under the host sanitizers: g++ builds the stand-alone
program tests/cpu/mdec_shed_check.cpp with -fsanitize=address,undefined over the core and mdec_plan.cpp, the program reads the corpus's
coefficients and budgets from a file written here, and what it reports per frame -- step, count, the two sums, the result and a hash of
the row -- is held to the numpy statement (tests/mdec_shed_ref.py).  Nothing is loaded into python under a sanitizer.

The corpus (tests/mdec_shed_corpus.py) refines frames in magnitude class 1 only: its first fits in classes 2 and 3 are all declined.
So that the core's rows are also checked where the shed predicate is in class 2 or 3, six frames of random coefficients are added
here, with a scale and a budget chosen freely -- the rule does not ask that N be the plain encode's answer."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import mdec_shed_corpus as C
import mdec_shed_ref as S
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fnv1a64(data):
    h = 1469598103934665603
    for v in bytes(data):
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpu/mdec_shed_check.cpp")
    path = str(tmp_path_factory.mktemp("mdec_shed") / "mdec_shed_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", path,
                    os.path.join(ROOT, "psxavenc_amd/csrc/mdec_plan.cpp"), os.path.join(ROOT, "tests/cpu/mdec_shed_check.cpp")], check=True)
    return path


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), "the sanitizer build reported:\n" + r.stderr[-4000:]
    return r.stdout.splitlines()


def raster(Fz):
    """zig-zag-ordered coefficients back to raster order, as the program reads them"""
    out = np.zeros_like(Fz)
    out[:, S.ZAGZIG] = Fz
    return out.astype(np.int16)


def synthetic():
    """[(codec, Fz, budget, N)]: twelve blocks of coefficients so large that only the escape carries them, whatever the run, a few of which are exactly 1, 2 or 3 quantiser steps at scale 1;
    N = 2, and a budget that the stream meets only when all of class 2 (class 3) has gone.  Shedding so few levels costs less than the
    coarser scale does on all the others, so the frame is refined"""
    rng = np.random.default_rng(20261020)
    out = []
    for codec in (0, 1, 2):
        for cls in (2, 3):
            lv = rng.integers(41, 200, (12, 64)) * rng.choice(np.array([-1, 1]), (12, 64))
            for m in (1, 2, 3):
                lv[rng.integers(0, 12, 8), rng.integers(1, 64, 8)] = m * rng.choice(np.array([-1, 1]), 8)
            Fz = lv * S.QUANT_ZZ + rng.integers(-3, 4, (12, 64))
            Fz[:, 0] = rng.integers(-1000, 1001, 12)
            bits = S.refine(codec, Fz, 1 << 20, 2, 3).bits
            b = S.frame_need(int(bits[63 * cls])) + (codec & 1)        # (an odd budget for v3)
            o = S.refine(codec, Fz, b, 2, 3)
            assert o.state == "refined" and S.step_class(o.step)[0] == cls, (codec, cls, o.state, o.first_fit)
            out.append((codec, Fz, b, 2))
    return out


def test_frames_equal_the_statement(exe, tmp_path):
    cases = []          # (codec, Fz, budget, N, K, the statement's outcome)
    for gi, g in enumerate(C.groups()):
        res = C.plain(gi)[1]
        for i in range(g.n):
            for K in C.KS:
                cases.append((g.codec, C.coefs(gi, i), int(g.budgets[i]), int(res[i, 0]), K, C.outcome(gi, i, K)))
    for codec, Fz, b, N in synthetic():
        cases.append((codec, Fz, b, N, 3, S.refine(codec, Fz, b, N, 3)))
    path = str(tmp_path / "frames.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for codec, Fz, b, N, K, _ in cases:
            f.write(struct.pack("<5i", codec, Fz.shape[0], b, N, K))
            f.write(raster(Fz).tobytes())
    lines = run(exe, "frames", path)
    assert len(lines) == len(cases)
    classes = set()
    for line, (codec, Fz, b, N, K, o) in zip(lines, cases):
        got = [int(v) for v in line.split()[1:]]
        assert tuple(got[:4]) == o.record(), (line, o.record())
        assert got[4] == (o.state == "refined")
        if o.state == "refined":
            assert got[5:9] == list(o.result) and got[9] == int(o.bits[o.step]) and got[10] == fnv1a64(o.row), (line, o.result)
            classes.add(S.step_class(o.step)[0])
        else:
            assert got[5:] == [0] * 6
    assert classes == {1, 2, 3}


def test_fdct_equals_the_oracle(exe, tmp_path):
    """on the corpus's blocks (against mdec_coefs) and on full-range random blocks (against the oracle's own 8x8 transform)"""
    rng = np.random.default_rng(5)
    blocks = [rng.integers(-128, 128, (512, 64)), np.full((1, 64), -128), np.full((1, 64), 127),
              np.where(np.indices((8, 8)).sum(0) % 2 == 0, -128, 127).reshape(1, 64)]
    want = []
    for gi, g in enumerate(C.groups()):
        if g.w > 48:
            continue
        nx, ny = g.w // 16, g.h // 16
        for i in range(g.n):
            y = g.frames[i][:g.w * g.h].reshape(g.h, g.w).astype(np.int64) - 128
            c = g.frames[i][g.w * g.h:].reshape(g.h // 2, g.w // 2, 2).astype(np.int64) - 128
            coefs = O.mdec_coefs(g.w, g.h, g.frames[i])
            for fy in range(ny):
                for fx in range(nx):
                    mb = [c[fy * 8:fy * 8 + 8, fx * 8:fx * 8 + 8, 0], c[fy * 8:fy * 8 + 8, fx * 8:fx * 8 + 8, 1]]
                    mb += [y[fy * 16 + 8 * r:fy * 16 + 8 * r + 8, fx * 16 + 8 * q:fx * 16 + 8 * q + 8] for r in (0, 1) for q in (0, 1)]
                    blocks.append(np.stack([m.reshape(64) for m in mb]))
                    want.append(coefs[:, fy * nx + fx])
    n_random = sum(b.shape[0] for b in blocks[:4])
    samples = np.concatenate(blocks).astype(np.int16)
    src, dst = str(tmp_path / "blocks.bin"), str(tmp_path / "coefs.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", samples.shape[0]))
        f.write(samples.tobytes())
    run(exe, "fdct", src, dst)
    got = np.fromfile(dst, np.int16).reshape(-1, 64)
    assert got.shape == samples.shape
    ref = samples[:n_random].copy()
    for blk in ref:
        O.lib().orc_fdct_islow8(O.ptr(blk, O.i16p))
    assert np.array_equal(got[:n_random], ref)
    assert np.array_equal(got[n_random:], np.concatenate(want))


def test_every_refusal_of_the_plan_and_the_workspace(exe):
    lines = run(exe, "plan")
    refusals = {l.split(" ", 3)[1]: (int(l.split(" ", 3)[2]), l.split(" ", 3)[3] if len(l.split(" ", 3)) > 3 else "") for l in lines if l.startswith("refuse ")}
    rule = {"null_frames": "NULL argument", "null_out": "NULL argument", "null_results": "NULL argument", "negative_frames": "NULL argument",
            "magnitude_0": "max_magnitude 0 outside [1, 3]", "magnitude_4": "max_magnitude 4 outside [1, 3]",
            "frame_stride_small": "4-byte aligned and frame_stride >= w*h*3/2", "frame_stride_misaligned": "4-byte aligned",
            "out_stride_misaligned": "4-byte aligned", "frames_misaligned": "4-byte aligned", "out_misaligned": "4-byte aligned",
            "budget_small": "frame_max_size 7 outside [8, 512]", "budget_above_context": "frame_max_size 513 outside [8, 512]",
            "budget_above_stride": "larger than out_stride", "too_many_frames": "more than 16 777 215 frames"}
    for name in ("sound", "sound_per_frame", "sound_no_frames"):
        assert refusals.pop(name) == (0, ""), name
    assert set(refusals) == set(rule)
    for name, (rc, text) in refusals.items():
        assert rc == -1 and text.startswith("refine_frames_device:") and rule[name] in text, (name, rc, text)
    assert "rows 13" in lines
    for l in lines:
        if l.startswith("ws "):
            nblk, acc, decision, zeroed, dc_level, dc_code, block_off, stride = (int(v) for v in l.split()[1:])
            assert acc == 0 and decision == 13 * 64 * 8 and zeroed == decision + 64 and dc_level == zeroed
            assert dc_code >= dc_level + 2 * nblk and dc_code % 16 == 0 and block_off == dc_code + 4 * nblk
            assert stride >= block_off + 4 * (nblk + 1) and stride % 16 == 0
    assert [l for l in lines if l.startswith("groups ")] == ["groups 1 1", "groups 16 1", "groups 17 2", "groups 300 19", "groups 4096 256"]
