"""The wavefront model of the stand-in (tests/cpu/hip_lanes/hip_lanes_waves.h) against plain numpy, and its reports against kernels
that are wrong on purpose.

tests/cpu/wave_probe.hip runs every cross-lane operation of psxavenc_amd/csrc/wave_ops.h and of the reader kernels -- the DPP scan
and reduction, ballots, mbcnt, readlane / readfirstlane, the four shuffles at their edges in 32 and 64 bits, a barrier-separated LDS
transpose across four wavefronts, every atomic -- on random and extreme lanes; tests/wave_probe_ref.py holds the answers.  The model
must give those bytes under ASan / UBSan in all three orders (of workgroups, of wavefronts between barriers, of lanes between
collectives).  tests/test_gpu_wave_probe.py asks the MI355X for the same bytes, so the model's reading of the hardware is pinned too.

tests/cpu/wave_wrong_lanes.cpp holds the wrong kernels; each must end in its own report.  CPU only."""
import subprocess

import numpy as np
import pytest

import lanes_cpu as L
import wave_probe_ref as R


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return tmp_path_factory.mktemp("wave_model")


@pytest.fixture(scope="module")
def wrong(folder):
    exe = L.build(folder, "wave_wrong_lanes", L.SANITIZE)

    def run(case, order=0, seed=L.SEED):
        p = subprocess.run([exe, case, str(order), str(seed)], capture_output=True, env=L.sanitizer_env(), timeout=300)
        return p.returncode, L.own_stderr(p.stderr.decode(errors="replace"), True), p.stdout
    return run


def test_probe_kernels_give_numpy_bytes_in_every_order(folder):
    exe = L.build(folder, "wave_probe_lanes", L.SANITIZE)
    inputs = R.make_input()
    src, dst = str(folder / "in.bin"), str(folder / "out.bin")
    with open(src, "wb") as f:
        f.write(R.to_bytes(*inputs))
    want = R.expected(*inputs)
    for name, order in L.ORDERS:
        got = L.run(exe, src, dst, order, fibers=True)
        assert got == want, "%s order: %s" % (name, R.describe(got, want, inputs[0], inputs[2], inputs[3]))


def test_the_reference_is_not_vacuous():
    """the answers hold what the issue asks for: rows of zeros, of INT_MIN / 64, a single non-zero lane in every position, shuffles
    whose edge lanes keep their own value, sparse masks"""
    x, y, masks, tiles, atom = R.make_input()
    assert any((row == 0).all() for row in x) and any((row == R.INT_MIN // 64).all() for row in x)
    assert {int(np.nonzero(row)[0][0]) for row in x if np.count_nonzero(row) == 1} == set(range(64))
    up, down = R.shfl_up(x, 3), R.shfl_down(x, 3)
    assert (up[:, :3] == x[:, :3]).all() and (up[:, 3:] == x[:, :-3]).all()
    assert (down[:, 61:] == x[:, 61:]).all() and (down[:, :61] == x[:, 3:]).all()
    assert any(R.popcount(m) == 1 for m, _ in masks) and any(int(m) == 0 for m, _ in masks)


@pytest.mark.parametrize("case,code,text", [
    ("barrier_in_branch", 72, r"wait at barriers of different call sites.*wave_wrong_lanes\.cpp:\d+"),
    ("barrier_and_collective", 71, r"waits partly at a barrier .*wave_wrong_lanes\.cpp:\d+.* and partly at a collective"),
    ("two_sites", 70, r"wait at collectives of different call sites.*wave_wrong_lanes\.cpp:\d+"),
    ("returned_lane", 73, r"__shfl by lane \d+ from lane 5, which has returned.*wave_wrong_lanes\.cpp:\d+"),
    ("missing_lane", 73, r"readlane by lane \d+ from lane 40.*wave_wrong_lanes\.cpp:\d+"),
])
def test_wrong_kernels_end_in_the_models_report(wrong, case, code, text):
    import re
    for _, order in L.ORDERS:
        rc, err, _ = wrong(case, order)
        assert rc == code and re.search(text, err), (case, order, rc, err[-2000:])
        assert len(err.strip().split("\n")) == 1, err


@pytest.mark.parametrize("case,text", [
    ("lds_past", r"wave_wrong_lanes\.cpp:\d+.*(runtime error: (store|load)|AddressSanitizer: global-buffer-overflow)"),
    ("global_past", r"AddressSanitizer: heap-buffer-overflow"),
])
def test_out_of_range_reads_end_in_a_sanitizer_report(wrong, case, text):
    import re
    for _, order in L.ORDERS:
        rc, err, _ = wrong(case, order)
        assert rc != 0 and rc not in range(70, 76) and re.search(text, err, re.S), (case, order, rc, err[-3000:])


def test_lds_is_made_anew_for_every_workgroup(wrong):
    """LDS nobody wrote holds other bytes in every order, for every seed and in every workgroup: a kernel that lets them reach its
    output cannot give equal bytes in the three orders"""
    outs = []
    for order, seed in ((0, 1), (1, 1), (2, 1), (0, 2)):
        rc, err, out = wrong("lds_unwritten", order, seed)
        assert rc == 0 and not err.strip(), err
        outs.append(out)
    assert len(set(outs)) == len(outs)
