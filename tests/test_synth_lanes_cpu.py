"""The synthetic-input kernel file's own text (psxavenc_amd/csrc/synth_kernels.hip) on the CPU, lane by lane, under the host
sanitizers (tests/cpu/synth_lanes.cpp behind the stand-in tests/cpu/hip_lanes/hip/hip_runtime.h), against the statements the GPU
tests use (oracle_lib.synth_frames, oracle_lib.synth_pcm: oracle/synth.c) byte for byte: the index arithmetic of the two generators
-- which frame and dword a lane writes, which sample, and where the last workgroup stops -- over heap blocks of exactly the bytes a
call owns.  Two small geometries and two seeds of frames with a padded frame stride, every kind of PCM at pitch 1 and 2 from sample 0
and from one past 2^32; every lane order -- ascending, descending, shuffled -- must give the same bytes."""
import numpy as np
import pytest

import lanes_cpu as L

FILL = 0x3C
# (width, height, frames, spare bytes between frames): 96 and 576 dwords a frame, so 288 lanes (a second workgroup of 32) and 1152
GEOMETRIES = [(16, 16, 3, 4), (48, 32, 2, 0)]
SEEDS = [(1, 0, 4), (0x9E3779B9, 4093, 37)]                 # (seed, first frame, noise amplitude)
PCM = [(seed, chain, first, n, kind, pitch) for seed, chain in ((5, 0), (0xDEADBEEF, 23)) for kind in range(6)
       for first, n, pitch in ((0, 300, 1), (2 ** 32 + 32768 - 100, 257, 2))]


def _write(path):
    with open(path, "wb") as f:
        for w, h, n, spare in GEOMETRIES:
            for seed, first, amp in SEEDS:
                f.write(np.array([0, w, h, seed, first, n, amp, w * h * 3 // 2 + spare, FILL], np.uint32).tobytes())
        for seed, chain, first, n, kind, pitch in PCM:
            f.write(np.array([1, seed, chain, first & 0xFFFFFFFF, first >> 32, n, kind, pitch, FILL], np.uint32).tobytes())


def test_frames_and_pcm_are_the_statements(oracle, tmp_path):
    exe = L.build(tmp_path, "synth_lanes", L.SANITIZE)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write(src)
    raw, at = np.frombuffer(L.run_orders(exe, src, dst), np.uint8), 0
    for w, h, n, spare in GEOMETRIES:
        fb = w * h * 3 // 2
        for seed, first, amp in SEEDS:
            want = np.full((n, fb + spare), FILL, np.uint8)
            want[:, :fb] = oracle.synth_frames(w, h, n, seed=seed, amp=amp, first=first)
            want = want.reshape(-1)[:(n - 1) * (fb + spare) + fb]
            assert np.array_equal(raw[at:at + want.size], want), (w, h, seed, first, amp)
            at += want.size
    for seed, chain, first, n, kind, pitch in PCM:
        want = np.full((n - 1) * pitch + 1, FILL | (FILL << 8), np.uint16).view(np.int16)
        want[::pitch] = oracle.synth_pcm(seed, chain, first, n, kind)
        got = raw[at:at + 2 * want.size].view(np.int16)
        assert np.array_equal(got, want), (seed, chain, first, n, kind, pitch)
        at += 2 * want.size
    assert at == raw.size
