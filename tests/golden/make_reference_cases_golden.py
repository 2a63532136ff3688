#!/usr/bin/env python3
"""Generate tests/golden/reference_cases.npz: the reference's recorded answers, so that the suite runs where oracle/_ref is absent.

For the randomised cases of tests/test_adpcm_oracle.py::test_against_live_reference_build and
tests/test_gpu_adpcm.py::test_against_reference_build_when_shipped: the SHA-256 and length of the output bytes and the final
encoder states of the REFERENCE's own libpsxav (oracle/_ref/libpsxav_ref.so, built unchanged by oracle/Makefile), and its size
helpers.  Inputs are regenerated at test time from oracle/synth.c with the same seeded draws.

Run where oracle/_ref has been built:  python tests/golden/make_reference_cases_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def stereo_pad(kind, n, seed, pad=4032):
    pcm = np.zeros((n + pad) * 2, np.int16)
    pcm[0:2 * n:2] = O.synth_pcm(seed, 0, 0, n, kind)
    pcm[1:2 * n:2] = O.synth_pcm(seed, 1, 0, n, kind)
    return pcm


def mono_pad(kind, n, seed, pad=4032):
    pcm = np.zeros(n + pad, np.int16)
    pcm[:n] = O.synth_pcm(seed, 0, 0, n, kind)
    return pcm


def reference_cases():
    """the draws of test_against_live_reference_build (rng seed 1) and test_against_reference_build_when_shipped (rng seed 7)"""
    R = O.ref()
    assert R is not None, "oracle/_ref/libpsxav_ref.so not built"
    g = {}
    rng = np.random.default_rng(1)
    for trial in range(40):
        kind = int(rng.integers(0, 6))
        n = int(rng.integers(1, 3000))
        pcm = O.synth_pcm(int(rng.integers(1, 1 << 30)), trial, int(rng.integers(0, 1 << 20)), n, kind)
        b, sb = O.ref_spu_encode(pcm)
        g["live_spu%d_sha" % trial] = sha(b)
        g["live_spu%d_state" % trial] = np.array([sb.prev1, sb.prev2], np.int32)
    for trial in range(24):
        s = O.XaSettings(trial & 1, (trial >> 1) & 1, 37800 if trial & 4 else 18900, 8 if trial & 8 else 4, trial, trial * 3)
        n = int(rng.integers(1, 9000))
        kind = int(rng.integers(0, 6))
        pcm = stereo_pad(kind, n, trial) if s.stereo else mono_pad(kind, n, trial)
        b, _ = O.ref_xa_encode(s, pcm, n, lba=trial * 1000)
        g["live_xa%d_sha" % trial] = sha(b)
        g["live_xa%d_len" % trial] = np.array([b.size], np.int64)
    sizes = []
    for trial in range(16):
        s = O.XaSettings(trial & 1, (trial >> 1) & 1, 37800 if trial & 4 else 18900, 8 if trial & 8 else 4, 0, 0)
        rs = O.ref_settings(s)
        sizes.append([R.psx_audio_xa_get_samples_per_sector(rs), R.psx_audio_xa_get_buffer_size_per_sector(rs),
                      R.psx_audio_xa_get_sector_interleave(rs)])
    g["live_xa_size_helpers"] = np.array(sizes, np.int64)
    rng = np.random.default_rng(7)
    for trial in range(10):
        n = int(rng.integers(30, 4000))
        kind = int(rng.integers(0, 6))
        pcm = O.synth_pcm(int(rng.integers(1, 1 << 30)), trial, 0, n, kind)
        b, _ = O.ref_spu_encode(pcm)
        g["shipped_spu%d_sha" % trial] = sha(b)
    return g


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "reference_cases.npz"), **reference_cases())
