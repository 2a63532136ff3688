#!/usr/bin/env python3
"""Generate tests/golden/strspu_ref.npz: the audio lanes of two small format 8 streams ("psxhip STRSPU v1") --
every channel's SPU blocks, produced by the REFERENCE's own psx_audio_spu_encode (oracle/_ref/libpsxav_ref.so, libpsxav/adpcm.c
compiled unchanged) over the channel's samples fitted to 28 U.  It pins the audio of the format where oracle/_ref is absent.

Inputs are regenerated at test time from the recorded parameters (oracle/synth.c is a pure function).  Run where the reference
build exists:
    python tests/golden/make_strspu_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402
import strspu_ref as R  # noqa: E402

# channels, K audio sectors, options, PCM samples per channel (short of the fit: silence behind them; long: cut), synth seed and kind
CASES = [
    dict(channels=2, K=2, options=0x0001, samples=28 * 125 - 9, seed=811, kind=0),
    dict(channels=1, K=1, options=0x0042 | R.NO_LEADING_DUMMY | R.LOOP, samples=28 * 126 + 50, seed=812, kind=2),
]


def case_pcm(case):
    ch, n = case["channels"], case["samples"]
    pcm = np.zeros(n * ch, np.int16)
    for c in range(ch):
        pcm[c::ch] = O.synth_pcm(case["seed"], c, 0, n, case["kind"])
    return pcm


def main():
    assert O.ref() is not None, "needs oracle/_ref/libpsxav_ref.so (make -C oracle where the reference lies)"
    out = {"n_cases": np.int32(len(CASES))}
    for i, case in enumerate(CASES):
        U = R.units_per_channel(case["K"], case["channels"], case["options"])
        fitted = R.fit_pcm(case_pcm(case), case["channels"], U)
        blocks = np.stack([O.ref_spu_encode(fitted[c])[0].reshape(-1, 16) for c in range(case["channels"])])
        assert blocks.shape == (case["channels"], U, 16)
        out["params_%d" % i] = np.array([case[k] for k in ("channels", "K", "options", "samples", "seed", "kind")], np.int64)
        out["blocks_%d" % i] = blocks
    path = os.path.join(HERE, "strspu_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
