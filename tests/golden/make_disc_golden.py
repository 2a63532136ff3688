"""Regenerates tests/golden/disc_ref.npz: a dozen sectors of the three source sizes and their finished image as the statement
(tests/disc_ref.py, "psxhip disc finish v1") gives it.  Run from the repository root: python tests/golden/make_disc_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import disc_ref as R  # noqa: E402


def main():
    rng = np.random.default_rng(20261018)
    xa = rng.integers(0, 256, (3, 2336)).astype(np.uint8)             # XA sound sectors: form 2, real time, audio
    xa[:, 0:4] = [0, 0, 0x64, 0x01]
    xa[:, 4:8] = xa[:, 0:4]
    strcd = rng.integers(0, 256, (3, 2352)).astype(np.uint8)          # STRCD video sectors: form 1, real time, data
    strcd[:, 0x10:0x14] = [1, 1, 0x48, 0]
    strcd[:, 0x14:0x18] = strcd[:, 0x10:0x14]
    strv = rng.integers(0, 256, (3, 2048)).astype(np.uint8)           # STRV: no subheader of its own
    slot_source, start_lba = [0, 1, 2, -1], 4496                      # the BCD second and minute carry inside the run
    srcs = [R.Source(xa, 2336, file=1, channel=2), R.Source(strcd, 2352), R.Source(strv, 2048, data_subheader=(1, 0, 0x48, 0))]
    image = R.finish(slot_source, start_lba, srcs)
    assert image.shape == (12, 2352) and not R.check(image, start_lba)[0].any()
    np.savez_compressed(os.path.join(HERE, "disc_ref.npz"), xa=xa, strcd=strcd, strv=strv, slot_source=np.array(slot_source, np.int32),
                        start_lba=np.int32(start_lba), image=image)


if __name__ == "__main__":
    main()
