"""Regenerates tests/golden/disc_read_ref.npz: a dozen sectors of a finished image, most of them damaged, and what the statement
(tests/disc_read_ref.py, "psxhip disc read v1") says of them.  Run from the repository root:
python tests/golden/make_disc_read_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import disc_read_corpus as K  # noqa: E402
import disc_read_ref as D  # noqa: E402
import disc_ref as R  # noqa: E402


def main():
    rng = np.random.default_rng(20261019)
    video = K.sectors(rng, 5, 2336, forms=[1] * 5, kind=0x08)           # form 1, data
    audio = K.sectors(rng, 4, 2336, forms=[2] * 4, kind=0x04)           # form 2, audio
    image = R.finish([0, 1, -1], 4496, [R.Source(video, 2336, file=1, channel=0), R.Source(audio, 2336, file=1, channel=1)], 0, 12)
    assert not R.check(image, 4496)[0].any()
    image[0] = K.flip(image[0], [0x400], rng)                           # one byte
    image[3] = K.burst(image[3], 87, 0x123, rng)                        # the longest burst that is always repaired
    image[6] = K.scattered(image[6], 20, rng)
    image[9] = K.burst(image[9], 300, 0x200, rng)                       # unrepairable
    image[1] = K.flip(image[1], [0x700], rng)                           # form 2: EDC wrong, nothing repairs it
    image[4, 0x92C:] = 0                                                # form 2: EDC absent
    image[7] = K.flip(image[7], [0x11, 0x15], rng)                      # form 2: both channel bytes differ, in different ways
    image[5, 3] = 0x7F                                                  # sync
    tracks = [D.Track(2048, 3, 1, 0, 0x08, 0x08, 2048), D.Track(2336, 8, 1, -1, 0x04, 0x04, 2340), D.Track(2352, 2, -1, -1, 0, 0, 2352)]
    res = D.read(image, tracks)
    st = res.table[:, 2]
    assert ((st & D.REPAIRED) != 0).sum() == 3 and ((st & D.UNREPAIRABLE) != 0).sum() == 1 and (st & D.DROPPED).any() and (st & D.EMPTY).any()
    np.savez_compressed(os.path.join(HERE, "disc_read_ref.npz"), image=image,
                        tracks=np.array([[T.size, T.capacity, T.file, T.channel, T.mask, T.value, T.stride] for T in tracks], np.int32),
                        sectors=res.sectors, table=res.table, counts=res.counts,
                        summary=np.array([res.summary[k] for k in D.SUMMARY_FIELDS], np.int64),
                        **{"track%d" % t: b for t, b in enumerate(res.tracks)})


if __name__ == "__main__":
    main()
