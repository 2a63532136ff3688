"""The MIXED refinement bound the frame kernel proves "no scale <= p - 1 fits" with when a pass stops counting at its checkpoint.

csrc/mdec_search.h: a block's AC bits at any scale s <= s' are at least the sum of G = len - deficit over its codes at s'.  The
theorem holds block by block (a run never crosses a block), so for ANY split of a frame's macroblocks into a counted set (codes at
p - 1) and an uncounted set (codes at p, the ones the pass emits anyway)

    bits(s)  >=  fixed bits + sum over counted (AC bits - deficit at p - 1) + sum over uncounted (AC bits - deficit at p)

for every s <= p - 1.  The kernel's pass sums ARE that number (mdec_search_note_bound); here it is held against the true bits of
every finer scale, from the oracle's coefficients and the generated length / deficit tables the kernel uses, for every p, random
splits and both extremes.  All counted, the bound is the `bits - deficit` the kernel has always used."""
import numpy as np

import mdec_hard_content as H
import oracle_lib as O

SPLITS = 20


def noise_frames():
    return [("noise +-%d 320x240" % amp, 320, 240, O.synth_frames(320, 240, 8, seed=7, amp=amp)[5]) for amp in (4, 8, 16)]


def macroblock_curves(w, h, frame):
    """per macroblock (encode order; the oracle hands the coefficients out block-major: (6, macroblocks, 64)) and scale: AC bits,
    deficit sums -- (nmb, 64) each, column 0 unused"""
    tb, df = H.block_curves(H.frame_blocks(w, h, frame))
    nmb = (w // 16) * (h // 16)
    assert tb.shape[0] == 6 * nmb
    return tb.reshape(6, nmb, 64).sum(axis=0), df.reshape(6, nmb, 64).sum(axis=0)


def check_frame(k, name, w, h, frame):
    tb, df = macroblock_curves(w, h, frame)
    nmb = tb.shape[0]
    g = tb - df                                        # per macroblock and scale: the proven floor for all finer scales
    total = tb.sum(axis=0)                             # true AC bits per scale (the fixed bits are the same on both sides)
    floor = np.minimum.accumulate(np.where(np.arange(64) >= 1, total, np.iinfo(np.int64).max))     # min over s' <= s of bits(s')
    rng = np.random.default_rng(1000 + k)
    splits = np.concatenate([np.ones((1, nmb), np.int64), np.zeros((1, nmb), np.int64),
                             (rng.random((SPLITS, nmb)) < rng.random((SPLITS, 1))).astype(np.int64)])     # 1 = counted
    assert splits.shape[0] == SPLITS + 2
    worst = None
    for p in range(2, 64):
        bound = splits @ g[:, p - 1] + (1 - splits) @ g[:, p]
        assert (bound <= floor[p - 1]).all(), (name, p, bound.tolist(), int(floor[p - 1]))
        assert bound[0] == total[p - 1] - df[:, p - 1].sum(), (name, p)       # all counted: today's bits - deficit
        assert bound[1] == total[p] - df[:, p].sum(), (name, p)               # none counted: the emit scale's own bound
        slack = int((floor[p - 1] - bound).min())
        worst = slack if worst is None else min(worst, slack)
    return worst


def test_mixed_bound_on_noise():
    for k, (name, w, h, frame) in enumerate(noise_frames()):
        print("%s: tightest mixed bound is %d bits under the true minimum" % (name, check_frame(k, name, w, h, frame)))


def test_mixed_bound_on_the_hard_content_catalogue():
    cat = H.catalogue()
    assert {"dip", "loose", "ordinary"} <= {f.kind for f in cat} and len(cat) >= 30
    tight = [check_frame(10 + k, f.name, f.w, f.h, f.frame) for k, f in enumerate(cat)]
    print("%d catalogue frames; tightest mixed bound per frame: min %d, median %d bits under the true minimum"
          % (len(cat), min(tight), int(np.median(tight))))
    assert min(tight) >= 0


def test_the_code_table_carries_the_same_lengths_and_deficits_as_the_length_table():
    """an uncounted macroblock folds bits and deficit of its emitted codes from the CODE table (bits << 24 | deficit << 17 | code),
    a counted one from the length table (bits | deficit << 8): cell by cell the same numbers, and cell 0 (no code) is empty"""
    len16, code, _, _ = H.header_tables()
    assert np.array_equal(code >> 24, len16 & 0xFF)
    assert np.array_equal((code >> 17) & 0xF, len16 >> 8)
    assert (len16 >> 8).max() <= 0xF
    assert len16[0, 0] == 0 and code[0, 0] == 0
