"""psxhip MDEC reconstruct v1 (tests/mdec_recon_ref.py) against the oracle's float64 reconstruction (orc_mdec_reconstruct: exact
dequantisation, cosine IDCT, lrint), on every stream the oracle's encoder produced for the parse tests.  The per-pixel bound is
derived from the statement's own constants and shifts, the mean error must be unbiased, and the no-overflow claim is a computed
worst case."""
import re
import os

import numpy as np

import mdec_decode_corpus as DC
import mdec_recon_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_rounded_cosines_and_the_headers():
    c = R.idct_matrix()
    assert np.array_equal(c, np.rint(R.real_matrix() * 2.0 ** R.CBITS).astype(np.int64))
    assert sorted(set(np.abs(c).ravel().tolist())) == sorted(set(R.IDCT_MAG[1:]))
    src = open(os.path.join(ROOT, "psxavenc_amd/csrc/bs_vlc_decode.h")).read()

    def arr(name):
        m = re.search(name + r"\[\d+\] = \{(.*?)\};", src, re.S)
        return np.array([int(x, 0) for x in m.group(1).replace("\n", " ").split(",") if x.strip()], np.int64)
    assert np.array_equal(arr("bs_dec_quant"), R.QUANT)
    assert np.array_equal(arr("bs_dec_zigzag")[R.zagzig()], np.arange(64))
    assert np.array_equal(arr("bs_dec_idct"), c.ravel())


def test_no_intermediate_overflows_32_bits():
    wc = R.worst_case()
    for name, v in wc.items():
        assert v < 2 ** 31, (name, v)
    assert wc["T"] < 2 ** 15 + 2 ** 14           # what the column pass was sized for
    # the device's min(scale, SAT) gives the saturated product of the statement for every scale
    lv = np.array([-512, -1, 0, 1, 40, 511], np.int64)[:, None, None]
    q = np.array([2, 16, 83], np.int64)[None, :, None]
    s = np.array([0, 1, 63, R.SAT - 1, R.SAT, R.SAT + 1, 65535], np.int64)[None, None, :]
    assert np.array_equal(np.clip(lv * q * s, -R.SAT, R.SAT - 1), np.clip(lv * q * np.minimum(s, R.SAT), -R.SAT, R.SAT - 1))
    # and the statement itself at the corners: every coefficient saturated, either sign, checkerboard signs
    for f in (np.full((1, 8, 8), R.SAT - 1), np.full((1, 8, 8), -R.SAT),
              (np.indices((8, 8)).sum(axis=0) % 2 * (2 * R.SAT - 1) - R.SAT)[None]):
        c = R.idct_matrix()
        row = np.einsum("bvu,ux->bvx", f.astype(np.int64), c)
        assert np.abs(row).max() + (1 << (R.SHIFT1 - 1)) <= wc["row sum"]
        t = (row + (1 << (R.SHIFT1 - 1))) >> R.SHIFT1
        assert np.abs(t).max() <= wc["T"]
        assert np.abs(np.einsum("bvx,vy->byx", t, c)).max() + (1 << (R.SHIFT2 - 1)) <= wc["column sum"]


def test_statement_is_within_its_derived_bound_of_the_oracle(oracle):
    O = oracle
    n_px, n_off, worst = 0, 0, 0
    for case, _ in DC.clean_cases():
        rc, levels, q, _, _ = DC.oracle_decode(case)
        assert rc == 0
        want = O.mdec_reconstruct(case.w, case.h, levels, q).astype(np.int64)
        got = R.reconstruct(case.w, case.h, levels, q).astype(np.int64)
        f8 = R.dequantise(levels, q)
        bound = R.place(case.w, case.h, np.minimum(np.broadcast_to(R.pixel_bound(f8)[:, None, None], f8.shape), 255)).astype(np.int64)
        d = np.abs(got - want)
        assert (d <= bound).all(), (case.name, int(d.max()), int(bound.max()))
        n_px += d.size
        n_off += int((d != 0).sum())
        worst = max(worst, int(d.max()))
    print("pixels %d, differing %d (%.3f %%), worst %d" % (n_px, n_off, 100.0 * n_off / n_px, worst))


def test_mean_error_on_noise_is_unbiased(oracle):
    """against the real-valued pixels (before lrint), over noise content: |mean| < 0.05, the scaler tests' figure"""
    O = oracle
    tot, n = 0.0, 0
    for codec in (0, 1):
        fr = O.synth_frames(320, 240, 4, seed=77, amp=40)
        out, res, rc = O.mdec_encode(codec, 320, 240, fr, 30000)
        assert rc == 0
        for i in range(fr.shape[0]):
            rc, levels, q, _, _ = O.mdec_decode(320, 240, out[i])
            f8 = R.dequantise(levels, q)
            cs = R.real_matrix()
            real = np.einsum("bvu,ux,vy->byx", f8 / 8.0, cs, cs) + 128.0
            got = R.idct_blocks(f8).astype(np.float64)
            inside = (real > 0.5) & (real < 254.5)               # the clamp is not an error of the arithmetic
            tot += float((got - real)[inside].sum())
            n += int(inside.sum())
    assert n > 500000 and abs(tot / n) < 0.05, (tot / n, n)


def test_placement_is_the_encoders_block_order(oracle):
    """a frame of flat blocks with distinct DCs lands where orc_mdec_reconstruct puts it, exactly (a flat block has no rounding)"""
    O = oracle
    w, h = 48, 32
    levels = np.zeros((6 * 6, 64), np.int16)
    levels[:, 0] = (np.arange(36) * 4 - 60)                       # pixel = 128 + DC * 2 / 8
    assert np.array_equal(R.reconstruct(w, h, levels, 1), O.mdec_reconstruct(w, h, levels, 1))
