"""The numpy statement of "psxhip MDEC shed v1" (tests/mdec_shed_ref.py), checked on its own: for every frame of the corpus
(tests/mdec_shed_corpus.py) all 63 K candidates are made by brute force -- the shed predicate applied to the levels, the stream written
by the independent bit writer (tests/mdec_foreign_streams.py) and measured, the distortion summed directly -- and the statement's
delta-based curves, its first fit and its acceptance must equal them.  K = 3 covers K = 1 and 2: their candidates are its first 63 and
126.  The refined rows are read back by the oracle's decoder, and the outcome is held to a recording (tests/golden/mdec_shed_ref.npz;
`python tests/mdec_shed_corpus.py` writes it), so that the statement cannot drift unnoticed.

The corpus's synthetic content produces the non-monotone case by itself (a longer run can cost more than the code it removes): no
constructed block was needed.  Its first fits in magnitude classes 2 and 3 are all declined by the acceptance; refined rows in those
classes are checked on constructed coefficients in tests/test_mdec_shed_core_cpu.py."""
import os

import numpy as np
import pytest

import mdec_foreign_streams as W
import mdec_shed_corpus as C
import mdec_shed_ref as S
import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mdec_shed_ref.npz")
FRAMES = [(gi, i) for gi, g in enumerate(C.groups()) for i in range(g.n)]


def _id(p):
    return "%s-%d" % (C.groups()[p[0]].name.replace(" ", "_"), p[1])


@pytest.mark.parametrize("gi,i", FRAMES, ids=[_id(p) for p in FRAMES])
def test_statement_equals_brute_force(gi, i):
    g = C.groups()[gi]
    b, N = int(g.budgets[i]), int(C.plain(gi)[1][i, 0])
    o3 = C.outcome(gi, i, 3)
    if N == 1 or N >= 64:
        for K in C.KS:
            o = C.outcome(gi, i, K)
            assert o.state == "untouched" and o.record() == (0, 0, 0, 0) and o.row is None
        return
    M = N - 1
    F = C.coefs(gi, i)
    lvM = S.levels(F, M)
    _, carried, _ = S.dc_terms(g.codec, F)
    ac = F.copy()
    ac[:, 0] = 0
    version = 2 if g.codec == 0 else 3
    bits, dist, gone, need = [], [], [], []
    for t in range(0, 63 * 3 + 1):
        lv = S.shed(lvM, t)
        given = lv.copy()
        given[:, 0] = carried
        data, nbits = W.write(given, version, M, wrap=g.codec == 2)
        bits.append(nbits)
        need.append(len(data))
        dist.append(int(((ac - lv * S.QUANT_ZZ * M) ** 2).sum()))
        gone.append(int(np.count_nonzero(lvM) - np.count_nonzero(lv)))
    assert bits == o3.bits.tolist() and dist == o3.dist.tolist() and gone == o3.gone.tolist()
    assert need[0] > b - (b & 1), "step 0 is the plain stream at scale M, which does not fit by the definition of N"
    assert need[0] == O.mdec_need(g.codec, g.w, g.h, g.frames[i])[M]
    d_plain = int(((ac - S.levels(F, N) * S.QUANT_ZZ * N) ** 2).sum())
    for K in C.KS:
        o = C.outcome(gi, i, K)
        assert o.bits.tolist() == bits[:63 * K + 1]
        fit = [t for t in range(1, 63 * K + 1) if need[t] <= b - (b & 1)]
        assert o.first_fit == (fit[0] if fit else 0)
        if not fit:
            assert o.state == "declined" and o.record() == (0, 0, 0, 0)
        elif dist[fit[0]] < d_plain:
            assert o.state == "refined" and o.record() == (fit[0], gone[fit[0]], d_plain, dist[fit[0]])
        else:
            assert o.state == "declined" and o.record() == (0, 0, d_plain, dist[fit[0]])


def _refined():
    return [(gi, i, K) for gi, i in FRAMES for K in C.KS if C.outcome(gi, i, K).state == "refined"]


def test_refined_rows_parse_to_the_shed_levels_and_fit():
    assert _refined()
    for gi, i, K in _refined():
        g, o = C.groups()[gi], C.outcome(gi, i, K)
        b = int(g.budgets[i])
        plain_rows, plain_res = C.plain(gi)
        assert o.row.shape == (b,) and o.result[0] == plain_res[i, 0] - 1 and o.result[1] <= ((b - (b & 1)) + 3 & ~3)
        rc, lv, q, v, nbits = O.mdec_decode(g.w, g.h, o.row, v3dc_wrap=int(g.codec == 2))
        assert (rc, q, v, nbits) == (0, o.M, 2 if g.codec == 0 else 3, int(o.bits[o.step]))
        assert np.array_equal(lv[:, 1:], o.lv[:, 1:])
        assert np.array_equal(lv[:, 1:], S.shed(S.levels(C.coefs(gi, i), o.M), o.step)[:, 1:])
        # the DC is never shed: what the plain row carries
        rc, lv_plain, _, _, _ = O.mdec_decode(g.w, g.h, plain_rows[i, :b], v3dc_wrap=int(g.codec == 2))
        assert rc == 0 and np.array_equal(lv[:, 0], lv_plain[:, 0])
        assert not o.row[8 + 2 * ((nbits + 15) // 16):].any()
        hwords = (int(np.count_nonzero(lv[:, 1:])) + 2 * lv.shape[0] + 2 + 63) & ~63
        assert list(o.result[2:]) == [(hwords + 1) >> 1, hwords]


def _sse(g, frame, row, b):
    rc, lv, q, _, _ = O.mdec_decode(g.w, g.h, row[:b], v3dc_wrap=int(g.codec == 2))
    assert rc == 0
    px = O.mdec_reconstruct(g.w, g.h, lv, q)
    return int(((px.astype(np.int64) - frame.astype(np.int64)) ** 2).sum())


def test_refined_frames_gain_in_pixels_over_the_corpus():
    """a condition on the corpus, not a per-frame guarantee: the acceptance lives in the coefficient domain"""
    for K in C.KS:
        plain = shed = 0
        for gi, i, k in _refined():
            if k != K:
                continue
            g, b = C.groups()[gi], int(C.groups()[gi].budgets[i])
            plain += _sse(g, g.frames[i], C.plain(gi)[0][i], b)
            shed += _sse(g, g.frames[i], C.outcome(gi, i, K).row, b)
        print("K=%d: sum of pixel SSE over the refined frames %d (plain %d)" % (K, shed, plain))
        assert shed < plain


def test_corpus_covers_the_rule():
    states = {(g.codec, C.outcome(gi, i, 3).state) for gi, g in enumerate(C.groups()) for i in range(g.n)}
    assert states == {(c, s) for c in (0, 1, 2) for s in ("untouched", "declined", "refined")}
    scales = {int(C.plain(gi)[1][i, 0]) for gi, i in FRAMES if C.outcome(gi, i, 3).state == "untouched"}
    assert scales == {1, 64}
    assert {S.step_class(C.outcome(gi, i, 3).first_fit)[0] for gi, i in FRAMES if C.outcome(gi, i, 3).first_fit} == {1, 2, 3}
    assert any(o.state == "declined" and o.first_fit == 0 for o in (C.outcome(gi, i, 3) for gi, i in FRAMES))        # nothing fits
    assert any(o.bits is not None and (np.diff(o.bits) > 0).any() for o in (C.outcome(gi, i, 3) for gi, i in FRAMES))  # bits(t) > bits(t - 1)
    assert {(g.w, g.h) for g in C.groups()} == {(16, 16), (32, 16), (48, 32), (320, 240)}
    assert any(g.uniform is not None and g.uniform % 2 for g in C.groups()) and any(g.uniform is not None and g.uniform % 2 == 0 for g in C.groups())
    assert any(g.uniform is None and len(set(g.budgets.tolist())) > 1 for g in C.groups())


def test_outcome_equals_the_recording():
    want = np.load(GOLDEN)
    got = C.recording()
    assert sorted(want.files) == sorted(got)
    for k in got:
        assert np.array_equal(want[k], got[k]), k
