"""The statement of "psxhip ADPCM beam v1" (tests/adpcm_beam_ref.py) on the corpus (tests/adpcm_beam_corpus.py), against what is
independent of it: the CPU oracle's unit encoder (B = 1 is libpsxav/adpcm.c:142-191 bit for bit), the decoder's statement
(tests/adpcm_decode_ref.py: the reported error IS the squared error of the decoded record, the new state its last two samples), the
per-unit guarantee against the oracle from the same state, and the plain form against the numpy form the other tests use.

The guarantee is per unit: nothing here compares whole chains' errors (behind the first unit that differs the two encoders carry
different states), and nothing compares the errors of two beam widths (a wider beam's pools differ; e is not monotone in B)."""
import numpy as np
import pytest

import adpcm_beam_corpus as BC
import adpcm_beam_ref as B
import adpcm_decode_ref as R
import adpcm_encode_corpus as K


def _units(filter_count, bits, beam):
    """(chain, unit, state before, samples, record, e, state after, pick) of every unit of the corpus"""
    rec, err, after, pick, _ = BC.expected(filter_count, bits, beam)
    for c in range(BC.N_CHAINS):
        x, before = BC.samples(c), BC.start_state(c)
        for u in range(BC.unit_count(c)):
            yield c, u, before, x[28 * u:28 * u + 28], rec[c, u], int(err[c, u]), tuple(int(v) for v in after[c, u]), pick[c, u]
            before = tuple(int(v) for v in after[c, u])


@pytest.mark.parametrize("filter_count,bits", BC.CODINGS)
def test_beam_of_one_is_the_reference_encoder(filter_count, bits):
    n = 0
    for c, u, before, x, rec, e, after, pick in _units(filter_count, bits, 1):
        want, want_state, want_e = BC.oracle_unit(x, before, filter_count, bits)
        assert np.array_equal(rec, want) and after == want_state and e == min(want_e, B.SAT) and pick[2] == 0, (c, u)
        n += 1
    assert n > 200


@pytest.mark.parametrize("beam", (2, 3, 4))
@pytest.mark.parametrize("filter_count,bits", BC.CODINGS)
def test_the_error_is_the_decoders_and_at_most_the_references(filter_count, bits, beam):
    for c, u, before, x, rec, e, after, pick in _units(filter_count, bits, beam):
        dec, _, _, _ = R.decode_unit(rec, bits, filter_count, before[0], before[1])
        dec = np.asarray(dec, np.int64)
        assert e == int(((dec - x.astype(np.int64)) ** 2).sum()), (c, u)
        assert after == (int(dec[27]), int(dec[26])), (c, u)
        assert e <= BC.oracle_unit(x, before, filter_count, bits)[2], (c, u)         # the same unit from the same state: per unit


@pytest.mark.parametrize("filter_count,bits", BC.CODINGS)
def test_plain_and_numpy_statement_agree(filter_count, bits):
    """a fixed subset recomputed with explicit lists: the short chains of every content kind and start state, all four widths, and
    the first three units of the long ones"""
    for beam in BC.BEAMS:
        rec, err, after, pick, _ = BC.expected(filter_count, bits, beam)
        for c in range(BC.N_CHAINS):
            n = min(BC.unit_count(c), 7 if beam == 4 else 3)
            r, e, a, p = B.encode_chain(BC.samples(c), BC.start_state(c), n, filter_count, bits, beam)
            assert np.array_equal(r, rec[c, :n]) and np.array_equal(e, err[c, :n]) and np.array_equal(a, after[c, :n]) and \
                np.array_equal(p, pick[c, :n]), (beam, c)


@pytest.mark.parametrize("filter_count,bits", BC.CODINGS)
def test_the_corpus_reaches_the_rules_corners(filter_count, bits):
    rec, err, after, pick, stats = BC.expected(filter_count, bits, 4, True)
    n = np.array([BC.unit_count(c) for c in range(BC.N_CHAINS)])
    on = np.arange(K.MAX_UNITS)[None, :] < n[:, None]
    assert (pick[..., 2][on] != 0).any(), "a unit whose winning path is not the anchor"
    assert (pick[..., 2][on] == 0).any(), "a unit whose winning path is the anchor"
    # the plain encoder's choice from the same incoming state
    before = np.concatenate([np.array([BC.start_state(c) for c in range(BC.N_CHAINS)], np.int32)[:, None], after[:, :-1]], axis=1)
    xs = np.stack([np.pad(BC.samples(c), (0, 28 * K.MAX_UNITS))[:28 * K.MAX_UNITS] for c in range(BC.N_CHAINS)]).reshape(BC.N_CHAINS, K.MAX_UNITS, 28)
    _, _, _, plain = B.encode_units_np(xs[on], before[on][:, 0], before[on][:, 1], filter_count, bits, 1)
    assert (plain[:, :2] != pick[on][:, :2]).any(axis=1).any(), "a unit whose (filter, shift) differs from the plain encoder's"
    assert {"rail_lo", "rail_hi", "tie", "saturated"} <= stats, stats
    # the same four through the plain form, on the chains that are there for them
    seen = set()
    for c in (BC.N_CORPUS, BC.N_CORPUS + 2, BC.N_CORPUS + 3, 7):
        B.encode_chain(BC.samples(c), BC.start_state(c), min(BC.unit_count(c), 2), filter_count, bits, 4, seen)
    assert {"rail_lo", "rail_hi", "tie", "saturated"} <= seen, seen
