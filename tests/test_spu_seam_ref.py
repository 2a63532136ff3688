"""The statement of "psxhip SPU loop seam v1" (tests/spu_seam_ref.py) against brute force, on the CPU: the
seam-block rule against the flags the reference's framing loop writes, the fixed points against a decoder that plays the loop, the
report's early exit against two whole decodes; and that the corpus (tests/spu_seam_corpus.py) holds what it says."""
import numpy as np

import adpcm_decode_ref as R
import spu_bank_corpus as B
import spu_seam_corpus as K
import spu_seam_ref as S


def test_the_corpus_holds_every_kind_of_entry_and_of_outcome():
    ents, pcm = K.bank()
    assert len(ents) == 24 and {e["samples"] for e in ents} == {28, 29, 56, 300, 1125}
    assert 100 <= min(r[4] for r in K.RECIPES) and max(r[4] for r in K.RECIPES) == 32000
    assert any(r[5] == 0 for r in K.RECIPES) and any(r[5] > 0 for r in K.RECIPES)
    for k in range(4):
        _, p, seams, outcome = K.expected(k, 0, S.STEADY)
        D = [r[3] for r in p["rows"]]
        assert any(s == 0 and d > 1 for s, d in zip(seams, D)) and any(0 < s < d - 1 for s, d in zip(seams, D))
        assert any(s == d - 1 and d > 1 for s, d in zip(seams, D))
        assert any(not e["enable_loop"] and e["loop"] < 0 for e in ents), "no loop"
        assert any(e["enable_loop"] and e["loop"] >= 0 and r[6] < 0 for e, r in zip(ents, p["rows"])), "a loop point behind the end"
        assert any(not e["enable_loop"] and r[6] >= 0 and s < 0 for e, r, s in zip(ents, p["rows"], seams)), "a loop point without enable_loop"
        none = [s for e, s in zip(ents, seams) if e["enable_loop"] and e["loop"] < 0]
        assert none and all(s == (0 if K.MIXED_SETTINGS[k]["no_dummy"] else -1) for s in none), "enable_loop without a loop point"
        # the outcomes, from the statement alone
        assert all((o == -1) == (s < 0) for o, s in zip(outcome, seams))
        assert sum(o == 0 for o in outcome) >= 2, outcome
        assert sum(2 <= o < S.PASSES for o in outcome) >= 2, outcome
        assert sum(o == S.PASSES for o in outcome) >= 2, outcome
    assert {s["no_dummy"] for s in K.MIXED_SETTINGS} == {False, True}


def test_the_material_is_periodic_over_the_body():
    """everything in an entry repeats with the body's length: where the intro is longer than the body, it already holds the body's
    samples one period early (to the rounding of a sample)"""
    ents, pcm = K.bank()
    checked = 0
    for e, (samples, _, _, partials, amplitude, noise, seed) in zip(ents, K.RECIPES):
        start = e["loop"] * e["freq"] // 28000 if e["loop"] >= 0 else 0
        first = 28 * start if 28 * start < samples else 0
        n = samples - first
        x = pcm[e["pcm_offset"]:e["pcm_offset"] + samples].astype(np.int64)
        assert np.array_equal(x, K.material(samples, first, partials, amplitude, noise, seed)), "deterministic"
        if first >= n:
            assert np.abs(x[first - n:first] - x[first:first + n]).max() <= 1
            checked += 1
    assert checked >= 3


def test_the_seam_block_is_where_the_reference_s_flags_send_the_loop():
    """brute force: the block a voice jumps to at LOOP_REPEAT, read from the reference's file -- the block flagged LOOP_START, or,
    without one, the voice's start address (key-on sets the repeat address to it): the dummy block, which is no data block, or
    data block 0"""
    ents, pcm = K.bank()
    seen = set()
    for k, s in enumerate(K.MIXED_SETTINGS):
        bank, p = B.ref_bank(s, ents, pcm)
        for e, row, base in zip(ents, p["rows"], p["unit_base"]):
            D, dummy = row[3], row[2]
            body = bank[16 * (base - dummy):16 * (base + D)].reshape(-1, 16)          # the voice's blocks from its start address on
            if not (D > 0 and body[-1, 1] & 1 and body[-1, 1] & 2):
                want = -1                                                             # the voice ends, or runs into the trap block
            else:
                flagged = [u for u in range(len(body)) if body[u, 1] & 4]
                target = flagged[0] if flagged else 0
                want = target - dummy if target >= dummy else -1
            assert S.seam_block(s, e) == want, (k, e)
            seen.add((want < 0, want == 0, bool(dummy)))
    assert len(seen) >= 5


def test_a_fixed_entry_is_a_fixed_point_of_the_decoder():
    """for every entry fixed at pass k, a decoder started at e_k ends at e_k, and what it decodes is what the encoder reconstructed
    (the state the next unit was encoded from is the decoder's state there); an entry without a fixed point keeps pass 0's blocks"""
    ents, pcm = K.bank()
    for beam in (0, 2):
        xs = [S.padded(e, pcm) for e in ents]
        seams = [S.seam_block(K.MIXED_SETTINGS[2], e) for e in ents]
        off, _ = S.encode_entries(xs, seams, beam, S.OFF)
        blocks, outcome = S.encode_entries(xs, seams, beam, S.STEADY)
        fixed = 0
        for e, x, s, blk, first, o in zip(ents, xs, seams, blocks, off, outcome):
            if s < 0 or o == S.PASSES or o == 0:
                assert np.array_equal(blk, first), "pass 0's blocks are those of mode OFF"
            assert np.array_equal(blk[:max(s, 0)], first[:max(s, 0)]), "the intro is never touched"
            if s < 0 or o == S.PASSES:
                continue
            # brute force: encode the body from every state the chain of passes visits, without the bookkeeping
            state = S.encode_chains([x[:28 * s]], [(0, 0)], beam)[0][1] if s > 0 else (0, 0)
            for _ in range(o):
                state = S.encode_chains([x[28 * s:]], [state], beam)[0][1]
            body, end = S.encode_chains([x[28 * s:]], [state], beam)[0]
            assert end == state and np.array_equal(body, blk[s:])
            y, after, _ = R.decode_chain(blk[s:], 4, 5, state)
            assert after == state, "the decoder's loop closes"
            again, after2, _ = R.decode_chain(blk[s:], 4, 5, after)
            assert after2 == state and np.array_equal(again, y), "every repeat is the same samples"
            fixed += 1
        assert fixed >= 8


def test_the_early_exit_is_the_two_whole_decodes():
    ents, pcm = K.bank()
    rng = np.random.default_rng(5)
    shapes = set()
    for k in (0, 2):
        for mode in (S.OFF, S.STEADY):
            bank, p, seams, _ = K.expected(k, 0, mode)
            for e, base, row, s in zip(ents, p["unit_base"], p["rows"], seams):
                blk = bank[16 * base:16 * (base + row[3])].reshape(-1, 16)
                for x in (None, S.padded(e, pcm)):
                    full = S.report(blk, s, x)
                    assert S.report_early(blk, s, x) == full, (k, mode, e)
                if s >= 0:
                    shapes.add((full["settled"], full["first_units"] == row[3] - s, full["first_units"] == 0))
    # blocks nobody encoded: random bytes, and a stream that never forgets its start state
    for D, s in ((1, 0), (7, 0), (7, 3), (7, 6), (40, 11)):
        for blk in (rng.integers(0, 256, (D, 16)).astype(np.uint8), R.fixed_point_stream(D)):
            x = rng.integers(-32768, 32768, 28 * D).astype(np.int16)
            full = S.report(blk, s, x)
            assert S.report_early(blk, s, x) == full
            shapes.add((full["settled"], full["first_units"] == D - s, full["first_units"] == 0))
    assert {(1, False, False), (1, False, True)} <= shapes and any(not sh[0] for sh in shapes), shapes
    assert S.report(np.zeros((3, 16), np.uint8), -1, None) == dict.fromkeys(S.FIELDS, 0) | {"seam_block": -1}


def settled_of_fixed(k, beam):
    """[(entry, outcome, settled)] of the entries of the statement's STEADY bank that are fixed at a pass k > 0"""
    ents, pcm = K.bank()
    bank, p, seams, outcome = K.expected(k, beam, S.STEADY)
    out = []
    for i, (e, base, row, s, o) in enumerate(zip(ents, p["unit_base"], p["rows"], seams, outcome)):
        if 0 < o < S.PASSES:
            out.append((i, o, S.report(bank[16 * base:16 * (base + row[3])].reshape(-1, 16), s, S.padded(e, pcm))["settled"]))
    return out


def test_the_corpus_s_fixed_entries_are_settled_by_choice_of_material():
    """the corpus's second condition (tests/spu_seam_corpus.py), from the statement alone, under both beams and all four settings"""
    for k in range(4):
        for beam in (0, 2):
            fixed = settled_of_fixed(k, beam)
            assert len(fixed) >= 4 and all(settled == 1 for _, _, settled in fixed), (k, beam, fixed)


def test_fixed_is_a_promise_about_the_encoder_s_loop_not_about_the_first_time_through():
    """The first time through, the decoder enters the body with s_0, not with the s_k the kept pass was planned from.  Where it has
    not run into the encoder's states by the end of the body, pass 2 does not start from e_k either, and the report need not say
    `settled`.  The counter-example: a body of one block (two partials, amplitude 900, the corpus's recipe with seed 1), fixed at
    pass 3.  What the report then shows is the price of the mode: pass 1 of such an entry is worse than under mode OFF, every later
    pass better"""
    x = K.material(28, 0, 2, 900, 0, 1)
    (plain,), _ = S.encode_entries([x], [0], 0, S.OFF)
    (steady,), (outcome,) = S.encode_entries([x], [0], 0, S.STEADY)
    r, r0 = S.report(steady, 0, x), S.report(plain, 0, x)
    print("outcome %d; steady %s; off %s" % (outcome, r, r0))
    assert outcome == 3 and r["settled"] == 0 and (r["first_units"], r["first_peak"]) == (1, 252)
    assert (r0["pass1_err"], r["pass1_err"]) == (6001, 755111) and (r0["pass2_err"], r["pass2_err"]) == (1386354, 28827)
