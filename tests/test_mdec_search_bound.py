"""CPU simulation of the search policy (psxavenc_amd/csrc/mdec_search.h) when a (p - 1, p) pass reports a lower BOUND for the
scales <= p - 1 instead of the count at p - 1 (mdec_search_note_bound: the frame kernel stops counting at its checkpoint when the
sample says the bound will do).  On the synthetic curves of tests/test_mdec_search.py, with the count of such a pass replaced at
random by a bound anywhere in [0, true bits - deficit], and every record also run without any bound by the same program:

  * the answer is always the first scale that fits, whatever the guess;
  * a search that starts from the answer p (what a steady-state frame does) ends within one pass of the reference's ascending scan
    (`answer` passes, 63 when nothing fits): the (p - 1, p) pass finds that p fits, a bound that proves nothing is followed at once by
    a pass that counts p - 1 (mdec_search_next_after_bound), and from there every pass evaluates a scale below p - 1 nobody has;
  * from any guess a bound that proves nothing costs exactly ONE pass: the pass that counts p - 1 right after it restores the state
    a search that counted all along would be in.  So on every record in which no bound changed what the model sees,
    passes == passes without bounds + bounds that proved nothing -- an equality, asserted record by record.  The issue's "one pass
    more than the linear scan" cannot be asked from wrong guesses: the search WITHOUT any bound takes up to 48 passes more than the
    scan on these curves (tests/test_mdec_search.py allows it 64);
  * the model does see a difference where a bound PROVES (p - 1 is settled without a point at p - 1 for the two-point model: the
    issue's "no point for the two-point model") or where the emit scale's own evaluation proves p - 1 too.  From there the two
    searches predict from different points and part ways, in either direction.  What is held there: each such divergence changes
    one prediction, which the next pass's evaluation re-anchors, so over the records that diverge the mean cost must stay below one
    pass per record on top of the bounds that proved nothing; and no search, diverged or not, takes more than two passes per scale."""
import os
import subprocess

import numpy as np
import pytest

from test_mdec_search import curve, first_fit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("search_bound") / "search_bound_sim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests/cpu/search_bound_sim.cpp")], check=True)
    return exe


@pytest.mark.parametrize("kind", ["smooth", "bumpy", "flat", "noproof"])
def test_search_with_bounds_for_counts_returns_the_first_fit(prog, kind):
    rng = np.random.default_rng({"smooth": 21, "bumpy": 22, "flat": 23, "noproof": 24}[kind])
    recs, wants = [], []
    for _ in range(3000):
        fixed = int(rng.integers(3000, 30000))
        tb, fb = curve(rng, fixed, kind)
        limit = int(rng.integers(fixed - 2000, 140000))
        want = first_fit(tb, limit)
        for guess in (want if want < 64 else 63, max(1, want - 1), min(63, want + 1), int(rng.integers(1, 64))):
            recs.append(np.concatenate([[limit, fixed, guess, len(recs)], tb, fb]).astype(np.int32))
            wants.append(want)
    r = subprocess.run([prog], input=np.stack(recs).tobytes(), stdout=subprocess.PIPE, check=True, timeout=120)
    got = np.array([[int(x) for x in ln.split()] for ln in r.stdout.decode().splitlines()])
    assert got.shape == (len(recs), 7)
    answer, passes, bounds, proved, diverged, plain_answer, plain_passes = got.T
    wants = np.array(wants)
    assert np.array_equal(answer, wants), np.nonzero(answer != wants)[0][:10]
    assert np.array_equal(plain_answer, wants)
    assert bounds.sum() > 1000 and (bounds - proved).sum() > 500          # bounds did stand in for counts, and often proved nothing
    linear = np.minimum(wants, 63)
    from_answer = np.arange(len(recs)) % 4 == 0        # (the first guess of every four is the answer itself)
    assert (passes[from_answer] <= linear[from_answer] + 1).all(), (kind, (passes - linear)[from_answer].max())
    extra = passes - plain_passes - (bounds - proved)   # passes beyond "one per bound that proved nothing"
    same = diverged == 0
    print(kind, "passes: mean %.2f (%.2f without bounds), max %d (%d); %d bounds, %d proved; %d records diverged, extra passes there: mean %.2f, %d .. %d"
          % (passes.mean(), plain_passes.mean(), passes.max(), plain_passes.max(), bounds.sum(), proved.sum(), (~same).sum(),
             extra[~same].mean() if (~same).any() else 0.0, extra[~same].min() if (~same).any() else 0, extra[~same].max() if (~same).any() else 0))
    assert same.sum() * 2 >= len(recs)
    assert (extra[same] == 0).all(), (kind, np.nonzero(same & (extra != 0))[0][:10])
    if (~same).any():
        assert extra[~same].mean() <= 1.0, (kind, extra[~same].mean())
    assert passes.max() <= 2 * 63
