"""CPU tests of what the MDEC rate-control search takes on trust (csrc/mdec_search.h): the refinement deficit in csrc/bs_vlc_lut.h is
a valid lower bound (a failing coarse scale may only rule out finer ones when bits - deficit still exceeds the budget) and as tight as
claimed; both kernels' tables carry the same deficit; the budget -> bit limit formula is the bit writer's; and the policy returns the
first fit on the real, non-monotone curves of tests/mdec_hard_content.py.  Reference throughout: the CPU oracle (oracle/) and brute
force; the generator's own recursion (tools/gen_tables.py::refinement_deficit) is not consulted."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mdec_hard_content as H
import oracle_lib as O

LEVELS = list(range(1, 43)) + [100, 510]


@pytest.fixture(scope="module")
def oracle_lens():
    """code lengths from the oracle's own table: (rows |level| = 0..41 as the kernels clamp it, runs 0..62)"""
    L = O.lib()
    t = np.zeros((H.LUT_H, H.LUT_W), np.int64)
    for lv in range(1, H.LUT_H):
        for run in range(H.LUT_W):
            t[lv, run] = L.orc_mdec_ac_code(run, lv) >> 24
    return t


# ---------------------------------------------------------------- the oracle's curve
def test_need_curve_gives_the_encoders_answer_at_every_threshold():
    """oracle_lib.mdec_need against the encoder the suite already trusts: at budget need[s], need[s] - 1 and need[s] - 2 for every s,
    orc_mdec_encode_frame answers min{k : need[k] <= budget} (an odd budget loses its last byte), or reports that nothing fits"""
    cat = H.catalogue()
    picks = [f for f in cat if (f.w, f.h) == (48, 32)][:6] + [f for f in cat if (f.w, f.h) == (192, 128)][:2] + [cat[4]]
    assert any(f.dips() for f in picks)
    n = 0
    for f in picks:
        for codec in ((0, 1, 2) if f.w == 48 else (f.codecs[0],)):
            need = f.need(codec)
            for b in f.budgets(codec)[::(1 if f.w == 48 else 4)]:
                want = H.first_fit(need, b)
                _, res, rc = O.mdec_encode(codec, f.w, f.h, f.frame[None, :], b)
                assert (rc == -2 and want == 64) or (rc == 0 and res[0, 0] == want), (f.name, codec, b, want, rc, res)
                if rc == 0:
                    assert res[0, 1] == (need[want] + 3) & ~3
                n += 1
    assert n > 2000


def test_catalogue_has_what_the_gpu_tests_need():
    """(catalogue() asserts its own properties when it is built; here the counts the GPU tests assert again, from the curves alone)"""
    cat = H.catalogue()
    for codec in (0, 1, 2):
        differ = late = 0
        answers = set()
        for f in cat:
            if codec in f.codecs:
                need = f.need(codec)
                for b in f.budgets(codec):
                    ff = H.first_fit(need, b)
                    answers.add(ff)
                    differ += ff != H.last_fail_plus_one(need, b)
                    late += ff < 64 and need[63] > b - (b & 1)
        assert differ >= 100 and late >= 2 and len(answers - {64}) >= 40, (codec, differ, late, len(answers))
    assert all(b >= 8 for f in cat for b in f.budgets(f.codecs[0]))


# ---------------------------------------------------------------- the table the kernels read
def test_both_tables_carry_the_same_deficit_and_the_oracles_lengths(oracle_lens):
    len16, code, quant, zz = H.header_tables()
    lens, defs = len16 & 0xFF, len16 >> 8
    assert np.array_equal((code >> 17) & 0x7F, defs), "bs_ac_code_lut and bs_ac_len16_lut disagree on a deficit"
    assert np.array_equal(code >> 24, lens)
    assert defs.max() <= 15 and not defs[0].any() and not lens[0].any()
    assert np.array_equal(lens, oracle_lens)
    L = O.lib()
    for run in range(63):
        for lv in LEVELS:                           # rows past the table's last one are read from it: all escapes
            assert lens[min(lv, H.LUT_H - 1), run] == L.orc_mdec_ac_code(run, lv) >> 24 == L.orc_mdec_ac_code(run, -lv) >> 24
        for lv in range(1, H.LUT_H):                # the code bits (sign slot cleared); an escape carries none
            w = L.orc_mdec_ac_code(run, lv)
            assert code[lv, run] & 0x1FFFF == (0 if (w >> 24) == 22 else w & 0xFFFFFF), (run, lv)
    # what makes "the magnitudes at their minimum" the cheapest refinement: a longer level never costs less
    assert (np.diff(lens[1:], axis=0) >= 0).all()
    sys.path.insert(0, os.path.join(O.ROOT, "tools"))
    import gen_tables as G
    assert quant.tolist() == [G.QUANT[i] for i in G.zagzig()] and zz.tolist() == G.zagzig()


def _cost(lens, digits, last, runs_before=0):
    """bits of `digits` (patterns x positions: 0 = still zero, m = a coefficient of magnitude m) followed by a coefficient of
    magnitude `last` (patterns,): the codes a finer scale writes where a coarser one wrote (run = positions, level)"""
    n = digits.shape[0]
    run = np.full(n, runs_before, np.int64)
    cost = np.zeros(n, np.int64)
    for i in range(digits.shape[1]):
        m = digits[:, i]
        hit = m > 0
        cost += np.where(hit, lens[np.minimum(m, H.LUT_H - 1), np.where(hit, run, 0)], 0)
        run = np.where(hit, 0, run + 1)
    return cost + lens[np.minimum(last, H.LUT_H - 1), run]


def test_deficit_equals_brute_force_for_runs_up_to_10(oracle_lens):
    """every way r <= 10 zeros can turn into coefficients of magnitude 1..3 before a last magnitude L..L + 2, L = 1..41: the cheapest
    costs exactly len - deficit -- the bound is valid and as tight as the table claims"""
    lens, defs = H.luts()[:2]
    assert np.array_equal(lens, oracle_lens)
    for r in range(11):
        k = np.arange(4 ** r, dtype=np.int64)
        digits = np.stack([(k >> (2 * i)) & 3 for i in range(r)], axis=1) if r else np.zeros((1, 0), np.int64)
        # the prefix's cost and the zeros left before the last coefficient; the last coefficient's code is added per (L, magnitude)
        n = digits.shape[0]
        run = np.zeros(n, np.int64)
        cost = np.zeros(n, np.int64)
        for i in range(r):
            m = digits[:, i]
            hit = m > 0
            cost += np.where(hit, oracle_lens[m, np.where(hit, run, 0)], 0)
            run = np.where(hit, 0, run + 1)
        cheapest_prefix = np.array([cost[run == t].min() for t in range(r + 1)])
        for L in range(1, H.LUT_H):
            best = min(int((cheapest_prefix + oracle_lens[min(last, H.LUT_H - 1), :r + 1]).min()) for last in (L, L + 1, L + 2))
            assert best == lens[L, r] - defs[L, r], (r, L, best, int(lens[L, r]), int(defs[L, r]))


def test_no_random_refinement_beats_the_bound(oracle_lens):
    """every run up to 62, every L: 2000 random refinements each (random subsets of the zeros -- few insertions mostly, where an escape
    gets split into short codes --, random magnitudes, a last magnitude >= L); none costs less than len - deficit.  The 2000 ways the
    zeros fill in are drawn once per run and shared by its 41 values of L (their cost does not depend on L); the last magnitude is
    drawn per (run, L)."""
    lens, defs = H.luts()[:2]
    rng = np.random.default_rng(62)
    n = 2000
    tight = 0
    for r in range(63):
        p = rng.choice([0.0, 0.5 / max(r, 1), 1.0 / max(r, 1), 2.0 / max(r, 1), 0.1, 0.3, 0.7], n)[:, None]
        mags = np.where(rng.random((n, r)) < 0.8, rng.integers(1, 4, (n, r)), rng.integers(1, 60, (n, r)))
        digits = np.where(rng.random((n, r)) < p, mags, 0).astype(np.int64)
        for L in range(1, H.LUT_H):
            last = L + np.where(rng.random(n) < 0.7, 0, rng.integers(0, 12, n))
            cost = _cost(oracle_lens, digits, last)
            floor = lens[L, r] - defs[L, r]
            assert cost.min() >= floor, (r, L, int(cost.min()), int(floor))
            tight += cost.min() == floor
    assert tight >= 63 * 41 // 2          # (the sampler finds the cheapest refinement itself more often than not)


# ---------------------------------------------------------------- the bound on blocks
def _suite_content_blocks():
    """blocks of the content classes the GPU tests use, at a size that keeps this quick"""
    sys.path.insert(0, os.path.join(O.ROOT, "tests", "golden"))
    from make_mdec_golden import special_frames
    w, h = 192, 128
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:h, 0:w]
    frames = [O.synth_frames(w, h, 1, seed=40 + a, amp=a)[0] for a in (0, 1, 3, 8, 30)] + list(special_frames(w, h))
    sparse = np.full((h, w), 90)
    sparse[rng.integers(0, h, 40), rng.integers(0, w, 40)] = rng.integers(0, 256, 40)
    for y in (sparse, np.kron(rng.integers(0, 256, (h // 8, w // 8)), np.ones((8, 8), np.int64)),
              ((xx // 3 + yy // 5) % 2) * 200 + rng.integers(0, 3, (h, w)), rng.integers(0, 256, (h, w)), (xx & 1) * 255):
        f = np.full(w * h * 3 // 2, 128, np.uint8)
        f[:w * h] = np.clip(y, 0, 255).astype(np.uint8).ravel()
        f[w * h:] = rng.integers(100, 156, w * h // 2)
        frames.append(f)
    return np.concatenate([H.frame_blocks(w, h, f) for f in frames])


def _coefficient_blocks(rng, n):
    """coefficient-domain blocks: sparse and dense, magnitudes up to the int16 range, and levels put either side of the table's last
    row (41) and of the clamp (510 / 512) at a scale of their own"""
    quant = H.luts()[2]
    out = np.zeros((n, 64), np.int64)
    for i in range(n):
        kind = i % 5
        top = (3, 40, 300, 3000, 32767)[(i // 5) % 5]
        if kind < 3:                                 # sparse: 1..19 terms
            k = int(rng.integers(1, 20))
            pos = rng.choice(np.arange(1, 64), k, replace=False)
            out[i, pos] = rng.integers(1, top + 1, k)
        elif kind == 3:                              # dense
            out[i, 1:] = rng.integers(0, top + 1, 63) * (rng.random(63) < rng.uniform(0.3, 1.0))
        else:                                        # levels 39..43 and 508..514 at scale s, sparse or dense
            s = int(rng.integers(1, 64))
            k = int(rng.integers(1, 40))
            pos = rng.choice(np.arange(1, 64), k, replace=False)
            lv = rng.choice([39, 40, 41, 42, 43, 508, 509, 510, 511, 512, 513, 514], k)
            out[i, pos] = np.minimum(lv * quant[pos] * s, 32767)
    return out


def test_block_bits_follow_the_oracles_code_lengths(oracle_lens):
    """the vectorised curve code of the helper against a plain loop over the oracle's code table, on coefficient-domain blocks"""
    lens, defs, quant, _ = H.luts()
    rng = np.random.default_rng(3)
    blocks = _coefficient_blocks(rng, 400)
    L = O.lib()
    for s in (1, 2, 5, 13, 31, 63):
        got = H.block_bits(blocks, s, lens, defs, quant)[0]
        for b in range(blocks.shape[0]):
            bits, run = 0, 0
            for i in range(1, 64):
                d = int(quant[i]) * s
                lv = min((2 * int(blocks[b, i]) + d) // (2 * d), 510)
                if lv == 0:
                    run += 1
                else:
                    bits += L.orc_mdec_ac_code(run, lv) >> 24
                    run = 0
            assert bits == got[b], (s, b)


def test_refinement_bound_holds_on_every_block_and_pair_of_scales():
    """bits(block, s) >= bits(block, s') - deficits(block, s') for every s <= s': blocks of every catalogue frame and of the suite's
    content classes, and 20 000 coefficient-domain blocks; with enough non-monotone and loose-bound blocks for that to mean something"""
    cat = H.catalogue()
    real = np.concatenate([np.unique(H.frame_blocks(f.w, f.h, f.frame), axis=0) for f in cat] + [_suite_content_blocks()])
    real = np.unique(real, axis=0)
    made = _coefficient_blocks(np.random.default_rng(20000), 20000)
    nonmono = loose = 0
    for name, blocks in (("frames", real), ("coefficients", made)):
        tb, df = H.block_curves(blocks)
        tb, fb = tb[:, 1:], tb[:, 1:] - df[:, 1:]
        floor = np.minimum.accumulate(tb, axis=1)            # min over s <= s' of bits(s)
        bad = np.nonzero((floor < fb).any(axis=1))[0]
        assert bad.size == 0, "%s: the bound fails on %d blocks, first %s" % (name, bad.size, blocks[bad[0]].tolist())
        nm = (np.diff(tb, axis=1) > 0).any(axis=1)
        ls = (fb < floor).any(axis=1)
        print("%s: %d blocks, %d non-monotone, %d with a loose bound somewhere, %d with a deficit somewhere"
              % (name, blocks.shape[0], nm.sum(), ls.sum(), (df > 0).any(axis=1).sum()))
        nonmono += int(nm.sum())
        loose += int(ls.sum())
    assert real.shape[0] >= 5000 and made.shape[0] >= 20000
    assert nonmono >= 500 and loose >= 5000, (nonmono, loose)


# ---------------------------------------------------------------- budget -> bit limit
def test_limit_bits_is_the_bit_writers_capacity():
    """the kernels turn a budget into limit_bits = 16 * ((budget - 8) >> 1).  The oracle's bit writer (the reference's, capacity test
    between the two bytes of a word) accepts a stream of b bits exactly when b <= that: with the exact bit counts of real streams
    (8 .. 68 000 bytes) and even and odd budgets either side of each, the encoder's answer is the first scale within the limit"""
    cat = H.catalogue()
    tiny = H.Frame("one macroblock", 16, 16, H.tile(H.dip_macroblocks(2024, 176)[3][0], 16, 16), "dip")
    picks = [(tiny, 1), (next(f for f in cat if (f.w, f.h) == (48, 32)), 1), (next(f for f in cat if (f.w, f.h) == (192, 128)), 3),
             (cat[1], 9), (next(f for f in cat if f.kind == "loose"), 9)]
    seen = set()
    for f, step in picks:
        for codec in (0, 1):
            tb, _, _ = H.exact_bits(codec, f.w, f.h, f.frame)
            for s in range(1, 64, step):
                words = (int(tb[s]) + 15) // 16
                for budget in (8 + 2 * words + k for k in (-3, -2, -1, 0, 1, 2)):
                    if budget < 8:
                        continue
                    limit = 16 * ((budget - 8) >> 1)
                    want = next((k for k in range(1, 64) if tb[k] <= limit), 64)
                    _, res, rc = O.mdec_encode(codec, f.w, f.h, f.frame[None, :], budget)
                    assert (rc == -2 and want == 64) or (rc == 0 and res[0, 0] == want), (f.name, codec, s, budget, want, rc, res)
                    seen.add(budget)
    for f, codec, budget in ((cat[1], 0, 70000), (cat[1], 0, 70001), (tiny, 0, 8), (tiny, 0, 9)):
        _, res, rc = O.mdec_encode(codec, f.w, f.h, f.frame[None, :], budget)
        tb, _, _ = H.exact_bits(codec, f.w, f.h, f.frame)
        want = next((k for k in range(1, 64) if tb[k] <= 16 * ((budget - 8) >> 1)), 64)
        assert (rc == -2 and want == 64) or (rc == 0 and res[0, 0] == want)
    assert min(seen) < 40 and max(seen) > 60000 and any(b & 1 for b in seen) and any(not b & 1 for b in seen)


# ---------------------------------------------------------------- the policy on real curves
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("search") / "libsearch_sim.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-o", so, os.path.join(O.ROOT, "tests/cpu/search_sim.cpp")], check=True)
    L = C.CDLL(so)
    ip = C.POINTER(C.c_int)
    L.search_sim.argtypes = [ip, ip, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, ip]
    return L


def test_search_policy_returns_the_first_fit_on_real_non_monotone_curves(sim):
    """csrc/mdec_search.h driven by every catalogue frame's real curve (total bits tied to oracle_lib.mdec_need, deficits from the
    header) at every threshold budget, from guesses 1, want - 1, want, want + 1, want + 2, 63 and five random ones: the first fit, with
    its stream staged"""
    rng = np.random.default_rng(35)
    ip = C.POINTER(C.c_int)
    worst, n, differ = (0, None), 0, 0
    for f in H.catalogue():
        codec = f.codecs[0]
        need = f.need(codec)
        tb, df, fixed = H.exact_bits(codec, f.w, f.h, f.frame, need)
        t = np.ascontiguousarray(tb, dtype=np.int32)
        fb = np.ascontiguousarray(tb - df, dtype=np.int32)
        nmb = (f.w // 16) * (f.h // 16)
        for budget in f.budgets(codec):
            limit = 16 * ((budget - 8) >> 1)
            want = H.first_fit(need, budget)
            differ += want != H.last_fail_plus_one(need, budget)
            guesses = {1, want - 1, want, want + 1, want + 2, 63} | {int(g) for g in rng.integers(1, 64, 5)}
            for g in sorted(g for g in guesses if 1 <= g <= 63):
                passes, lo, hi = C.c_int(), C.c_int(), C.c_int()
                r = sim.search_sim(t.ctypes.data_as(ip), fb.ctypes.data_as(ip), limit, fixed, g, limit + 32 * nmb,
                                   C.byref(passes), C.byref(lo), C.byref(hi))
                assert r == want, (f.name, budget, g, r, want)
                n += 1
                if passes.value > worst[0]:
                    worst = (passes.value, (f.name, budget, g))
    print("%d searches, %d budgets where the first fit is not last failure + 1; most passes: %d %s" % (n, differ, worst[0], worst[1]))
    assert differ >= 100 and n >= 30000
    assert worst[0] <= 64
