"""MDEC rate control on the GPU at exact budgets and on frames whose bits(scale) curve is NOT monotone.

The answer is the FIRST quant scale whose stream fits (psxavenc/mdec.c:663-723).  The frame kernel evaluates one or two scales per
pass and stops when csrc/mdec_search.h says every scale below its best fit is known to fail -- evaluated, or ruled out by a coarser
scale's bits minus its refinement deficit; the split kernel counts rounds of sixteen scales.  On monotone content "the first that
fits" and "one above the last that fails" are the same scale; tests/mdec_hard_content.py holds frames where they are not, and for
every scale of every frame the budgets at which its stream fits exactly, is one byte and is one word too long.  Bar: the bytes up to
the budget and the four result words equal the CPU oracle's, case by case; a case no scale fits reports quant_scale 64 (device entry
point) or PSXHIP_ENOFIT (host entry point).  No case is dropped.  The row of such a case is pinned to what both kernels do and
include/psxav_hip.h says: exactly frame_max_size bytes are written per frame, all zero when no scale fits (the reference asserts
there, and the oracle leaves its last attempt behind: neither is a byte to compare with); "nothing written" is the rule for a
budget outside the context's range only, which tests/test_gpu_mdec.py covers.  Rows are pre-filled, so a byte written past any
budget, odd ones included, shows.

Every threshold comes from the oracle's own curve (oracle_lib.mdec_need), every expected byte from oracle_lib.mdec_encode called for
that case.  A context takes budgets up to its max_frame_size, and that also picks the kernel's shape: the cases of a size go to a
context of 8192 bytes (two 12-wavefront groups per CU, the production shape) when their budget is at most that, else to one as
large as the largest of them (one 16-wavefront group)."""
import concurrent.futures
import ctypes as C
import os
import time

import numpy as np
import pytest

import mdec_hard_content as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

SMALL_CAP = 8192
FILL = 0xAB


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---------------------------------------------------------------- cases and what the oracle says about them
class Case:
    __slots__ = ("fi", "budget", "scale", "res", "stream")

    def __init__(self, fi, budget, rc, res, out):
        self.fi, self.budget = fi, budget
        self.scale = int(res[0]) if rc == 0 else 64
        self.res = res.copy() if rc == 0 else None
        self.stream = out[:int(res[1])].copy() if rc == 0 else None        # (past bytes_used the oracle's row is zero)


def _oracle_case(codec, f, fi, budget):
    out, res, rc = O.mdec_encode(codec, f.w, f.h, f.frame[None, :], int(budget))
    assert rc in (0, -2), rc
    if rc == 0:
        assert not out[0, int(res[0, 1]):].any()
    return Case(fi, int(budget), rc, res[0], out[0])


def _oracle_many(codec, todo):
    """[(frame, frame index, budget)] -> [Case], O.mdec_encode called for each (on a few host threads: ctypes lets go of the GIL)"""
    O.lib().orc_mdec_ac_code(0, 1)                   # builds the oracle's tables once, before the threads
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda t: _oracle_case(codec, *t), todo))


_cases = {}


def cases(codec):
    """every catalogue frame of this codec x every threshold budget of its own curve"""
    if codec not in _cases:
        t0 = time.time()
        cat = H.catalogue()
        todo = [(f, fi, b) for fi, f in enumerate(cat) if codec in f.codecs for b in f.budgets(codec)]
        cs = _oracle_many(codec, todo)
        for c in cs:                                  # the curve and the encoder agree on the answer (tests/test_mdec_bound.py, on the CPU)
            assert c.scale == H.first_fit(cat[c.fi].need(codec), c.budget)
        _cases[codec] = cs
        print("codec %d: %d cases, oracle side %.1f s" % (codec, len(cs), time.time() - t0))
    return _cases[codec]


def groups(codec, sizes=None):
    """{(w, h, context max_frame_size): [Case]}"""
    cat = H.catalogue()
    by = {}
    for c in cases(codec):
        f = cat[c.fi]
        if sizes is None or (f.w, f.h) in sizes:
            by.setdefault((f.w, f.h, c.budget <= SMALL_CAP), []).append(c)
    return {(w, h, SMALL_CAP if small else max(c.budget for c in cs)): cs for (w, h, small), cs in by.items()}


def guards(codec, cs):
    """(first fit differs from 'highest failing scale + 1', scale 63 fails yet a finer scale fits, distinct answers) from the curves"""
    cat = H.catalogue()
    differ = late = 0
    for c in cs:
        need = cat[c.fi].need(codec)
        ff = H.first_fit(need, c.budget)
        differ += ff != H.last_fail_plus_one(need, c.budget)
        late += ff < 64 and need[63] > c.budget - (c.budget & 1)
    return differ, late, len({c.scale for c in cs if c.scale < 64})


# ---------------------------------------------------------------- contexts, launches, comparison
def encoder(codec, w, h, cap, env=None):
    """a context created under the given switches (they are read when the context is created)"""
    from psxavenc_amd.mdec import MdecEncoder
    env = dict(env or {})
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return MdecEncoder(codec, w, h, max_frame_size=cap, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


SPLIT_ON = {"PSXHIP_MDEC_SPLIT_MAX": None}
SPLIT_OFF = {"PSXHIP_MDEC_SPLIT_MAX": "0"}


class Uploaded:
    """the distinct frames of a list of cases on the device, and row -> frame"""
    def __init__(self, torch, cs):
        cat = H.catalogue()
        fis = sorted({c.fi for c in cs})
        self.at = {fi: k for k, fi in enumerate(fis)}
        self.d = torch.from_numpy(np.stack([cat[fi].frame for fi in fis])).to("cuda:0")
        self.torch = torch

    def rows(self, cs):
        idx = self.torch.tensor([self.at[c.fi] for c in cs], dtype=self.torch.int64, device="cuda:0")
        d_frames = self.d.index_select(0, idx)
        d_budgets = self.torch.tensor([c.budget for c in cs], dtype=self.torch.int32, device="cuda:0")
        return d_frames, d_budgets


def launch(torch, enc, d_frames, d_budgets, cap):
    d_out = torch.full((d_frames.shape[0], (cap + 3) & ~3), FILL, dtype=torch.uint8, device="cuda:0")
    return enc.encode_frames_device(d_frames, d_budgets, d_out=d_out)


def compare(cs, out, res, tag):
    """bytes up to the budget and the four result words, or quant_scale 64 over a zero row; nothing written past the budget"""
    bad = []
    for k, c in enumerate(cs):
        if c.res is None:
            ok = res[k].tolist() == [64, 0, 0, 0] and not out[k, :c.budget].any()
        else:
            n = c.stream.size
            ok = np.array_equal(res[k], c.res) and np.array_equal(out[k, :n], c.stream) and not out[k, n:c.budget].any()
        ok = ok and (out[k, c.budget:] == FILL).all()                 # "exactly frame_max_size bytes are written per frame"
        if not ok:
            bad.append(k)
    if bad:
        cat = H.catalogue()
        k = bad[0]
        c = cs[k]
        raise AssertionError("%s: %d of %d cases differ; first: row %d, '%s', budget %d, oracle scale %d, got %s" % (
            tag, len(bad), len(cs), k, cat[c.fi].name, c.budget, c.scale, res[k].tolist()))


def check_launch(torch, enc, up, cs, cap, tag):
    d_frames, d_budgets = up.rows(cs)
    d_out, d_res = launch(torch, enc, d_frames, d_budgets, cap)
    torch.cuda.synchronize()
    compare(cs, d_out.cpu().numpy(), d_res.cpu().numpy(), tag)


# ---------------------------------------------------------------- the guards: the run contains what it is meant to contain
@pytest.mark.parametrize("codec", [0, 1, 2])
def test_the_cases_contain_frames_on_which_first_fit_is_not_last_failure_plus_one(codec):
    """computed from the oracle's curves only.  Reachable by construction: 24 plainly tiled dip patterns with three budgets per
    scale give about six cases each where a fitting scale lies between two failing ones."""
    cs = cases(codec)
    differ, late, answers = guards(codec, cs)
    print("codec %d: %d cases, %d differ from last failure + 1, %d fit although scale 63 fails, %d distinct answers, %d fit nowhere"
          % (codec, len(cs), differ, late, answers, sum(c.scale == 64 for c in cs)))
    assert differ >= 100 and late >= 2 and answers >= 40, (differ, late, answers)
    assert any(c.scale == 64 for c in cs)
    cat = H.catalogue()
    sizes = {(cat[c.fi].w, cat[c.fi].h) for c in cs}
    assert {(320, 240), (192, 128), (48, 32)} <= sizes and ((640, 480) in sizes) == (codec == 1)
    big = {c.fi for c in cs if (cat[c.fi].w, cat[c.fi].h) == (320, 240)}
    assert sum(cat[fi].kind == "dip" for fi in big) >= 6 and sum(cat[fi].kind == "loose" for fi in big) == 2
    assert sum(cat[fi].kind == "ordinary" for fi in {c.fi for c in cs}) == 3
    dips = {s for fi in {c.fi for c in cs} for s in cat[fi].dips(codec)}          # (the split-kernel tests run every case)
    for b in H.BOUNDARIES:
        assert (b - 1 in dips or b in dips) and (b + 1 in dips or b + 2 in dips), (b, sorted(dips))


# ---------------------------------------------------------------- frame kernel
@pytest.mark.parametrize("codec", [0, 1, 2])
def test_frame_kernel_at_every_threshold(torch_cuda, codec):
    """each frame replicated once per threshold budget, budgets in a device tensor, one launch per size and context shape"""
    torch = torch_cuda
    t0 = time.time()
    n = 0
    for (w, h, cap), cs in sorted(groups(codec).items()):
        enc = encoder(codec, w, h, cap, SPLIT_ON if len(cs) > 12 else SPLIT_OFF)      # (launches of up to 12 frames take the split kernel)
        check_launch(torch, enc, Uploaded(torch, cs), cs, cap, "codec %d %dx%d cap %d" % (codec, w, h, cap))
        assert enc.watchdog() == 0
        enc.close()
        n += len(cs)
    assert n == len(cases(codec))
    print("codec %d: %d cases in %.1f s (oracle side included on first use)" % (codec, n, time.time() - t0))


@pytest.mark.parametrize("mode", ["default", "impatient", "off"])
@pytest.mark.parametrize("codec", [0, 1, 2])
def test_frame_kernel_at_scale_shuffled_launch_after_launch(torch_cuda, monkeypatch, codec, mode):
    """every size and context shape, each group of cases replicated to at least 1400 rows and shuffled so that neighbours differ in
    content and budget (the previous frame's answer is the next one's hint: mostly a wrong one here), four launches back to back on
    one context, under the three settings of the retry queue (a frame handed on restarts from a bare (frame, scale) and loses its
    search state); again with two launch lanes"""
    torch = torch_cuda
    monkeypatch.delenv("PSXHIP_MDEC_NO_RETRY_QUEUE", raising=False)
    monkeypatch.delenv("PSXHIP_MDEC_QUEUE_PATIENCE", raising=False)
    if mode == "impatient":
        monkeypatch.setenv("PSXHIP_MDEC_QUEUE_PATIENCE", "0")
    elif mode == "off":
        monkeypatch.setenv("PSXHIP_MDEC_NO_RETRY_QUEUE", "1")
    rng = np.random.default_rng(1400 + codec)
    for (w, h, cap), cs in sorted(groups(codec).items()):
        rows = [c for _ in range(-(-1400 // len(cs))) for c in cs]
        rows = [rows[i] for i in rng.permutation(len(rows))]
        assert len(rows) >= 1400
        up = Uploaded(torch, rows)
        d_frames, d_budgets = up.rows(rows)
        for lanes in (1, 2):
            enc = encoder(codec, w, h, cap)
            if lanes > 1:
                enc.set_lanes(2)
            outs = [launch(torch, enc, d_frames, d_budgets, cap) for _ in range(4)]
            enc.fence()
            torch.cuda.synchronize()
            for r, (o, q) in enumerate(outs):
                compare(rows, o.cpu().numpy(), q.cpu().numpy(), "codec %d %dx%d cap %d %s lanes %d launch %d" % (codec, w, h, cap, mode, lanes, r))
            assert enc.watchdog() == 0
            enc.close()


# ---------------------------------------------------------------- split kernel
@pytest.mark.parametrize("codec", [0, 1, 2])
def test_split_kernel_launches_of_1_2_5_12_frames(torch_cuda, codec):
    """every case again in launches of 1, 2, 5 and 12 frames with per-frame budgets: the split kernel (rounds of sixteen scales; a
    dip at 8, 16 or 32 has its fitting scale in one round and the failing one above it in the next), against the oracle and
    against the frame kernel (the same library with PSXHIP_MDEC_SPLIT_MAX=0) on the same launches"""
    torch = torch_cuda
    rng = np.random.default_rng(12 + codec)
    for (w, h, cap), cs in sorted(groups(codec).items()):
        cs = [cs[i] for i in rng.permutation(len(cs))]
        up = Uploaded(torch, cs)
        for env, name in ((SPLIT_ON, "split"), (SPLIT_OFF, "frame kernel")):
            enc = encoder(codec, w, h, cap, env)
            at, k, outs = 0, 0, []
            while at < len(cs):
                n = (1, 2, 5, 12)[k % 4]
                part = cs[at:at + n]
                d_frames, d_budgets = up.rows(part)
                outs.append((part, launch(torch, enc, d_frames, d_budgets, cap)))
                at += n
                k += 1
                if k % 64 == 0 or at >= len(cs):                      # (bounds the rows held on the device)
                    torch.cuda.synchronize()
                    for part, (o, q) in outs:
                        compare(part, o.cpu().numpy(), q.cpu().numpy(), "codec %d %dx%d cap %d %s, launch of %d" % (codec, w, h, cap, name, len(part)))
                    outs = []
            assert enc.watchdog() == 0
            enc.close()


def _answer_to_budget(codec, fi):
    """answer -> a case that gives it: of frame fi where it has one, else of another frame of the same size (scale s + 1 is never
    the first fit of a frame that needs more bytes there than at s)"""
    cat = H.catalogue()
    m, other = {}, {}
    for c in cases(codec):
        if c.scale < 64:
            if c.fi == fi:
                m.setdefault(c.scale, c)
            elif (cat[c.fi].w, cat[c.fi].h) == (cat[fi].w, cat[fi].h):
                other.setdefault(c.scale, c)
    return {**other, **m}


def _one_frame_calls(enc, calls, tag):
    """encode_frame_bs, the reference's call (one frame, frame_max_size poked by the caller), case after case"""
    cat = H.catalogue()
    for k, c in enumerate(calls):
        enc.frame_max_size = c.budget
        out = enc.encode_frame_bs(cat[c.fi].frame)
        got = np.array([enc.quant_scale, enc.bytes_used, enc.blocks_used, enc.uncomp_hwords_used], np.int32)
        n = c.stream.size
        assert np.array_equal(got, c.res), (tag, k, cat[c.fi].name, c.budget, got.tolist(), c.res.tolist())
        assert np.array_equal(out[:n], c.stream) and not out[n:c.budget].any(), (tag, k, cat[c.fi].name, c.budget)


@pytest.mark.parametrize("codec", [0, 1, 2])
def test_one_frame_calls_starting_next_to_a_dip(torch_cuda, codec):
    """encode_frame_bs in sequences where the call before a dip case (budget need[s]: s fits, s + 1 does not) left as its answer --
    the split kernel's starting point for the next call, whatever the budgets -- (a) the dip case's own answer, (b) s + 1, s + 2,
    s + 3, each counted on its own, (c) one below the answer, (d) a scale <= 6 before an answer above 8: the short first round of eight
    scales, after which the rounds end at 8, 24, 40 and 56 instead of 16, 32 and 48.  The call before is the same frame -- or, for scales it never answers, another of its size -- at the
    budget of its own that answers the wanted scale.  The frame kernel (PSXHIP_MDEC_SPLIT_MAX=0) runs the same sequences as a second
    reference only: it takes a hint for the budget it was found at, and the two calls differ in budget
    (test_frame_kernel_from_a_chosen_hint is its test)."""
    cat = H.catalogue()
    seqs = []
    kinds = {"a": 0, "b1": 0, "b2": 0, "b3": 0, "c": 0, "d": 0}
    sides, short_sides = set(), set()
    for fi, f in enumerate(cat):
        if codec not in f.codecs or f.kind != "dip" or f.w > 320:
            continue
        by_answer = _answer_to_budget(codec, fi)
        need = f.need(codec)
        for s in f.dips(codec):
            dip = next(c for c in cases(codec) if c.fi == fi and c.budget == int(need[s]))
            a = dip.scale                                             # (below s where a finer scale fits this budget too)
            assert a <= s and need[s + 1] > dip.budget
            for before, kind in ((a, "a"), (s + 1, "b1"), (s + 2, "b2"), (s + 3, "b3"), (a - 1, "c")):
                if before in by_answer:
                    seqs.append((f, [by_answer[before], dip]))
                    kinds[kind] += 1
            if a > 8:
                for low in (2, 6):
                    if low in by_answer:
                        seqs.append((f, [by_answer[low], dip]))
                        kinds["d"] += 1
                        short_sides.add(s)
            sides.add(s)
    assert min(kinds.values()) >= 10, kinds
    for b in H.BOUNDARIES:
        assert (b - 1 in sides or b in sides) and (b + 1 in sides or b + 2 in sides), sorted(sides)
    for b in (24, 40):                                                # round ends after a short first round that the catalogue has dips at
        assert (b - 1 in short_sides or b in short_sides) and (b + 1 in short_sides or b + 2 in short_sides), sorted(short_sides)
    print("codec %d: %d sequences %s" % (codec, len(seqs), kinds))
    for env, name in ((SPLIT_ON, "split"), (SPLIT_OFF, "frame kernel")):
        encs = {}
        for f, calls in seqs:
            key = (f.w, f.h)
            if key not in encs:
                encs[key] = encoder(codec, f.w, f.h, max(c.budget for g, cc in seqs if (g.w, g.h) == key for c in cc), env)
            _one_frame_calls(encs[key], calls, "codec %d %s" % (codec, name))
        for e in encs.values():
            assert e.watchdog() == 0
            e.close()


# ---------------------------------------------------------------- frame kernel from a chosen hint
def hint_pairs(codec):
    """[(frame, frame index, budget need[s], hint h, dip s, the frame to encode first: the oracle answers h for it at that budget)]
    for every dip of every dip frame (all sizes) and h = s - 1 .. s + 3 and 63, and the (frame name, s, h) no frame was found for"""
    cat = H.catalogue()
    want = []
    for fi, f in enumerate(cat):
        if codec in f.codecs and f.kind == "dip":
            need = f.need(codec)
            for s in f.dips(codec):
                b = int(need[s])                                      # (the answer is s, or below it where a finer scale needs no more)
                want += [(f, fi, b, h, s) for h in sorted({s - 1, s, s + 1, s + 2, s + 3, 63}) if 1 <= h <= 63]
    O.lib().orc_mdec_ac_code(0, 1)
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        found = list(ex.map(lambda t: H.frame_answering(codec, t[0].w, t[0].h, t[2], t[3]), want))
    pairs = [t + (fr,) for t, fr in zip(want, found) if fr is not None]
    return pairs, [t for t, fr in zip(want, found) if fr is None]


@pytest.mark.parametrize("codec", [0, 1, 2])
def test_frame_kernel_from_a_chosen_hint(torch_cuda, codec):
    """On a context with the split kernel off a one-frame call goes through the frame kernel and takes the answer of the call before
    it, at the same budget, as its first guess (PSXHIP_MDEC_TRUST=1: always -- the default policy stops trusting such hints once most of
    them were wrong, as they are here on purpose).  For each dip (s fits, s + 1 does not, budget need[s]) of every dip frame, all
    sizes: a call whose oracle answer AT THAT BUDGET is h, then the dip frame, for h = s - 1, s, s + 1, s + 2, s + 3 and 63.
    h = s + 2 is the sharp one: the first pass counts s + 1 and emits s + 2, both fail, and only a valid bound keeps scale s open.
    The frame before is synthetic noise whose amplitude is searched with the oracle until it answers h; every pair must exist, but
    for h = 63 where the oracle shows that not even full-range noise needs scale 63 at that budget.  The per-frame record
    (PSXHIP_MDEC_STATS=1) must show the hint as the first guess, and two passes at least wherever the hint is not the answer (which is s,
    or a scale below it that needs no more bytes)."""
    from psxavenc_amd import _lib
    pairs, missing = hint_pairs(codec)
    for f, fi, b, h, s in missing:
        assert h == 63 and H.loudest_answer(codec, f.w, f.h, b) < 63, (f.name, s, h)
    print("codec %d: %d (dip, hint) pairs; no noise answers 63 for: %s" % (codec, len(pairs), [(f.name, s) for f, fi, b, h, s in missing]))
    sizes = {(p[0].w, p[0].h) for p in pairs}
    assert {(320, 240), (192, 128), (48, 32)} <= sizes and ((640, 480) in sizes) == (codec == 1)
    assert sum(p[3] == 63 and p[4] < 58 for p in pairs) >= 10 and sum(p[3] == p[4] + 2 for p in pairs) >= 25
    todo = [(H.Frame("before", f.w, f.h, before, "hint"), -1, b) for f, fi, b, h, s, before in pairs]
    befores = _oracle_many(codec, todo)
    dips = {(c.fi, c.budget): c for c in cases(codec)}
    NT = 8 + 4 * 1024 + 16 + 2048
    encs, passes = {}, []
    for (f, fi, b, h, s, before), cb in zip(pairs, befores):
        assert cb.scale == h
        key = (f.w, f.h)
        if key not in encs:
            cap = max(SMALL_CAP, max(p[2] for p in pairs if (p[0].w, p[0].h) == key))
            encs[key] = encoder(codec, f.w, f.h, cap, dict(SPLIT_OFF, PSXHIP_MDEC_STATS="1", PSXHIP_MDEC_TRUST="1"))
        enc = encs[key]
        for frame, c in ((before, cb), (f.frame, dips[(fi, b)])):
            out, res = enc.encode_frames_host(frame[None, :], b)
            n = c.stream.size
            assert np.array_equal(res[0], c.res), (f.name, b, h, res[0].tolist(), c.res.tolist())
            assert np.array_equal(out[0, :n], c.stream) and not out[0, n:b].any(), (f.name, b, h)
        t = (C.c_ulonglong * NT)()
        _lib.check(_lib.lib().psxhip_mdec_read_stats(enc._h, t, NT, 0))
        rec = int(t[8 + 4 * 1024 + 16])
        guess, answer, npass = rec & 0xFF, (rec >> 16) & 0xFF, (rec >> 24) & 0xFF
        a = dips[(fi, b)].scale
        assert a <= s and guess == h and answer == a, (f.name, b, h, s, a, guess, answer, npass)
        assert npass >= (1 if h == a else 2), (f.name, b, h, s, a, npass)
        passes.append(npass)
    for e in encs.values():
        assert e.watchdog() == 0
        e.close()
    print("codec %d: passes per dip case: max %d, mean %.2f" % (codec, max(passes), float(np.mean(passes))))


# ---------------------------------------------------------------- nothing fits / fits late
@pytest.mark.parametrize("codec", [0, 1, 2])
def test_nothing_fits_and_fits_only_below_a_failing_scale_63(torch_cuda, codec):
    """Budget min(need) - 2: no scale fits -- quant_scale 64 over a zero row from the device entry point, PSXHIP_ENOFIT from the
    host one, from both kernels.  A budget scale 63 fails but a finer scale fits (dips at the top of the range): that finer scale."""
    from psxavenc_amd import _lib
    torch = torch_cuda
    cat = H.catalogue()
    todo, late = [], 0
    for fi, f in enumerate(cat):
        if codec not in f.codecs:
            continue
        need = f.need(codec)
        todo.append((f, fi, int(need[1:].min()) - 2))
        for s in range(1, 63):
            b = int(need[s])
            if need[63] > b and H.first_fit(need, b) == s:
                todo.append((f, fi, b))
                late += 1
    assert late >= 2
    cs = _oracle_many(codec, todo)
    nofit = [c for c in cs if c.scale == 64]
    assert len(nofit) == len({c.fi for c in cs}) and len(cs) - len(nofit) == late
    by = {}
    for c in cs:
        by.setdefault((cat[c.fi].w, cat[c.fi].h), []).append(c)
    for (w, h), part in sorted(by.items()):
        cap = max(SMALL_CAP, max(c.budget for c in part))
        up = Uploaded(torch, part)
        for env, name in ((SPLIT_ON, "default"), (SPLIT_OFF, "frame kernel")):
            enc = encoder(codec, w, h, cap, env)
            check_launch(torch, enc, up, part, cap, "codec %d %dx%d %s, one launch" % (codec, w, h, name))
            for c in part:                                            # one frame per launch: the split kernel unless it is off
                check_launch(torch, enc, up, [c], cap, "codec %d %dx%d %s, one frame" % (codec, w, h, name))
                if c.scale == 64:
                    with pytest.raises(_lib.PsxHipError) as e:
                        enc.encode_frames_host(cat[c.fi].frame[None, :], c.budget)
                    assert e.value.code == _lib.PSXHIP_ENOFIT
                else:
                    out, res = enc.encode_frames_host(cat[c.fi].frame[None, :], c.budget)
                    assert np.array_equal(res[0], c.res) and np.array_equal(out[0, :c.stream.size], c.stream), (cat[c.fi].name, c.budget)
            assert enc.watchdog() == 0
            enc.close()


# ---------------------------------------------------------------- the cases reach the second pass
def test_dip_cases_reach_the_second_pass(torch_cuda):
    """PSXHIP_MDEC_STATS=1 on one launch of the shuffled 320x240 cases: the per-frame records (first guess | answer << 16 | passes << 24)
    show dip cases that took two passes and more"""
    from psxavenc_amd import _lib
    torch = torch_cuda
    cat = H.catalogue()
    (w, h, cap), cs = max(groups(0, {(320, 240)}).items(), key=lambda kv: len(kv[1]))
    rng = np.random.default_rng(5)
    cs = [cs[i] for i in rng.permutation(len(cs))][:2048]
    enc = encoder(0, w, h, cap, {"PSXHIP_MDEC_STATS": "1"})
    check_launch(torch, enc, Uploaded(torch, cs), cs, cap, "stats launch")
    NT = 8 + 4 * 1024 + 16 + 2048
    t = (C.c_ulonglong * NT)()
    _lib.check(_lib.lib().psxhip_mdec_read_stats(enc._h, t, NT, 1))
    rec = np.array(list(t)[8 + 4 * 1024 + 16:8 + 4 * 1024 + 16 + len(cs)], dtype=np.uint64)
    answer, passes = ((rec >> 16) & 0xFF).astype(int), ((rec >> 24) & 0xFF).astype(int)
    assert enc.watchdog() == 0
    enc.close()
    fits = np.array([c.scale < 64 for c in cs])
    assert np.array_equal(answer[fits], np.array([c.scale for c in cs])[fits])
    dip = np.array([cat[c.fi].kind == "dip" and c.scale < 64 for c in cs])
    print("passes over %d dip cases: max %d, mean %.2f, histogram %s" % (dip.sum(), passes[dip].max(), passes[dip].mean(),
                                                                        np.bincount(passes[dip]).tolist()))
    assert passes[dip].max() >= 2
