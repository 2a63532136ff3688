"""The v2 frame kernel's sampled count (mdec-k3.9): a pass that counts at p - 1 and emits at p stops counting at its quarter-pass
checkpoint when the sample says the MIXED bound -- AC bits minus deficit at p - 1 over the macroblocks counted so far, at p over the
rest (csrc/mdec_search.h, mdec_search_note_bound; tests/test_mdec_mixed_bound.py for the bound itself) -- will prove "no scale
<= p - 1 fits" anyway.  Whatever the judge decides, the answer and the bytes are the reference's: every case here is compared with
the CPU oracle, byte for byte and result word for result word.

What the judge decides is read from the diagnostics instantiation (PSXHIP_MDEC_STATS=1): bit 15 of a frame's record says that its
last pass stopped counting, bits 24.. its passes, bits 32.. the scales of its first four passes (| 0x40: a pass that only counts).
What it SHOULD decide is worked out here from the oracle's coefficients, the generated tables and the pass order the library
hands out (psxhip_mdec_pass_order): the tickets before the mark are the sample.  The cases are chosen with that model so that the
judge's projection is at least one standard error away from the kernel's own threshold of two, on the expected side (the model
computes the very sums the judge reads: the distance only has to cover rounding).

Geometry: 256x128 (128 macroblocks) is the smallest frame whose passes have a checkpoint in both workgroup shapes; a launch of 32
frames runs the 16-wavefront shape, one of 600 the 12-wavefront shape; 320x240 rides along with 64 frames."""
import ctypes as C
import os

import numpy as np
import pytest

import mdec_hard_content as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

CAP = 8192
FILL = 0xAB
NT = 8 + 4 * 1024 + 16 + 2048
FRAME0 = 8 + 4 * 1024 + 16
RATIOS = (1.02, 1.10, 1.3, 1.7)              # need(p - 1) / limit
STOP_BIT = 1 << 15


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---------------------------------------------------------------- the judge, from the oracle's side
def mb_curves(w, h, frame):
    """per macroblock in RASTER order (the oracle hands the coefficients out as (6, macroblocks, 64)) and scale: AC bits, deficits"""
    tb, df = H.block_curves(H.frame_blocks(w, h, frame))
    nmb = (w // 16) * (h // 16)
    return tb.reshape(6, nmb, 64).sum(axis=0), df.reshape(6, nmb, 64).sum(axis=0)


def sample_of(w, h, large):
    """raster indices of the macroblocks of the tickets before the checkpoint's mark, or None when the passes have no checkpoint"""
    from psxavenc_amd import _lib
    L = _lib.lib()
    L.psxhip_mdec_pass_order.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_int]
    L.psxhip_mdec_pass_order.restype = C.c_int
    n = L.psxhip_mdec_pass_order(w, h, large, None, 0)
    buf = (C.c_uint32 * n)()
    assert L.psxhip_mdec_pass_order(w, h, large, buf, n) == n
    o = np.frombuffer(buf, dtype=np.uint32)
    waves = 16 if large else 12
    trips = n // waves
    if trips < 8:
        return None
    q = o[:(trips >> 2) * waves]
    q = q[q != 0xFFFF].astype(np.int64)
    return (q >> 8) * (w // 16) + (q & 0xFF)


class Judge:
    """what the checkpoint's judge sees of a (p - 1, p) pass over a frame at a budget, in bits"""
    def __init__(self, tb, df, sample, p, budget, held=0):
        nmb, n = tb.shape[0], len(sample)
        g = tb - df
        self.limit = 16 * ((budget - 8) >> 1)
        fixed = 72 * nmb + 10                                             # v2: 10-bit DC and 2-bit end of block x 6, end of frame
        self.projected = fixed + int(g[sample, p - 1].sum()) + int(g[sample, p].sum()) * (nmb - n) // n
        x = ((tb[sample, p] + 72) >> 2).astype(np.float64)
        self.se = 4.0 * np.sqrt(max(x.var(), 0.0) * n * (1.0 - n / nmb)) * (nmb / n)
        self.emit_projected = int((tb[sample, p] + 72).sum()) * nmb // n + 10
        rest = np.setdiff1d(np.arange(nmb), sample)
        # the bound the pass ends with: the sample counted, the rest not -- but for the (at most `held`) macroblocks the wavefronts
        # were already in when the flag came; the worst case for "the bound fails" is that those were the ones that gain most
        gain = np.sort(g[rest, p - 1] - g[rest, p])[::-1]
        self.bound_low = fixed + int(g[sample, p - 1].sum()) + int(g[rest, p].sum())
        self.bound_high = self.bound_low + int(np.maximum(gain[:held], 0).sum())
        self.exact = fixed + int(g[:, p - 1].sum())                       # what an exact count of p - 1 proves for the scales below

    def margin(self):
        """how far the projection clears the limit, in standard errors (the kernel stops counting above 2)"""
        return (self.projected - self.limit) / max(self.se, 1.0)


# ---------------------------------------------------------------- cases
class Row:
    def __init__(self, name, w, h, frame, budget, kind, p=None):
        self.name, self.w, self.h, self.frame, self.budget, self.kind, self.p = name, w, h, frame, int(budget), kind, p
        out, res, rc = O.mdec_encode(0, w, h, frame[None, :], int(budget))
        assert rc in (0, -2), rc
        self.res = res[0].copy() if rc == 0 else None
        self.stream = out[0, :int(res[0, 1])].copy() if rc == 0 else None
        self.scale = int(res[0, 0]) if rc == 0 else 64


def ratio_rows(w, h, large, n_frames, seed):
    """per noise frame and ratio r a budget with need(p - 1) = r x budget and answer p; among the scales that allow it the one
    where the judge (of this workgroup shape: its sample) is surest of the expected decision (for 1.3 nothing is expected: the
    first that allows it).  Frames on which a decision is a close call are passed over: the first n_frames of the generator's
    sequence on which none is."""
    rows = []
    sample = sample_of(w, h, large)
    frames = O.synth_frames(w, h, 4 * n_frames, seed=seed, amp=4)
    kept = 0
    for k in range(4 * n_frames):
        need = O.mdec_need(0, w, h, frames[k])
        tb, df = mb_curves(w, h, frames[k])
        mine = []
        for r in RATIOS:
            best = None
            for p in range(2, 40):
                b = int(need[p - 1] / r) & ~1
                if not (8 < b <= CAP and need[p] <= b < need[p - 1] and H.first_fit(need, b) == p):
                    continue
                m = Judge(tb, df, sample, p, b).margin()
                score = m - 2.0 if r >= 1.5 else 2.0 - m
                if best is None or (score > best[0] and r != 1.3):
                    best = (score, p, b)
            if best is None or (r != 1.3 and best[0] < 1.0):          # the judge's decision would be a close call
                break
            mine.append((r, best[1], best[2]))
        if len(mine) < len(RATIOS):
            continue
        for r, p, b in mine:
            rows.append(Row("noise +-4 %dx%d #%d need(p-1) = %.2f x limit" % (w, h, k, r), w, h, frames[k], b, r, p))
            assert rows[-1].scale == p
        kept += 1
        if kept == n_frames:
            return rows
    raise AssertionError("only %d of %d frames give the judge four clear cases at %dx%d" % (kept, 4 * n_frames, w, h))


def _paste(dst, src, w, h, mbs):
    """the macroblocks `mbs` (raster indices) of NV21 frame src over dst"""
    out = dst.copy()
    nx = w // 16
    lo, ls = out[:w * h].reshape(h, w), src[:w * h].reshape(h, w)
    co, cs = out[w * h:].reshape(h // 2, w), src[w * h:].reshape(h // 2, w)
    for m in mbs:
        fy, fx = divmod(int(m), nx)
        lo[fy * 16:fy * 16 + 16, fx * 16:fx * 16 + 16] = ls[fy * 16:fy * 16 + 16, fx * 16:fx * 16 + 16]
        co[fy * 8:fy * 8 + 8, fx * 16:fx * 16 + 16] = cs[fy * 8:fy * 8 + 8, fx * 16:fx * 16 + 16]
    return out


def fooled_row(w, h, large, seed=11):
    """A frame that is busier on the macroblocks of the tickets before the mark than elsewhere, at the budget one word short of
    need(p - 1) or a little less (so that an exact count of p - 1 proves the scales below it): the sample says the mixed bound will clear the limit (by three standard errors and more), the emit projection stays
    under the limit (the pass is not stopped), and the bound the pass ends with cannot prove p - 1 -- whichever macroblocks the
    wavefronts were in when the flag came.  Searched over a few pairs of noise amplitudes."""
    sample = sample_of(w, h, large)
    waves = 16 if large else 12
    for quiet, busy in ((4, 6), (4, 5), (6, 8), (3, 5), (8, 10), (5, 6), (8, 12), (3, 4)):
        fq = O.synth_frames(w, h, 1, seed=seed, amp=quiet)[0]
        fb = O.synth_frames(w, h, 1, seed=seed, amp=busy)[0]
        f = _paste(fq, fb, w, h, sample)
        need = O.mdec_need(0, w, h, f)
        tb, df = mb_curves(w, h, f)
        for p in range(2, 12):
          # (from one word short of need(p - 1) downwards: the first budget at which an exact count of p - 1 proves everything
          #  below it too, deficits and all -- the pass after the failed bound is then the frame's last)
          for b in range(int(need[p - 1]) - 2, int(need[p]) - 1, -2):
            if not (8 < b <= CAP and H.first_fit(need, b) == p):
                continue
            j = Judge(tb, df, sample, p, b, held=3 * waves)
            if j.exact <= j.limit:
                continue
            if j.margin() >= 3.0 and j.emit_projected <= j.limit and j.bound_high <= j.limit:
                return Row("busy before the mark (+-%d in +-%d) %dx%d %s" % (busy, quiet, w, h, "16" if large else "12"), w, h, f, b, "fooled", p)
    raise AssertionError("no frame fools the judge at %dx%d" % (w, h))


def reverse_row(w, h, large, seed=12):
    """the reverse: quiet before the mark, busy elsewhere, one word short of need(p - 1): the sample never promises the proof"""
    sample = sample_of(w, h, large)
    fq = O.synth_frames(w, h, 1, seed=seed, amp=3)[0]
    fb = O.synth_frames(w, h, 1, seed=seed, amp=6)[0]
    f = _paste(fb, fq, w, h, sample)
    need = O.mdec_need(0, w, h, f)
    tb, df = mb_curves(w, h, f)
    for p in range(2, 12):
        b = int(need[p - 1]) - 2
        if 8 < b <= CAP and H.first_fit(need, b) == p and Judge(tb, df, sample, p, b).margin() <= 1.0:
            return Row("quiet before the mark %dx%d %s" % (w, h, "16" if large else "12"), w, h, f, b, "reverse", p)
    raise AssertionError("no reverse frame at %dx%d" % (w, h))


_shared = {}


def shared(key, make):
    if key not in _shared:
        _shared[key] = make()
    return _shared[key]


# ---------------------------------------------------------------- launches
def encoder(w, h, env):
    from psxavenc_amd.mdec import MdecEncoder
    env = dict(env, PSXHIP_MDEC_SPLIT_MAX="0")
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return MdecEncoder(0, w, h, max_frame_size=CAP, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def shape_of(torch, n_frames):
    """1: a launch of this many frames runs the 16-wavefront shape (the host's rule: no more frames than the device has compute
    units, so that every frame gets a CU of its own), 0: the 12-wavefront shape -- the judge's sample is the shape's"""
    return 1 if n_frames <= torch.cuda.get_device_properties(0).multi_processor_count else 0


def run(torch, enc, rows, launches=1):
    """the rows as one launch (per-frame budgets in a device tensor), `launches` times; returns the last launch's (bytes, results)"""
    d_frames = torch.from_numpy(np.stack([r.frame for r in rows])).to("cuda:0")
    d_budgets = torch.tensor([r.budget for r in rows], dtype=torch.int32, device="cuda:0")
    outs = []
    for _ in range(launches):
        d_out = torch.full((len(rows), CAP), FILL, dtype=torch.uint8, device="cuda:0")
        outs.append(enc.encode_frames_device(d_frames, d_budgets, d_out=d_out))
    enc.fence()
    torch.cuda.synchronize()
    return [(o.cpu().numpy(), q.cpu().numpy()) for o, q in outs]


def compare(rows, out, res, tag):
    bad = []
    for k, r in enumerate(rows):
        if r.res is None:
            ok = res[k].tolist() == [64, 0, 0, 0] and not out[k, :r.budget].any()
        else:
            n = r.stream.size
            ok = np.array_equal(res[k], r.res) and np.array_equal(out[k, :n], r.stream) and not out[k, n:r.budget].any()
        if not (ok and (out[k, r.budget:] == FILL).all()):
            bad.append(k)
    assert not bad, "%s: %d of %d rows differ from the oracle; first: row %d, '%s', budget %d, oracle scale %d, got %s" % (
        tag, len(bad), len(rows), bad[0], rows[bad[0]].name, rows[bad[0]].budget, rows[bad[0]].scale, res[bad[0]].tolist())


def records(enc, n):
    from psxavenc_amd import _lib
    t = (C.c_ulonglong * NT)()
    _lib.check(_lib.lib().psxhip_mdec_read_stats(enc._h, t, NT, 1))
    return np.array(list(t)[FRAME0:FRAME0 + n], dtype=np.uint64)


def fields(rec):
    rec = rec.astype(np.int64)
    trace = np.stack([(rec >> (32 + 8 * k)) & 0xFF for k in range(4)], axis=1)
    return rec & 0xFF, (rec & STOP_BIT) != 0, (rec >> 16) & 0xFF, (rec >> 24) & 0xFF, trace


# ---------------------------------------------------------------- four budgets per frame
@pytest.mark.parametrize("w,h,n", [(256, 128, 32), (256, 128, 600), (320, 240, 64)])
def test_counting_stops_where_the_bound_will_do_and_only_there(torch_cuda, w, h, n):
    large = shape_of(torch_cuda, n)
    base = shared(("ratio", w, h, large), lambda: ratio_rows(w, h, large, 8 if w == 256 else 4, seed=40 + w))
    rng = np.random.default_rng(n)
    rows = [base[i] for i in rng.permutation(np.arange(n) % len(base))]
    assert n <= 2048
    enc = encoder(w, h, {"PSXHIP_MDEC_STATS": "1"})
    (out, res), = run(torch_cuda, enc, rows)
    rec = records(enc, n)
    assert enc.watchdog() == 0
    enc.close()
    compare(rows, out, res, "%dx%d, %d frames" % (w, h, n))
    guess, stopped, answer, passes, _ = fields(rec)
    want = np.array([r.scale for r in rows])
    kind = np.array([r.kind for r in rows])
    assert np.array_equal(answer, want)
    for r in RATIOS:
        m = kind == r
        print("%dx%d x %d, need(p-1) = %.2f x limit: %d rows, counting stopped in the last pass of %d, passes per frame %.2f, first guess right on %d"
              % (w, h, n, r, m.sum(), stopped[m].sum(), passes[m].mean(), (guess[m] == want[m]).sum()))
    assert not stopped[(kind == 1.02) | (kind == 1.10)].any()
    far = kind == 1.7
    assert stopped[far].all()
    first_try = far & (guess == want)
    assert first_try.sum() * 2 >= far.sum(), (first_try.sum(), far.sum())      # (the pilot is right on noise more often than not)
    assert (passes[first_try] == 1).all()


@pytest.mark.parametrize("n", [32, 600])
def test_a_warm_launch_far_over_the_limit_takes_one_pass_per_frame(torch_cuda, n):
    """need(p - 1) = 1.7 x limit on every frame of the launch (one frame, one budget), the second launch on the context: every
    frame starts from the answer (PSXHIP_MDEC_TRUST=1: the previous launch's and the neighbour's answers are always taken), stops
    counting at the mark and is done in one pass"""
    w, h = 256, 128
    large = shape_of(torch_cuda, n)
    base = shared(("ratio", w, h, large), lambda: ratio_rows(w, h, large, 8, seed=40 + w))
    row = [r for r in base if r.kind == 1.7][0]
    rows = [row] * n
    enc = encoder(w, h, {"PSXHIP_MDEC_STATS": "1", "PSXHIP_MDEC_TRUST": "1"})
    run(torch_cuda, enc, rows)
    records(enc, n)
    (out, res), = run(torch_cuda, enc, rows)
    rec = records(enc, n)
    assert enc.watchdog() == 0
    enc.close()
    compare(rows, out, res, "%s, %d frames, second launch" % (row.name, n))
    guess, stopped, answer, passes, _ = fields(rec)
    print("%s x %d, warm: first guess right on %d, passes %s, counting stopped on %d" % (row.name, n, (guess == row.p).sum(), np.bincount(passes).tolist(), stopped.sum()))
    assert (answer == row.p).all() and (guess == row.p).all()
    assert stopped.all() and (passes == 1).all()


# ---------------------------------------------------------------- the judge fooled
@pytest.mark.parametrize("n", [32, 600])
def test_a_fooled_judge_costs_a_pass_and_nothing_else(torch_cuda, n):
    """every frame of the launch is the frame that is busy before the mark (of this launch's shape), then the reverse; the second
    launch on the context starts from the first one's answer (PSXHIP_MDEC_TRUST=1: such hints are always taken), so its first pass is
    (p - 1, p): emit p -- fits -- and a bound that cannot prove p - 1, then a pass that only counts p - 1"""
    large = shape_of(torch_cuda, n)
    w, h = 256, 128
    for make, tag in ((fooled_row, "fooled"), (reverse_row, "reverse")):
        row = shared((tag, w, h, large), lambda: make(w, h, large))
        rows = [row] * n
        enc = encoder(w, h, {"PSXHIP_MDEC_STATS": "1", "PSXHIP_MDEC_TRUST": "1"})
        run(torch_cuda, enc, rows)
        records(enc, n)
        (out, res), = run(torch_cuda, enc, rows)
        rec = records(enc, n)
        assert enc.watchdog() == 0
        enc.close()
        compare(rows, out, res, "%s, %d frames" % (row.name, n))
        guess, stopped, answer, passes, trace = fields(rec)
        p = row.p
        assert (answer == p).all()
        hinted = guess == p
        print("%s: answer %d, first guess right on %d of %d, passes %s, last pass stopped counting on %d"
              % (row.name, p, hinted.sum(), n, np.bincount(passes).tolist(), stopped.sum()))
        assert hinted.sum() * 4 >= 3 * n
        assert not stopped.any()                        # fooled: the last pass only counts; reverse: the judge never stops the count
        if tag == "fooled":
            assert (passes[hinted] == 2).all()
            assert (trace[hinted, 0] == p).all() and (trace[hinted, 1] == ((p - 1) | 0x40)).all(), trace[hinted][:4]
        # (the reverse: nothing is asked of its passes -- a sample that quiet makes the checkpoint stop the pass for a finer guess, as
        #  it always has; what is asked is that the judge never takes the count away, and the oracle's bytes)


# ---------------------------------------------------------------- hard content, everything in one launch
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("n", [200, 1400])
def test_hard_content_and_every_case_above_mixed_in_one_launch(torch_cuda, n, lanes):
    """the non-monotone 320x240 frames of tests/mdec_hard_content.py at their exact, one-byte-over and one-word-over budgets (the cases
    tests/test_gpu_mdec_thresholds.py keeps, with the oracle's bytes), shuffled together with the four-budget rows and the two frames
    made for this launch's judge: 200 rows run the 16-wavefront shape, 1400 the 12-wavefront shape"""
    import test_gpu_mdec_thresholds as T
    large = shape_of(torch_cuda, n)
    w, h = 320, 240
    cat = H.catalogue()
    (_, _, cap), cs = max(((k, v) for k, v in T.groups(0, {(w, h)}).items() if k[2] == CAP), key=lambda kv: len(kv[1]))
    hard = shared("hard", lambda: [_from_case(cat, c) for c in cs if cat[c.fi].kind in ("dip", "loose")])
    assert len(hard) >= 150 and sum(r.scale == 64 for r in hard) >= 1
    extra = shared(("ratio", w, h, large), lambda: ratio_rows(w, h, large, 4, seed=40 + w))
    extra = extra + [shared(("fooled", w, h, large), lambda: fooled_row(w, h, large)), shared(("reverse", w, h, large), lambda: reverse_row(w, h, large))]
    rng = np.random.default_rng(100 * n + lanes)
    pick = [hard[i % len(hard)] for i in rng.permutation(max(len(hard), n - n // 4))[:n - n // 4]]
    rows = pick + [extra[i % len(extra)] for i in range(n - len(pick))]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    enc = encoder(w, h, {})
    if lanes > 1:
        enc.set_lanes(2)
    for k, (out, res) in enumerate(run(torch_cuda, enc, rows, launches=2)):
        compare(rows, out, res, "hard content, %d rows, %d lane(s), launch %d" % (len(rows), lanes, k))
    assert enc.watchdog() == 0
    enc.close()


def _from_case(cat, c):
    r = Row.__new__(Row)
    f = cat[c.fi]
    r.name, r.w, r.h, r.frame, r.budget, r.kind, r.p = f.name, f.w, f.h, f.frame, c.budget, "hard", None
    r.res, r.stream, r.scale = c.res, c.stream, c.scale
    return r
