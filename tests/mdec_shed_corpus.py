"""The corpus of the MDEC shed tests (tests/test_mdec_shed_ref.py, test_mdec_shed_core_cpu.py, test_gpu_mdec_shed.py): groups of frames
that one encoder context takes -- a codec, a frame size, the frames and their budgets -- and what the statement
(tests/mdec_shed_ref.py) says of every frame for K = 1, 2 and 3.  Not a conftest and not a test.

Content: oracle_lib.synth_frames at several amplitudes, some with uniform noise on top.  Budgets are drawn from the oracle's need curve (oracle_lib.mdec_need): a target scale N and a share `alpha` of
the gap between need[N] and need[N - 1] -- a budget just above need[N] wants much shed, one just below need[N - 1] little.  alpha
None: N = 1 (everything fits); "tiny": 8 bytes, which nothing fits (N = 64).
"""
import functools

import numpy as np

import mdec_shed_ref as S
import oracle_lib as O

KS = (1, 2, 3)


class Group:
    def __init__(self, name, codec, w, h, frames, budgets, uniform):
        self.name, self.codec, self.w, self.h = name, codec, w, h
        self.frames = frames                         # (n, w * h * 3 / 2) uint8
        self.budgets = budgets                       # (n,) int32
        self.uniform = uniform                       # the one budget of a call without a per-frame list, or None
        self.max_size = int(budgets.max())

    @property
    def n(self):
        return self.frames.shape[0]


def _noisy(frames, amount, seed):
    rng = np.random.default_rng(seed)
    return np.clip(frames.astype(np.int64) + rng.integers(-amount, amount + 1, frames.shape), 0, 255).astype(np.uint8)


def _budget(need, N, alpha, odd):
    """a budget whose plain answer is N: need[N] <= b - (b & 1) < need[N - 1]"""
    if alpha is None:
        b = int(need[1]) + 16
    elif alpha == "tiny":
        return 8
    else:
        lo, hi = int(need[N]), int(need[N - 1]) - 2          # (both even)
        assert hi >= lo, "scale %d is not the answer of any budget" % N
        b = lo + (int(alpha * (hi - lo)) & ~1)
    return b + 1 if odd else b


def _pick_scale(need, want):
    """the scale nearest `want` (from below, then above) that some budget answers with"""
    for N in list(range(want, 1, -1)) + list(range(want + 1, 64)):
        if need[N - 1] - 2 >= need[N]:
            return N
    raise AssertionError("flat need curve")


def _group(name, codec, w, h, frames, plan, uniform_from=None):
    """plan: per frame (target scale, alpha, odd); uniform_from: the frame whose budget every frame gets"""
    budgets = np.zeros(len(frames), np.int32)
    for i, (want, alpha, odd) in enumerate(plan):
        need = O.mdec_need(codec, w, h, frames[i])
        N = _pick_scale(need, want) if alpha not in (None, "tiny") else 0
        budgets[i] = _budget(need, N, alpha, odd)
    if uniform_from is not None:
        budgets[:] = budgets[uniform_from]
    return Group(name, codec, w, h, frames, budgets, int(budgets[0]) if uniform_from is not None else None)


@functools.lru_cache(maxsize=None)
def groups():
    out = []
    for codec in (0, 1, 2):
        tag = ("v2", "v3", "v3dc")[codec]
        # one frame: the launch of one
        f = _noisy(O.synth_frames(16, 16, 1, seed=11 + codec, amp=24), 6, 100 + codec)
        out.append(_group(tag + " 16x16 one", codec, 16, 16, f, [(3, 0.6, False)]))
        # thirteen frames with a budget each: every kind of outcome
        f = np.concatenate([O.synth_frames(32, 16, 4, seed=21 + codec, amp=8), _noisy(O.synth_frames(32, 16, 5, seed=31 + codec, amp=32), 10, 200 + codec),
                            _noisy(O.synth_frames(32, 16, 4, seed=41 + codec, amp=64), 24, 300 + codec)])
        plan = [(2, 0.9, False), (2, 0.1, True), (3, 0.5, False), (4, 0.02, False), (0, None, False), (0, "tiny", False), (3, 0.95, True),
                (5, 0.7, False), (4, 0.35, False), (2, 0.8, False), (6, 0.85, True), (2, 0.65, False), (3, 0.2, False)]
        out.append(_group(tag + " 32x16 thirteen", codec, 32, 16, f, plan))
        # six frames, one odd budget
        f = _noisy(O.synth_frames(48, 32, 6, seed=51 + codec, amp=16), 4, 400 + codec)
        out.append(_group(tag + " 48x32 uniform odd", codec, 48, 32, f, [(3, 0.7, True)] * 6, uniform_from=2))
        # 320x240: more than one workgroup per frame in the analysis
        f = _noisy(O.synth_frames(320, 240, 2, seed=61 + codec, amp=12), 3, 500 + codec)
        out.append(_group(tag + " 320x240 uniform even", codec, 320, 240, f, [(3, 0.8, False)] * 2, uniform_from=0))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def plain(gi):
    """the oracle's plain encode of group gi: (rows (n, max budget), results (n, 4)); a frame that fits no scale has a zero row, scale 64"""
    g = groups()[gi]
    rows = np.zeros((g.n, g.max_size), np.uint8)
    res = np.zeros((g.n, 4), np.int32)
    for i in range(g.n):
        b = int(g.budgets[i])
        r, rr, rc = O.mdec_encode(g.codec, g.w, g.h, g.frames[i:i + 1], b)
        if rc == 0:
            rows[i, :b], res[i] = r[0], rr[0]
        else:
            res[i] = [64, 0, 0, 0]
    return rows, res


@functools.lru_cache(maxsize=None)
def coefs(gi, i):
    g = groups()[gi]
    return S.blocks_from_coefs(O.mdec_coefs(g.w, g.h, g.frames[i]), g.w, g.h)


@functools.lru_cache(maxsize=None)
def _prepared(gi, i):
    return S.prepare(groups()[gi].codec, coefs(gi, i), int(plain(gi)[1][i, 0]))


@functools.lru_cache(maxsize=None)
def outcome(gi, i, K):
    g = groups()[gi]
    return S.refine(g.codec, coefs(gi, i), int(g.budgets[i]), int(plain(gi)[1][i, 0]), K, _prepared(gi, i))


def expected(gi, K):
    """rows, results and refine records of group gi after the refinement: (rows, results (n, 4) int32, records (n, 4) int64)"""
    g = groups()[gi]
    rows, res = (a.copy() for a in plain(gi))
    rec = np.zeros((g.n, 4), np.int64)
    for i in range(g.n):
        o = outcome(gi, i, K)
        rec[i] = o.record()
        if o.state == "refined":
            rows[i] = 0
            rows[i, :g.budgets[i]] = o.row
            res[i] = o.result
    return rows, res, rec


def _hash(row):
    h = 1469598103934665603
    for v in bytes(row):
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def recording():
    """the outcome as numbers and hashes: per group the budgets and plain scales, and per K the refine records, first fits, results
    and FNV-1a hashes of the refined rows (0 elsewhere)"""
    out = {}
    for gi, g in enumerate(groups()):
        out["g%d_budgets" % gi] = g.budgets.astype(np.int64)
        out["g%d_scales" % gi] = plain(gi)[1][:, 0].astype(np.int64)
        for K in KS:
            os_ = [outcome(gi, i, K) for i in range(g.n)]
            out["g%d_k%d_records" % (gi, K)] = np.array([o.record() for o in os_], np.int64)
            out["g%d_k%d_first_fit" % (gi, K)] = np.array([o.first_fit for o in os_], np.int64)
            out["g%d_k%d_results" % (gi, K)] = np.array([o.result if o.row is not None else [0, 0, 0, 0] for o in os_], np.int64)
            out["g%d_k%d_row_hash" % (gi, K)] = np.array([_hash(o.row) if o.row is not None else 0 for o in os_], np.uint64)
    return out


if __name__ == "__main__":
    import os
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mdec_shed_ref.npz"), **recording())
