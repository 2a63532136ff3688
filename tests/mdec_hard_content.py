"""Content on which the MDEC rate control is hard, and the oracle-side curves the tests of it are built from.

The encoder must return the FIRST quant scale, counting up from 1, whose stream fits the budget (psxavenc/mdec.c:663-723).
bits(scale) is not monotone, so that is not "one above the last scale that fails" -- but on noise, gradients, flat tiles and
the other content the suite used before this module, the bits fall at every step and the two cannot be told apart.  Here are
frames on which they differ, and the budgets at which it shows:

  dip_macroblocks()    seeded 16x16 luma patterns whose stream GROWS at some step s -> s + 1 (a "dip" at s: scale s fits a budget
                       that scale s + 1 does not)
  tile() and friends   frames made of them: plainly tiled, with per-macroblock DC offsets, two patterns in alternate columns,
                       a pattern over part of a frame of noise
  loose_frames()       frames whose refinement bound (csrc/mdec_search.h) is loose: a failing scale proves little there
  threshold_budgets()  for every scale the budget at which its stream fits exactly, one byte less (odd) and one word less
  frame_answering()    synthetic noise whose amplitude is searched until the oracle answers a wanted scale at a given budget
  catalogue()          the frames the CPU and GPU tests share, with the properties the tests rely on asserted

Everything here comes from the CPU oracle (oracle/, through oracle_lib) and numpy; the one thing read from the product is the table
header csrc/bs_vlc_lut.h, which tests/test_mdec_bound.py checks against the oracle cell by cell.  Nothing of the product is run.
Not a conftest and not a test: imported by tests/test_mdec_bound.py, tests/test_gpu_mdec_thresholds.py and tools/cpu_bits_curve.py.
"""
import functools
import os
import re

import numpy as np

import oracle_lib as O

ROOT = O.ROOT
LUT_H, LUT_W = 42, 63


# ---------------------------------------------------------------- the table header and the bits curve
@functools.lru_cache(maxsize=None)
def header_tables():
    """(len16 (42, 63), code (42, 63), quant in scan order (64), scan -> raster (64)) as written in csrc/bs_vlc_lut.h"""
    src = open(os.path.join(ROOT, "psxavenc_amd/csrc/bs_vlc_lut.h")).read()

    def arr(name, base):
        m = re.search(name + r"\[\d+\] = \{(.*?)\};", src, re.S)
        return np.array([int(x, base) for x in m.group(1).replace("\n", " ").split(",") if x.strip()], np.int64)
    return (arr("bs_ac_len16_lut", 16).reshape(LUT_H, LUT_W), arr("bs_ac_code_lut", 16).reshape(LUT_H, LUT_W),
            arr("bs_quant_zz", 10), arr("bs_zagzig", 10))


def luts():
    """(lengths, deficits, quant in scan order, scan -> raster): the fields of bs_ac_len16_lut, index [min(|level|, 41), run]"""
    len16, _, quant, zz = header_tables()
    return len16 & 0xFF, len16 >> 8, quant, zz


def block_bits(mag, scale, lens, defs, quant):
    """AC bits and deficit sum of every block at one scale.  mag: (blocks, 64) coefficient magnitudes in scan order (the DC slot
    is ignored).  Levels by the integer closed form of the reference's rounding division (tests/test_mdec_oracle.py pins it):
    |level| = (2 |c| + d) // (2 d), d = quant * scale; a level's length does not depend on its sign, and everything past the
    table's last row -- the clamp at -512 / 510 included -- is one 22-bit escape."""
    d = quant * scale
    q = (2 * mag + d) // (2 * d)
    nz = q != 0
    nz[:, 0] = False
    idx = np.arange(64)[None, :]
    prev = np.maximum.accumulate(np.where(nz, idx, 0), axis=1)              # position of the last coefficient so far (0: the DC slot)
    run = idx - np.concatenate([np.zeros((mag.shape[0], 1), np.int64), prev[:, :-1]], axis=1) - 1
    lv = np.minimum(q, LUT_H - 1)
    run = np.where(nz, run, 0)
    return (np.where(nz, lens[lv, run], 0).sum(axis=1), np.where(nz, defs[lv, run], 0).sum(axis=1))


def block_curves(mag, scales=range(1, 64)):
    """(bits (blocks, 64), deficit sums (blocks, 64)) over the scales, column 0 unused"""
    lens, defs, quant, _ = luts()
    mag = np.ascontiguousarray(mag, dtype=np.int64)
    tb = np.zeros((mag.shape[0], 64), np.int64)
    df = np.zeros((mag.shape[0], 64), np.int64)
    for s in scales:
        tb[:, s], df[:, s] = block_bits(mag, s, lens, defs, quant)
    return tb, df


def frame_blocks(w, h, frame):
    """coefficient magnitudes of a frame's blocks in scan order, from the oracle's DCT: (blocks, 64)"""
    zz = luts()[3]
    return np.abs(O.mdec_coefs(w, h, frame).reshape(-1, 64)[:, zz].astype(np.int64))


def curves(w, h, frame, scales=range(1, 64)):
    """AC bits and deficit sum of one frame per scale: (tb_ac[64], def[64]), index 0 unused"""
    tb, df = block_curves(frame_blocks(w, h, frame), scales)
    return tb.sum(axis=0), df.sum(axis=0)


def exact_bits(codec, w, h, frame, need=None):
    """(total bits per scale [64], deficit sums [64], fixed bits): the AC bits of curves() plus the scale-independent rest (DC, end
    of block, end of frame: read off the oracle's own stream at scale 1), held to the oracle's curve at every scale"""
    need = O.mdec_need(codec, w, h, frame) if need is None else need
    ac, df = curves(w, h, frame)
    out, res, rc = O.mdec_encode(codec, w, h, frame[None, :], int(need[1]))
    assert rc == 0 and res[0, 0] == 1
    rc, _, _, _, nbits = O.mdec_decode(w, h, out[0], v3dc_wrap=int(codec == 2))
    assert rc == 0
    fixed = nbits - int(ac[1])
    tb = ac + fixed
    tb[0] = 0
    assert np.array_equal(8 + 2 * ((tb[1:] + 15) // 16), need[1:]), "numpy bits curve and the oracle disagree"
    return tb, df, fixed


# ---------------------------------------------------------------- budgets
def first_fit(need, budget):
    """the reference's answer from the curve alone: the first scale whose stream fits (64: none).  The bit writer's capacity test
    sits between the two bytes of a word (mdec.c:321-333), so an odd budget loses its last byte."""
    ok = np.nonzero(need[1:] <= budget - (budget & 1))[0]
    return int(ok[0]) + 1 if ok.size else 64


def last_fail_plus_one(need, budget):
    """what a search that trusts monotonicity answers: one above the highest scale that does not fit (64: scale 63 fails)"""
    bad = np.nonzero(need[1:] > budget - (budget & 1))[0]
    return int(bad[-1]) + 2 if bad.size else 1


def threshold_budgets(need):
    """for every scale: its stream fits exactly, is one byte too long (an odd budget), is one 16-bit word too long"""
    b = {int(need[s]) - k for s in range(1, 64) for k in (0, 1, 2)}
    return sorted(x for x in b if x >= 8)


def dip_scales(need):
    """scales s where the coarser scale s + 1 needs MORE bytes"""
    return [s for s in range(1, 63) if need[s + 1] > need[s]]


# ---------------------------------------------------------------- dip patterns
def _pattern(rng):
    a, b = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    c = int(rng.integers(10, 250))
    yy, xx = np.mgrid[0:16, 0:16]
    return (((xx // a + yy // b) % 2) * c + rng.integers(0, 4, (16, 16))).astype(np.uint8)


def _mb_frame(pattern):
    f = np.full(16 * 16 * 3 // 2, 128, np.uint8)
    f[:256] = pattern.ravel()
    return f


@functools.lru_cache(maxsize=None)
def dip_macroblocks(seed=2024, count=24, candidates=1500, min_bits=1):
    """The first `count` patterns of a seeded stream of checker-like 16x16 luma patterns (chroma 128) that have a step where the
    coarser scale costs at least `min_bits` MORE AC bits.  A v2 macroblock carries no state, so tiling a pattern over n macroblocks
    multiplies the step by n: over 16 macroblocks and more it is a 16-bit word at least, whatever its size.  Returns [(pattern (16, 16) uint8, dips)],
    dips = the scales s with bits(s + 1) >= bits(s) + min_bits; confirmed with the oracle's curve of the 64x64 tiling."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(candidates):
        p = _pattern(rng)
        tb = curves(16, 16, _mb_frame(p))[0]
        dips = [s for s in range(1, 63) if tb[s + 1] >= tb[s] + min_bits]
        if dips:
            out.append((p, tuple(dips)))
            if len(out) == count:
                break
    for p, dips in out:
        need = O.mdec_need(0, 64, 64, tile(p, 64, 64))
        assert all(need[s + 1] > need[s] for s in dips), dips
    return tuple(out)


def separate(dips):
    """number of separate dips: runs of consecutive dip scales count once"""
    return sum(1 for i, s in enumerate(dips) if i == 0 or s != dips[i - 1] + 1)


# ---------------------------------------------------------------- frames
def _nv21(luma):
    h, w = luma.shape
    f = np.full(w * h * 3 // 2, 128, np.uint8)
    f[:w * h] = luma.astype(np.uint8).ravel()
    return f


def tile(pattern, w, h, dc_seed=None):
    """the pattern over the whole frame.  dc_seed: every macroblock's luma is lifted by an offset of its own, which moves only the
    DC terms (v3 / v3dc then carry real DC deltas) -- kept inside what leaves the pixels in 0..255, so no AC term moves."""
    luma = np.tile(pattern.astype(np.int64), (h // 16, w // 16))
    if dc_seed is not None:
        room = 255 - int(pattern.max())
        assert room >= 1
        off = np.random.default_rng(dc_seed).integers(0, room + 1, (h // 16, w // 16))
        luma += np.kron(off, np.ones((16, 16), np.int64))
    assert luma.min() >= 0 and luma.max() <= 255
    return _nv21(luma)


def tile_columns(p0, p1, w, h):
    """two patterns in alternate macroblock columns"""
    row = np.concatenate([p0 if (k & 1) == 0 else p1 for k in range(w // 16)], axis=1)
    return _nv21(np.tile(row, (h // 16, 1)))


def tile_over_noise(pattern, w, h, rows, seed, amp):
    """the pattern over the top `rows` macroblock rows of a frame of synthetic noise: what a sample of the frame says about its bits
    (the pilot, the quarter-pass checkpoint) is then wrong about the part it did not see"""
    f = O.synth_frames(w, h, 1, seed=seed, amp=amp)[0].copy()
    luma = f[:w * h].reshape(h, w)
    luma[:rows * 16] = np.tile(pattern, (rows, w // 16))
    return f


def loose_frames(w, h):
    """frames on which the refinement bound is loose (the deficits are about a fifth of the AC bits at some scales): one-pixel
    stripes, and the hard-edged frame of the golden set"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_mdec_golden import special_frames
    yy, xx = np.mgrid[0:h, 0:w]
    return [("stripes", _nv21((xx & 1) * 255)), ("hard edges", special_frames(w, h)[8])]


# ---------------------------------------------------------------- a frame that answers a wanted scale at a given budget
def noise_frame(w, h, level, seed):
    """synthetic noise whose amplitude is level / (macroblock rows): amplitude level // rows everywhere, one more over the luma of
    the top level % rows macroblock rows (the generator keys its noise by pixel, so the two amplitudes blend without a seam)"""
    rows = h // 16
    a, k = divmod(int(level), rows)
    f = O.synth_frames(w, h, 1, seed=seed, amp=a)[0].copy()
    if k:
        f[:k * 16 * w] = O.synth_frames(w, h, 1, seed=seed, amp=a + 1)[0][:k * 16 * w]
    return f


def oracle_answer(codec, w, h, frame, budget):
    _, res, rc = O.mdec_encode(codec, w, h, frame[None, :], int(budget))
    assert rc in (0, -2)
    return int(res[0, 0]) if rc == 0 else 64


def frame_answering(codec, w, h, budget, want, seeds=(900, 901, 902, 903)):
    """Noise whose amplitude is searched with the oracle until the encoder answers `want` at `budget`: per seed a bisection for the
    smallest amplitude level that answers `want` or more (the answer grows with the amplitude), then the levels around it.  None when
    no seed has such a level: the answer jumps over `want` (consecutive scales that need nearly the same bytes), or not even the
    loudest noise needs a scale as coarse as `want` at this budget (loudest_answer() tells)."""
    rows = h // 16
    for seed in seeds:
        lo, hi = 0, 255 * rows
        if oracle_answer(codec, w, h, noise_frame(w, h, lo, seed), budget) > want:
            continue
        if oracle_answer(codec, w, h, noise_frame(w, h, hi, seed), budget) < want:
            continue                                     # (the loudest noise there is answers a finer scale at this budget)
        while hi - lo > 1:                               # answer(lo) <= want; answer(hi) taken as > want
            mid = (lo + hi) // 2
            if oracle_answer(codec, w, h, noise_frame(w, h, mid, seed), budget) <= want:
                lo = mid
            else:
                hi = mid
        for level in (lo, lo - 1, lo - 2, lo + 1, lo + 2, lo - 3):
            if 0 <= level <= 255 * rows:
                f = noise_frame(w, h, level, seed)
                if oracle_answer(codec, w, h, f, budget) == want:
                    return f
    return None


def loudest_answer(codec, w, h, budget, seeds=(900, 901, 902, 903)):
    """the coarsest answer full-range noise reaches at this budget"""
    return max(oracle_answer(codec, w, h, noise_frame(w, h, 255 * (h // 16), seed), budget) for seed in seeds)


# ---------------------------------------------------------------- the catalogue
class Frame:
    """one catalogue frame: name, size, NV21 bytes, the codecs it is run with, whether it is built on a dip pattern"""
    def __init__(self, name, w, h, frame, kind, codecs=(0, 1, 2)):
        self.name, self.w, self.h, self.frame, self.kind, self.codecs = name, w, h, np.ascontiguousarray(frame), kind, codecs
        self._need = {}

    def need(self, codec=0):
        """the oracle's bytes-needed curve, need[1..63]"""
        if codec not in self._need:
            self._need[codec] = O.mdec_need(codec, self.w, self.h, self.frame)
        return self._need[codec]

    def dips(self, codec=0):
        return dip_scales(self.need(codec))

    def budgets(self, codec=0):
        return threshold_budgets(self.need(codec))


BOUNDARIES = (8, 16, 32)          # the split kernel's rounds of scales end here (eight scales in a short first round, then sixteen)


@functools.lru_cache(maxsize=None)
def catalogue():
    """The frames the rate-control tests share.  Dip patterns: the first 24 of the seeded stream, the first with a dip at each scale
    next to a round boundary of the split kernel (7..10, 15..18, 31..34), the first five with two or more separate dips, the first two
    with a dip at 62 (scale 63 fails where a finer scale fits).  320x240 (the flagship size) for six plainly tiled dip frames, the
    dips at 8, 16, 32 and 62, a pattern over noise and both loose-bound frames;
    the rest alternate between 48x32 (6 macroblocks: no quarter-pass checkpoint) and 192x128 (96: checkpoint active), every third with
    per-macroblock DC offsets, some as two patterns in alternate columns; two at 640x480 for v3, a pattern over three rows of a
    quiet frame (so that every threshold stays inside what a context of that size accepts).  Three ordinary synthetic frames ride
    along.  check_catalogue() holds the properties the tests lean on."""
    pats = dip_macroblocks(2024, 176)
    picked = list(range(24))
    at_boundary = {}
    for tgt in (7, 8, 9, 10, 15, 16, 17, 18, 31, 32, 33, 34):
        k = next((i for i, (_, d) in enumerate(pats) if tgt in d), None)
        if k is not None:
            at_boundary[tgt] = k
            if k not in picked:
                picked.append(k)
    multi = [i for i, (_, d) in enumerate(pats) if separate(d) >= 2][:5]
    picked += [i for i in multi if i not in picked]
    top = [i for i, (_, d) in enumerate(pats) if 62 in d][:2]          # scale 63 fails a budget that scale 62 fits
    assert len(top) == 2
    picked += [i for i in top if i not in picked]

    out = []
    big = list(range(6)) + [at_boundary[b] for b in BOUNDARIES if b in at_boundary and at_boundary[b] >= 6]
    big += [i for i in top[:1] if i not in big]
    for i in big:
        out.append(Frame("dip %d tiled 320x240" % i, 320, 240, tile(pats[i][0], 320, 240), "dip"))
    out.append(Frame("dip 6 over noise 320x240", 320, 240, tile_over_noise(pats[6][0], 320, 240, 5, 21, 6), "dip"))
    for name, f in loose_frames(320, 240):
        out.append(Frame(name + " 320x240", 320, 240, f, "loose"))
    rest = [i for i in picked if i not in big and i != top[1]]
    out.append(Frame("dip %d tiled 192x128" % top[1], 192, 128, tile(pats[top[1]][0], 192, 128), "dip"))
    for n, i in enumerate(rest):
        w, h = ((48, 32), (192, 128))[n & 1]
        p = pats[i][0]
        if (w, h) == (48, 32) and not dip_scales(O.mdec_need(0, w, h, tile(p, w, h))):
            w, h = 192, 128                          # (six macroblocks do not make this pattern's step a whole word)
        if n % 3 == 2 and int(p.max()) <= 251:
            out.append(Frame("dip %d tiled %dx%d, DC offsets" % (i, w, h), w, h, tile(p, w, h, dc_seed=i), "dip"))
        elif n % 7 == 3:
            j = rest[(n + 1) % len(rest)]
            out.append(Frame("dips %d | %d in columns %dx%d" % (i, j, w, h), w, h, tile_columns(p, pats[j][0], w, h), "dip"))
        else:
            out.append(Frame("dip %d tiled %dx%d" % (i, w, h), w, h, tile(p, w, h), "dip"))
    out.append(Frame("dip 7 over noise 192x128", 192, 128, tile_over_noise(pats[7][0], 192, 128, 3, 22, 10), "dip"))
    for i in (4, 15):
        out.append(Frame("dip %d over a quiet frame 640x480" % i, 640, 480, tile_over_noise(pats[i][0], 640, 480, 3, 5, 0), "dip", codecs=(1,)))
    for (w, h, seed, amp) in ((320, 240, 31, 8), (192, 128, 32, 3), (48, 32, 33, 30)):
        out.append(Frame("synthetic amp %d %dx%d" % (amp, w, h), w, h, O.synth_frames(w, h, 1, seed=seed, amp=amp)[0], "ordinary"))
    check_catalogue(out, [pats[i] for i in picked])
    return tuple(out)


def check_catalogue(frames, patterns):
    """what the tests rely on, from the oracle alone"""
    assert len({p.tobytes() for p, _ in patterns}) >= 24, "at least 24 distinct dip patterns"
    dips = set()
    several = 0
    for f in frames:
        if f.kind == "dip":
            d = f.dips(f.codecs[0])
            dips.update(d)
            several += separate(d) >= 2
    for b in BOUNDARIES:
        assert b in dips, "a dip at scale %d itself" % b
        assert (b - 1 in dips or b in dips) and (b + 1 in dips or b + 2 in dips), "dips either side of %d|%d" % (b, b + 1)
    assert several >= 4, "at least four frames with two or more separate dips"
    assert all(f.dips(f.codecs[0]) for f in frames if f.kind == "dip"), "every dip frame has a dip at its own size"
    assert sum(f.kind == "dip" for f in frames) >= 24
    assert sum(62 in f.dips(f.codecs[0]) for f in frames) >= 2, "frames on which scale 63 needs more than scale 62"
    loose = [f for f in frames if f.kind == "loose"]
    assert len(loose) == 2
    for f in loose:                                  # the deficits reach a sixth of the AC bits at some scale: a failure proves little
        ac, df = curves(f.w, f.h, f.frame)
        assert (6 * df[1:] >= ac[1:]).any() and ac[1:].min() > 0, f.name
    assert len(frames) == len({f.name for f in frames})
