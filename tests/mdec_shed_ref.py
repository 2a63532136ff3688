"""The rule "psxhip MDEC shed v1"  as a numpy statement: what psxhip_mdec_refine_frames_device must compute.

Integers only.  The statement takes the encoder's FDCT coefficients F of a frame (blocks in the encoder's order, raster order inside a
block), the frame's budget b and the plain encode's quant scale N, and says whether the frame is refined at M = N - 1, with which shed
step t*, and what its row and result then are.  It imports nothing of the product and nothing of the oracle's code; the AC code
lengths and strings are read as data from oracle/bs_vlc_tables.h (mdec_foreign_streams.books()), the zig-zag order and the quant
matrix are written out below.  Not a conftest and not a test: imported by tests/test_mdec_shed_ref.py, tests/test_mdec_shed_core_cpu.py
and tests/test_gpu_mdec_shed.py.
"""
import functools

import numpy as np

from mdec_foreign_streams import books

QS_RELEASED = 65
CLASS_STEPS = 63                                     # shed steps per magnitude class: one per AC position, 63 down to 1

ZAGZIG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])
QUANT_ZZ = np.array([2, 16, 16, 19, 16, 19, 22, 22, 22, 22, 22, 22, 26, 24, 26, 27, 27, 27, 26, 26, 26, 26, 27, 27, 27, 29, 29, 29, 34,
                     34, 34, 29, 29, 29, 27, 27, 29, 29, 32, 32, 34, 34, 37, 38, 37, 35, 35, 34, 35, 38, 38, 40, 40, 40, 48, 48, 46, 46,
                     56, 56, 58, 69, 69, 83], np.int64)
ESCAPE_BITS = 22


@functools.lru_cache(maxsize=None)
def ac_len():
    """LEN[run][|level|], run 0..63, |level| 0..512: the bits of the pair's code with its sign, 22 where only the escape carries it"""
    t = np.full((64, 513), ESCAPE_BITS, np.int64)
    for (run, level), bits in books()[0].items():
        t[run, level] = len(bits) + 1
    t[:, 0] = 0
    return t


def div_rounded(n, d):
    """DIVIDE_ROUNDED (mdec.c:438): n / d rounded half away from zero, d > 0"""
    n = np.asarray(n, np.int64)
    return np.sign(n) * ((2 * np.abs(n) + d) // (2 * d))


def clampmap(v):
    return np.clip(v, -0x200, 0x1FE)


def blocks_from_coefs(coefs, w, h):
    """oracle_lib.mdec_coefs' (6, macroblocks, 64) in raster order -> (blocks, 64) int64 in zig-zag order, blocks in the encoder's
    order: macroblocks column by column, Cr, Cb, Y0..Y3 in each (mdec.c:605-642)"""
    nx, ny = w // 16, h // 16
    order = [(i, fy * nx + fx) for fx in range(nx) for fy in range(ny) for i in range(6)]
    F = np.stack([coefs[i, mb] for i, mb in order]).astype(np.int64)
    return F[:, ZAGZIG]


def levels(F, s):
    """lv_s: (blocks, 64), column 0 left 0"""
    lv = clampmap(div_rounded(F, QUANT_ZZ * s))
    lv[:, 0] = 0
    return lv


def dc_terms(codec, F):
    """(DC levels, what the stream carries per block -- the level (v2) or the delta in steps of 4 (v3, v3dc) --, DC bits of the frame)"""
    dc = clampmap(div_rounded(F[:, 0], 16))
    if codec == 0:
        return dc, dc.copy(), 10 * len(dc)
    _, pl, pc, zl, zc = books()
    carried = np.zeros_like(dc)
    last = [0, 0, 0]
    bits = 0
    for b in range(len(dc)):
        c = min(b % 6, 2)
        delta = int(div_rounded(int(dc[b]) - last[c], 4))
        last[c] = ((last[c] + 4 * delta + 0x8000) & 0xFFFF) - 0x8000
        if codec == 2:
            delta = delta + 0x100 if delta < -0x80 else (delta - 0x100 if delta > 0x80 else delta)
        assert abs(delta) <= 255, "the encoder has no DC code for this delta"
        carried[b] = delta
        if delta == 0:
            bits += len(zl if c == 2 else zc)
        else:
            m = abs(delta).bit_length() - 1
            bits += len((pl if c == 2 else pc)[m]) + 1 + m
    return dc, carried, bits


def step_class(t):
    """t >= 1 -> (m, p)"""
    return 1 + (t - 1) // CLASS_STEPS, 64 - ((t - 1) % CLASS_STEPS + 1)


def shed(lv, t):
    """the levels step t leaves: |lv| <= m - 1 zeroed everywhere, |lv| <= m zeroed at positions z >= p"""
    if t == 0:
        return lv.copy()
    m, p = step_class(t)
    a = np.abs(lv)
    z = np.arange(64)
    gone = (a <= m - 1) | ((a <= m) & (z >= p))
    gone[:, 0] = False
    return np.where(gone, 0, lv)


def ac_bits(lv):
    """bits of the AC codes of the levels as they stand"""
    LEN = ac_len()
    total = 0
    for row in lv:
        k = np.flatnonzero(row[1:]) + 1
        if k.size:
            runs = np.diff(np.concatenate([[0], k])) - 1
            total += int(LEN[runs, np.abs(row[k])].sum())
    return total


def frame_need(bits):
    """the bytes a stream of `bits` bits takes, header included, before the round-up to 4 (the encoder's own count)"""
    return 8 + 2 * ((bits + 15) // 16)


def fits(bits, b):
    return frame_need(bits) <= b - (b & 1)


def deltas(F, lvM, M, K):
    """per class m = 1..K and position p: the change in AC bits, in distortion and in the count of levels when step (m, p) follows the
    step before it, summed over the frame's blocks: (dbits, ddist, dcnt), each (K + 1, 64) with row 0 unused"""
    LEN = ac_len()
    dbits = np.zeros((K + 1, 64), np.int64)
    ddist = np.zeros((K + 1, 64), np.int64)
    dcnt = np.zeros((K + 1, 64), np.int64)
    A = np.abs(lvM)
    R = lvM * QUANT_ZZ * M
    gain = F * F - (F - R) ** 2
    for b in range(lvM.shape[0]):
        a = A[b]
        for m in range(1, K + 1):
            for p in np.flatnonzero(a == m):
                if p == 0:
                    continue
                below = np.flatnonzero(a[1:p] >= m)
                prev = below[-1] + 1 if below.size else 0
                above = np.flatnonzero(a[p + 1:] > m)
                r = p - prev - 1
                d = -LEN[r, m]
                if above.size:
                    nxt = p + 1 + above[0]
                    r2 = nxt - p - 1
                    d += LEN[r + 1 + r2, a[nxt]] - LEN[r2, a[nxt]]
                dbits[m, p] += d
                ddist[m, p] += gain[b, p]
                dcnt[m, p] += 1
    return dbits, ddist, dcnt


class Outcome:
    """what the rule says of one frame.  state: "untouched", "declined" or "refined"; step, count, d_plain, d_shed: the refine record;
    bits[t], dist[t], gone[t] for t = 0 .. 63 K: the whole curves (None when untouched); first_fit: t* also when declined; lv: the shed levels at scale M with the DC
    level in column 0 (refined only); row, result: the frame's new row and result (refined only)"""

    def __init__(self):
        self.state, self.step, self.count, self.d_plain, self.d_shed = "untouched", 0, 0, 0, 0
        self.first_fit = 0                           # t* whether the frame is then refined or declined; 0: nothing fits
        self.bits = self.dist = self.gone = self.lv = self.row = self.result = None
        self.M = 0

    def record(self):
        return (self.step, self.count, self.d_plain, self.d_shed)


MAX_K = 3


def prepare(codec, F, N):
    """everything of the rule that depends neither on the budget nor on K (None for a frame that is left alone)"""
    if N == 1 or N >= 64:                            # (PSXHIP_MDEC_QS_RELEASED is 65)
        return None
    M = N - 1
    lvM, lvN = levels(F, M), levels(F, N)
    ac = F.copy()
    ac[:, 0] = 0
    d_plain = int(((ac - lvN * QUANT_ZZ * N) ** 2).sum())
    d_base = int(((ac - lvM * QUANT_ZZ * M) ** 2).sum())
    return (lvM, dc_terms(codec, F), d_plain, d_base, ac_bits(lvM), deltas(F, lvM, M, MAX_K))


def refine(codec, F, b, N, K, prepared=None):
    """The rule.  F: blocks_from_coefs(); b: the frame's budget (vetted by the caller); N: the plain result's quant_scale; K: 1..3"""
    out = Outcome()
    prepared = prepared if prepared is not None else prepare(codec, F, N)
    if prepared is None:
        return out
    M = out.M = N - 1
    nblk = F.shape[0]
    lvM, (dc, carried, dc_bits), d_plain, d_base, bits0, (dbits, ddist, dcnt) = prepared
    steps = CLASS_STEPS * K
    bits = np.zeros(steps + 1, np.int64)
    dist = np.zeros(steps + 1, np.int64)
    gone = np.zeros(steps + 1, np.int64)
    bits[0] = dc_bits + bits0 + 2 * nblk + 10
    dist[0] = d_base
    for t in range(1, steps + 1):
        m, p = step_class(t)
        bits[t] = bits[t - 1] + dbits[m, p]
        dist[t] = dist[t - 1] + ddist[m, p]
        gone[t] = gone[t - 1] + dcnt[m, p]
    out.bits, out.dist, out.gone = bits, dist, gone
    out.state = "declined"
    fit = [t for t in range(1, steps + 1) if fits(int(bits[t]), b)]
    if not fit:
        return out
    t = out.first_fit = fit[0]
    out.d_plain, out.d_shed = d_plain, int(dist[t])
    if not out.d_shed < d_plain:
        return out
    out.state, out.step, out.count = "refined", t, int(gone[t])
    lv = shed(lvM, t)
    nnz = int(np.count_nonzero(lv[:, 1:]))
    lv[:, 0] = dc
    out.lv = lv
    given = lv.copy()
    given[:, 0] = carried
    out.row, out.result = write_row(codec, given, M, b, nnz)
    assert out.result[1] == (frame_need(int(bits[t])) + 3) & ~3
    return out


# ---------------------------------------------------------------- the row: what encode_frame_bs would write for these levels
def _bits(value, n):
    return format(value & ((1 << n) - 1), "0%db" % n) if n else ""


def write_row(codec, given, scale, b, nnz):
    """given: (blocks, 64), column 0 the DC level (v2) or delta (v3).  Returns (row (b,) uint8, [quant_scale, bytes_used, blocks_used,
    uncomp_hwords_used]) -- mdec.c:497,507,719-754"""
    ac, pl, pc, zl, zc = books()
    parts = []
    for blk, row in enumerate(given.tolist()):
        if codec == 0:
            parts.append(_bits(row[0], 10))
        else:
            delta, luma = row[0], blk % 6 >= 2
            if delta == 0:
                parts.append(zl if luma else zc)
            else:
                m = abs(delta).bit_length() - 1
                parts.append((pl if luma else pc)[m])
                parts.append("1" + _bits(delta - (1 << m), m) if delta > 0 else "0" + _bits(delta + (2 << m) - 1, m))
        last = 0
        for k in range(1, 64):
            if row[k]:
                code = ac.get((k - last - 1, abs(row[k])))
                parts.append(code + ("1" if row[k] < 0 else "0") if code else "000001" + _bits(k - last - 1, 6) + _bits(row[k], 10))
                last = k
        parts.append("10")
    parts.append(_bits(0x1FF if codec == 0 else 0x3FF, 10))
    s = "".join(parts)
    nbits = len(s)
    s += "0" * (-nbits % 16)
    words = np.frombuffer(int(s, 2).to_bytes(len(s) // 8, "big"), ">u2").astype("<u2")
    hwords = (nnz + 2 * given.shape[0] + 2 + 0x3F) & ~0x3F
    blocks_used = (hwords + 1) >> 1
    head = np.array([blocks_used & 0xFFFF, 0x3800, scale, 2 if codec == 0 else 3], "<u2")
    stream = np.frombuffer(head.tobytes() + words.tobytes(), np.uint8)
    assert stream.size <= b - (b & 1)
    row = np.zeros(b, np.uint8)
    row[:stream.size] = stream
    return row, [scale, (stream.size + 3) & ~3, blocks_used, hwords]
