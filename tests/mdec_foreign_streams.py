"""BS v2 / v3 streams that this project's encoder did not write: an independent bit writer and a seeded corpus made with it.

The decoder's other tests read streams of the oracle's encoder (oracle/mdec_oracle.c), which never escapes a pair that has a table
code, never writes level 0 or +511, a quant scale outside 1..63, a coefficient that saturates, a v3 DC that leaves ten bits, or a
block of 63 escapes.  The syntax allows all of them and another encoder may write them.

The writer itself uses numpy and the standard library only.  It imports nothing of the product, calls neither the oracle's encoder
nor its readers, and takes the 111 AC code strings, the two DC prefix books and the two zero codes from oracle/bs_vlc_tables.h as data.  It
writes the syntax of the head comment of psxavenc_amd/csrc/mdec_parse.h and is pinned by frames written out by hand
(tests/test_mdec_foreign_cpu.py).  Not a conftest and not a test: imported by tests/test_mdec_foreign_cpu.py and
tests/test_gpu_mdec_foreign.py.

One import is not the standard library's: the Case class of tests/mdec_decode_corpus.py is reused, and importing that module loads
tests/oracle_lib.py (the ctypes wrapper of the oracle) with it.  Nothing of either is called here; the readers are run by the tests.

The corpus pairs every Case (name, w, h, wrap, data, size) with what a reader must report:
(status, levels (blocks, 64) int16, quant scale, version, bits consumed) for the clean frames, the status alone for the negative ones.
"""
import functools
import os
import re

import numpy as np

from mdec_decode_corpus import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the code books, read as data
@functools.lru_cache(maxsize=None)
def books():
    """({(run, level): bits}, luma prefixes[8], chroma prefixes[8], luma zero code, chroma zero code)"""
    src = open(os.path.join(ROOT, "oracle/bs_vlc_tables.h")).read()
    ac = {(int(r), int(l)): b for r, l, b in re.findall(r'\{\s*(\d+),\s*(\d+),\s*"([01]+)"\}', src)}
    assert len(ac) == 111

    def strings(name):
        return tuple(re.findall(r'"([01]+)"', re.search(name + r"\[8\] = \{(.*?)\};", src).group(1)))
    zero = {k: re.search(r'#define ORC_DC_%s_ZERO "([01]+)"' % k, src).group(1) for k in ("LUMA", "CHROMA")}
    return ac, strings("orc_dc_luma_prefix"), strings("orc_dc_chroma_prefix"), zero["LUMA"], zero["CHROMA"]


# ---------------------------------------------------------------- the writer
EOB = "10"
ESCAPE = "000001"
END_CODE = {2: 0x1FF, 3: 0x3FF}


def _bits(value, n):
    return format(value & ((1 << n) - 1), "0%db" % n) if n else ""


class BitWriter:
    """One frame, one syntax element per call.  `escapes` and `table_codes` record what was written, for the coverage checks:
    (block, position, run, level, a table code exists) and (run, |level|, negative)."""

    def __init__(self, version, quant_scale):
        self.version, self.quant_scale = version, quant_scale
        self.parts = []
        self.nbits = 0
        self.hwords = 0                       # 16-bit words of the run-length data the stream stands for: the header's first field
        self.blk, self.k = 0, 0
        self.escapes, self.table_codes, self.dc_classes = [], [], []
        self.block_bits, self._start = [], 0  # bits per block, DC to end of block

    def _put(self, s):
        self.parts.append(s)
        self.nbits += len(s)

    def dc_v2(self, level):
        self._start = self.nbits
        self._put(_bits(level, 10))
        self.k = 0
        self.hwords += 1

    def dc_v3(self, delta, luma):
        """delta: the change of the component's DC in steps of 4, -255..255"""
        _, pl, pc, zl, zc = books()
        self._start = self.nbits
        if delta == 0:
            self._put(zl if luma else zc)
            self.dc_classes.append((bool(luma), 0, 0))
        else:
            m = abs(delta).bit_length() - 1
            assert 0 <= m <= 7
            self._put((pl if luma else pc)[m])
            self._put("1" + _bits(delta - (1 << m), m) if delta > 0 else "0" + _bits(delta + (2 << m) - 1, m))
            self.dc_classes.append((bool(luma), m + 1, 1 if delta > 0 else -1))
        self.k = 0
        self.hwords += 1

    def ac(self, run, level, escape=False):
        """(run, level) as its table code and a sign bit, or as the 22-bit escape when it has none or `escape` is set"""
        code = books()[0].get((run, abs(level))) if level else None
        if code is None or escape:
            assert 0 <= run <= 63 and -512 <= level <= 511
            self._put(ESCAPE + _bits(run, 6) + _bits(level, 10))
            self.escapes.append((self.blk, self.k + run + 1, run, level, code is not None))
        else:
            self._put(code + ("1" if level < 0 else "0"))
            self.table_codes.append((run, abs(level), level < 0))
        self.k += run + 1
        self.hwords += 1

    def eob(self):
        self._put(EOB)
        self.block_bits.append(self.nbits - self._start)
        self.blk += 1
        self.hwords += 1

    def end(self, code=None):
        self._put(_bits(END_CODE[self.version] if code is None else code, 10))

    def finish(self):
        """(bytes, bits written): the header, then the bits most significant first in 16-bit words stored low byte first"""
        bits = "".join(self.parts)
        assert len(bits) == self.nbits
        bits += "0" * (-len(bits) % 16)
        words = np.frombuffer(int(bits, 2).to_bytes(len(bits) // 8, "big"), ">u2").astype("<u2") if bits else np.zeros(0, "<u2")
        size_field = (((self.hwords + 0x3F) & ~0x3F) + 1) >> 1
        head = np.array([size_field & 0xFFFF, 0x3800, self.quant_scale, self.version], "<u2")
        return head.tobytes() + words.tobytes(), self.nbits


def _escape_test(policy):
    """escape_policy -> (f(block, position) -> bool, the (block, position) pairs written whatever their level)"""
    if policy is None or policy == "needed":
        return (lambda b, k: False), frozenset()
    if policy == "always":
        return (lambda b, k: True), frozenset()
    if isinstance(policy, tuple) and policy[0] == "p":
        rng = np.random.default_rng(policy[2])
        p = policy[1]
        return (lambda b, k: bool(rng.random() < p)), frozenset()
    at = frozenset((int(b), int(k)) for b, k in policy)
    return (lambda b, k: (b, k) in at), at


def _write_blocks(levels_or_deltas, version, quant_scale, escape_policy, end_code=None, raw_v2_dc=None, overrun=None):
    """The one block loop: DC, the coefficients that are not 0 (and the forced positions), end of block, per block; then the end code.
    For the negative frames: end_code replaces the version's own, raw_v2_dc = {block: 10-bit value} replaces a v2 DC, overrun =
    (block, f) appends an escape of run f(last position written) and level 5 before that block's end.  Returns (writer, the bit
    position of the end code)."""
    lv = np.asarray(levels_or_deltas, np.int64).reshape(-1, 64)
    esc, forced = _escape_test(escape_policy)
    w = BitWriter(version, quant_scale)
    for b in range(lv.shape[0]):
        if version == 2:
            w.dc_v2(int(lv[b, 0]) if raw_v2_dc is None or b not in raw_v2_dc else raw_v2_dc[b])
        else:
            w.dc_v3(int(lv[b, 0]), luma=b % 6 >= 2)
        last = 0
        row = lv[b].tolist()
        for k in range(1, 64):
            if row[k] != 0 or (b, k) in forced:
                w.ac(k - last - 1, row[k], esc(b, k))
                last = k
        if overrun is not None and overrun[0] == b:
            w.ac(overrun[1](last), 5, escape=True)
        w.eob()
    at = w.nbits
    w.end(end_code)
    return w, at


def write(levels_or_deltas, version, quant_scale, wrap=False, escape_policy="needed", return_writer=False):
    """One frame.  levels_or_deltas: (blocks, 64) in zig-zag order, blocks Cr, Cb, Y0..Y3 per macroblock; column 0 is the DC level
    (v2) or the DC delta in steps of 4 (v3).  escape_policy: "needed" (only pairs without a table code), "always", ("p", p, seed),
    or a set of (block, position) pairs, which are escaped and written even where the level is 0.  The bits do NOT depend on `wrap`:
    the wrap is the reader's, it only says which levels the deltas stand for (expected_levels()); here it is checked to be asked of
    a v3 stream only.  Returns (bytes, bits written)."""
    assert not wrap or version == 3, "the 10-bit DC wrap exists for v3 only"
    w, _ = _write_blocks(levels_or_deltas, version, quant_scale, escape_policy)
    data, nbits = w.finish()
    return (data, nbits, w) if return_writer else (data, nbits)


def expected_levels(levels_or_deltas, version, wrap):
    """the levels the syntax defines for what write() was given: for v3 the running sum of delta * 4 per component (Cr, Cb, Y), wrapped
    to ten bits when `wrap` is set and cast to int16 otherwise.  Also returns the running DCs before the cast."""
    lv = np.array(levels_or_deltas, np.int64).reshape(-1, 64)
    running = lv[:, 0].copy()
    if version == 3:
        last = [0, 0, 0]
        for b in range(lv.shape[0]):
            c = min(b % 6, 2)
            last[c] += int(lv[b, 0]) * 4
            if wrap:
                last[c] = ((last[c] + 512) & 0x3FF) - 512
            running[b] = last[c]
        lv[:, 0] = running
    return lv.astype(np.int16), running              # (astype wraps modulo 2^16: the int16 cast)


# ---------------------------------------------------------------- the corpus
SIZES = ((16, 16), (48, 32), (64, 64))
CODECS = ((2, 0), (3, 0), (3, 1))                    # (version, wrap): v2, v3, v3dc
SCALES = (0, 1, 63, 64, 16383, 16384, 65535)
POLICIES = ("needed", "always", "p30")
BLOCK_CLASSES = ("dense", "extremes", "sparse", "last", "empty", "codes", "runs", "zeros")
V2_DC_SET = (-512, -1, 0, 1, 510)
# both ends of every size class, either sign, and 0: -255, -128, -1, 0, 1, 128, 255 among them
V3_DELTA_SET = tuple(sorted({s * v for m in range(8) for v in (1 << m, (2 << m) - 1) for s in (-1, 1)} | {0}))


def _nblk(w, h):
    return (w // 16) * (h // 16) * 6


def _ac_levels(cls, nblk, rng, turn):
    """(levels (nblk, 64) with column 0 left 0, forced (block, position) pairs or None)"""
    lv = np.zeros((nblk, 64), np.int64)
    forced = None
    if cls == "dense":                               # all 63 non-zero, uniform in -512..511
        a = rng.integers(-512, 511, (nblk, 63))
        lv[:, 1:] = np.where(a >= 0, a + 1, a)
    elif cls == "extremes":
        lv[:, 1:] = rng.choice(np.array([-512, -511, -1, 1, 510, 511]), (nblk, 63))
    elif cls in ("sparse", "zeros"):                 # about 8 % non-zero and small: table codes and long runs
        mag = np.minimum(rng.geometric(0.5, (nblk, 63)), 12) * rng.choice(np.array([-1, 1]), (nblk, 63))
        lv[:, 1:] = np.where(rng.random((nblk, 63)) < 0.08, mag, 0)
        if cls == "zeros":                           # escapes of level 0: first, last and neighbouring positions, and a random one
            forced = set()
            for b in range(nblk):
                ks = {(1, 2, 63)[(b + turn) % 3], int(rng.integers(1, 64)), int(rng.integers(1, 64))}
                if b % 4 == 0:
                    ks |= {62, 63}
                for k in ks:
                    lv[b, k] = 0
                    forced.add((b, k))
    elif cls == "last":                              # one coefficient at position 63: a run of 62, which only an escape can carry
        a = rng.integers(-512, 511, nblk)
        lv[:, 63] = np.where(a >= 0, a + 1, a)
    elif cls == "codes":                             # every table code with either sign, in table order, as many as a block holds
        pairs = [(r, s * l) for (r, l) in books()[0] for s in (1, -1)]
        i = (turn * 37) % len(pairs)
        for b in range(nblk):
            k = 0
            while k + pairs[i][0] + 1 <= 63:
                k += pairs[i][0] + 1
                lv[b, k] = pairs[i][1]
                i = (i + 1) % len(pairs)
    elif cls == "runs":                              # one coefficient per block after a run of 0..62
        for b in range(nblk):
            run = (b + turn * 6) % 63
            lv[b, run + 1] = (1, -1, 2, -3, 40, -512, 511)[(b + turn) % 7]
    else:
        assert cls == "empty"
    return lv, forced


def _dc_column(version, wrap, nblk, rng, mode, turn):
    """column 0: v2 levels or v3 deltas.  mode 0: uniform; 1: the set, in turn per component; 2 (v3): a run of maximal deltas of one sign"""
    if version == 2:
        if mode == 0:
            return rng.integers(-512, 511, nblk)                     # -512..510: 511 is 0x1FF, the end code
        return np.array([V2_DC_SET[(b + turn) % len(V2_DC_SET)] for b in range(nblk)])
    if mode == 0:
        return rng.integers(-255, 256, nblk)
    if mode == 2:
        return np.full(nblk, 255 if turn % 2 == 0 else -255)
    out, at = np.zeros(nblk, np.int64), [5 * turn, 5 * turn + 11, 5 * turn + 17]
    for b in range(nblk):
        c = min(b % 6, 2)
        out[b] = V3_DELTA_SET[at[c] % len(V3_DELTA_SET)]
        at[c] += 1
    return out


class Written:
    """what the writer was given and what it recorded, kept beside a case for the coverage checks"""

    def __init__(self, cls, policy, version, wrap, given, running, writer):
        self.cls, self.policy, self.version, self.wrap = cls, policy, version, wrap
        self.given, self.running = given, running
        self.escapes, self.table_codes, self.dc_classes = writer.escapes, writer.table_codes, writer.dc_classes
        self.block_bits = writer.block_bits


def _sized(data, turn):
    """the three frame sizes in turn: the bytes written (even), one junk byte more (odd), rounded up to 4 with zeros.
    Returns (buffer, size, what was done: "exact", "junk", "fill" -- or "no fill" where the count was a multiple of 4 already)."""
    raw = np.frombuffer(data, np.uint8)
    assert raw.size % 2 == 0
    if turn % 3 == 0:
        return raw, raw.size, "exact"
    if turn % 3 == 1:
        return np.concatenate([raw, np.array([0xFF], np.uint8)]), raw.size + 1, "junk"
    n = (raw.size + 3) & ~3
    return np.concatenate([raw, np.zeros(n - raw.size, np.uint8)]), n, "fill" if n > raw.size else "no fill"


def make_case(name, w, h, version, wrap, given, quant_scale, policy, turn, cls="", seed=0):
    """(Case, (0, levels, quant scale, version, bits)) for one written frame; case.written keeps what the writer recorded"""
    pol = ("p", 0.3, seed) if policy == "p30" else policy
    data, nbits, writer = write(given, version, quant_scale, wrap, pol, return_writer=True)
    levels, running = expected_levels(given, version, wrap)
    buf, size, sizing = _sized(data, turn)
    case = Case(name, w, h, wrap, buf, size)
    case.written = Written(cls, policy, version, wrap, given, running, writer)
    case.written.sizing, case.written.bytes_written = sizing, len(data)
    return case, (0, levels, quant_scale, version, nbits)


@functools.lru_cache(maxsize=None)
def clean_cases(seed=20261018):
    """[(Case, expected)]: v2 / v3 / v3dc x 16x16, 48x32, 64x64 x the block classes x the escape policies x the header scales.
    DC content and frame size go round with the case number, so that each occurs with each codec, class and frame size."""
    rng = np.random.default_rng(seed)
    out = []
    for (version, wrap) in CODECS:
        for (w, h) in SIZES:
            nblk = _nblk(w, h)
            for ci, cls in enumerate(BLOCK_CLASSES):
                policies = POLICIES if cls not in ("empty", "zeros") else ("needed",)      # no AC to escape / the policy is the set
                for pi, policy in enumerate(policies):
                    for si, qs in enumerate(SCALES):
                        turn = len(out)
                        given, forced = _ac_levels(cls, nblk, rng, turn)
                        mode = (ci + pi + si) % (2 if version == 2 else 3)
                        given[:, 0] = _dc_column(version, wrap, nblk, rng, mode, si)
                        name = "v%d%s %dx%d %s %s qs%d dc%d" % (version, "dc" if wrap else "", w, h, cls, policy, qs, mode)
                        out.append(make_case(name, w, h, version, wrap, given, qs, forced if forced is not None else policy,
                                             turn, cls, seed=seed + turn))
                        out[-1][0].written.policy = "at" if forced is not None else policy
    return tuple(out)


@functools.lru_cache(maxsize=None)
def large_cases(seed=20261019):
    """320x240: one frame each of v2 and v3dc whose 1800 blocks are 63 escapes long (about 316 KB: 10 + 63 * 22 + 2 bits in v2; in
    v3dc every DC is a maximal delta, 15 bits for luma and 16 for chroma, the longest block the syntax has: 1404 bits), and one
    frame of empty blocks (12 bits each in v2)"""
    rng = np.random.default_rng(seed)
    w, h = 320, 240
    out = []
    for (version, wrap) in ((2, 0), (3, 1)):
        given, _ = _ac_levels("dense", _nblk(w, h), rng, 0)
        given[:, 0] = _dc_column(version, wrap, _nblk(w, h), rng, 0 if version == 2 else 2, 0)
        out.append(make_case("v%d%s 320x240 dense always" % (version, "dc" if wrap else ""), w, h, version, wrap, given, 1,
                             "always", 0, "dense"))
    given = np.zeros((_nblk(w, h), 64), np.int64)
    given[:, 0] = _dc_column(2, 0, _nblk(w, h), rng, 0, 0)
    out.append(make_case("v2 320x240 empty", w, h, 2, 0, given, 1, "needed", 0, "empty"))
    return tuple(out)


def _sparse_frame(w, h, rng):
    given, _ = _ac_levels("sparse", _nblk(w, h), rng, 0)
    given[:, 0] = rng.integers(-100, 101, _nblk(w, h))
    return given


@functools.lru_cache(maxsize=None)
def negative_cases(seed=20261020):
    """[(Case, status or None)]: a v2 DC of 0x1FF (-3), an escape whose run leads past 63 (-6), the other version's end code (-7),
    and frames cut before their end code, whose status (None here) is whatever the oracle says"""
    rng = np.random.default_rng(seed)
    out = []
    for (w, h) in SIZES[:2]:
        nblk = _nblk(w, h)
        for (version, wrap) in CODECS:
            tag = "v%d%s %dx%d" % (version, "dc" if wrap else "", w, h)
            given = _sparse_frame(w, h, rng)

            def frame(**hooks):
                bw, at = _write_blocks(given, version, 7, "needed", **hooks)
                return bw.finish() + (at,)

            if version == 2:
                for b in (0, nblk // 2, nblk - 1):
                    data, _, _ = frame(raw_v2_dc={b: 0x1FF})
                    out.append((Case(tag + " DC 0x1FF in block %d" % b, w, h, wrap, np.frombuffer(data, np.uint8)), -3))
            for b, how in ((0, lambda last: 63 - last), (nblk - 1, lambda last: 63), (nblk // 2, lambda last: 63 - last)):
                data, _, _ = frame(overrun=(b, how))
                out.append((Case(tag + " run past 63 in block %d" % b, w, h, wrap, np.frombuffer(data, np.uint8)), -6))
            data, _, _ = frame(end_code=END_CODE[5 - version])
            out.append((Case(tag + " the other version's end code", w, h, wrap, np.frombuffer(data, np.uint8)), -7))
            data, _, at = frame()
            first = 8 + 2 * (at >> 4)                                   # the byte offset of the word the end code starts in
            raw = np.frombuffer(data, np.uint8)
            assert first + 2 <= raw.size
            for size in sorted({first - 1, first, first + 1, raw.size - 1}):   # (none holds the whole end code)
                out.append((Case(tag + " cut at %d of %d" % (size, raw.size), w, h, wrap, raw, size), None))
    return tuple(out)
