"""Streams for the decoder's tests: clean ones from the CPU oracle's encoder, and a seeded corrupted corpus made from them.

Everything here comes from the oracle (oracle/, through oracle_lib) and numpy; nothing of the product is run.  Not a conftest
and not a test: imported by tests/test_mdec_parse_cpu.py, tests/test_mdec_recon_ref.py and tests/test_gpu_mdec_decode.py.

A case is a Case(name, w, h, wrap, data, size): `size` bytes of `data` are the frame, decoded as w x h with the v3dc wrap on or
off.  oracle_decode() is what the product is held to.  One thing about it: the oracle's reader fetches whole 16-bit words, so at an
odd size it looks at the byte after the frame; the product reads bytes past the end as zero (csrc/mdec_parse.h), and
oracle_decode() hands the oracle a copy of the frame followed by zeros, which makes the oracle say the same thing.
"""
import functools
import os
import sys

import numpy as np

import oracle_lib as O

ROOT = O.ROOT


class Case:
    def __init__(self, name, w, h, wrap, data, size=None):
        self.name, self.w, self.h, self.wrap = name, w, h, int(wrap)
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.size = self.data.size if size is None else int(size)
        assert 0 <= self.size <= self.data.size

    @property
    def nblk(self):
        return (self.w // 16) * (self.h // 16) * 6


def oracle_decode(case):
    """(status, levels (blocks, 64) int16, quant scale, version, bits consumed) from orc_mdec_decode_frame"""
    buf = np.zeros(case.size + 2, np.uint8)
    buf[:case.size] = case.data[:case.size]
    return O.mdec_decode(case.w, case.h, buf[:case.size], v3dc_wrap=case.wrap)


def _encode(codec, w, h, frames, budget):
    """[(row, bytes used, scale)] of the frames that fit"""
    out, res, rc = O.mdec_encode(codec, w, h, frames, budget)
    assert rc in (0, -2), rc
    return [(out[i], int(res[i, 1]), int(res[i, 0])) for i in range(frames.shape[0]) if 1 <= res[i, 0] <= 63]


@functools.lru_cache(maxsize=None)
def clean_cases():
    """oracle encodes for v2 / v3 / v3dc at several sizes, budgets and amplitudes; the special frames of the golden set; the hard
    content of tests/mdec_hard_content.py.  Every other case is cut at the bytes the encoder used, the rest keep the whole zero-filled
    budget row.  Returns [(Case, source NV21 frame)]."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_mdec_golden import special_frames
    import mdec_hard_content as HC
    cases = []

    def add(name, codec, w, h, frames, budget):
        frames = np.ascontiguousarray(frames)
        out, res, rc = O.mdec_encode(codec, w, h, frames, budget)
        assert rc in (0, -2), rc
        for i in range(frames.shape[0]):
            if not 1 <= res[i, 0] <= 63:
                continue
            size = min(int(res[i, 1]), budget) if len(cases) & 1 else budget      # (bytes used are rounded up to 4)
            cases.append((Case("%s #%d" % (name, i), w, h, codec == 2, out[i, :budget], size), frames[i]))

    for codec in (0, 1, 2):
        for (w, h, n) in ((16, 16, 3), (48, 32, 3), (320, 240, 2), (640, 480, 1)):
            for budget in (4096, 8191, 32768):
                for amp in (0, 4, 8, 40):
                    fr = O.synth_frames(w, h, n, seed=100 + amp, amp=amp, first=3)
                    add("synth c%d %dx%d b%d a%d" % (codec, w, h, budget, amp), codec, w, h, fr, budget)
        for (w, h, budget) in ((48, 32, 4096), (320, 240, 30000), (320, 240, 9000)):
            add("special c%d %dx%d b%d" % (codec, w, h, budget), codec, w, h, special_frames(w, h), budget)
    for f in HC.catalogue():
        for codec in f.codecs:
            need = f.need(codec)
            for s in (1, 12):
                budget = int(need[s]) + 4
                if budget <= 80000:
                    add("hard c%d %s s%d" % (codec, f.name, s), codec, f.w, f.h, f.frame[None, :], budget)
    assert len(cases) > 200
    assert {c.wrap for c, _ in cases} == {0, 1}
    return tuple(cases)


def _flip(data, bit):
    data[bit >> 3] ^= 0x80 >> (bit & 7)


@functools.lru_cache(maxsize=None)
def corrupted_cases(seed=20261016):
    """The corrupted corpus: truncations at every byte of a short frame, single and burst bit flips, wrong magic and wrong version,
    an all-zero row, an all-ones row, sizes below 8 -- and, so that every error the syntax has is met on purpose and not by luck of
    the flips: a valid header over an all-ones payload (runs past coefficient 63), a frame read with more blocks than it has (the
    end code where a DC belongs) and with fewer (a DC where the end code belongs).  Untouched streams ride along as the clean
    decodes."""
    rng = np.random.default_rng(seed)
    short = {}
    for codec in (0, 1, 2):
        for (w, h, amp, budget) in ((16, 16, 30, 2048), (48, 32, 12, 4096), (64, 64, 6, 4096)):
            fr = O.synth_frames(w, h, 1, seed=55 + codec, amp=amp, first=1)
            row, used, _ = _encode(codec, w, h, fr, budget)[0]
            used = min(used, budget)
            short[(codec, w, h)] = (row[:budget].copy(), used)
    cases = []
    for (codec, w, h), (row, used) in sorted(short.items()):
        wrap = codec == 2
        tag = "c%d %dx%d" % (codec, w, h)
        cases.append(Case(tag + " clean", w, h, wrap, row, used))
        cases.append(Case(tag + " clean, whole row", w, h, wrap, row))
        if (w, h) == (16, 16):
            for n in range(used + 1):
                cases.append(Case(tag + " cut at %d" % n, w, h, wrap, row[:used], n))
        for i in range(60):
            d = row[:used].copy()
            _flip(d, int(rng.integers(64, used * 8)))
            cases.append(Case(tag + " flip %d" % i, w, h, wrap, d))
        for i in range(40):
            d = row[:used].copy()
            start = int(rng.integers(64, used * 8 - 64))
            for b in range(start, start + int(rng.integers(2, 65))):
                if rng.integers(0, 2):
                    _flip(d, b)
            cases.append(Case(tag + " burst %d" % i, w, h, wrap, d))
        for i in range(8):                                # flips in the header
            d = row[:used].copy()
            _flip(d, int(rng.integers(0, 64)))
            cases.append(Case(tag + " header flip %d" % i, w, h, wrap, d))
        d = row[:used].copy(); d[3] = 0x39
        cases.append(Case(tag + " wrong magic", w, h, wrap, d))
        d = row[:used].copy(); d[2] = 0x01
        cases.append(Case(tag + " wrong magic, low byte", w, h, wrap, d))
        for v in (0, 1, 4, 0x0302):
            d = row[:used].copy(); d[6] = v & 255; d[7] = v >> 8
            cases.append(Case(tag + " version %d" % v, w, h, wrap, d))
        cases.append(Case(tag + " all-zero row", w, h, wrap, np.zeros(used, np.uint8)))
        cases.append(Case(tag + " all-ones row", w, h, wrap, np.full(used, 255, np.uint8)))
        for n in range(8):
            cases.append(Case(tag + " size %d" % n, w, h, wrap, row[:used], n))
        d = np.full(used, 255, np.uint8); d[:8] = row[:8]
        cases.append(Case(tag + " header + ones", w, h, wrap, d))
        d = np.zeros(used, np.uint8); d[:8] = row[:8]
        cases.append(Case(tag + " header + zeros", w, h, wrap, d))
        cases.append(Case(tag + " read as 16 more rows", w, h + 16, wrap, row[:used]))
        if h > 16:
            cases.append(Case(tag + " read as 16 fewer rows", w, h - 16, wrap, row[:used]))
    return tuple(cases)


# status codes the syntax can produce, per version.  -8 ("the end code lies past the last byte") is in the oracle's text but cannot
# happen: both end codes end in a 1 bit, bits past the end read as 0, so an end code that matched ended inside the frame.
REACHABLE = {2: {0, -1, -2, -3, -5, -6, -7}, 3: {0, -1, -2, -4, -5, -6, -7}}


def check_corpus_reaches_every_error(cases, statuses):
    """the oracle's answers over the corpus include every reachable code per codec, clean decodes among them"""
    seen = {2: set(), 3: set()}
    for c, st in zip(cases, statuses):
        ver = 2 if c.name.startswith("c0") else 3
        seen[ver].add(int(st))
    for ver in (2, 3):
        assert seen[ver] == REACHABLE[ver], (ver, sorted(seen[ver]))
    assert -3 not in seen[3] and -4 not in seen[2]
