"""The loop-seam tests' bank ("psxhip SPU loop seam v1"): 24 looping and non-looping entries of deterministic
numpy material that is exactly periodic over the body (a few partials with whole numbers of cycles over the body's samples, with
and without noise that repeats with the body), amplitudes 100 .. 32000, sample counts 28, 29, 56, 300 and 1125, the seam block at 0,
in the middle and in the last block; an entry without a loop, a loop point behind the end, a loop point without enable_loop, and
enable_loop without a loop point (the settings of tests/spu_bank_corpus.py frame the bank with and without the leading dummy).

The seeds are fixed so that, under the statement (tests/spu_seam_ref.py) and beam 0, the bank holds entries fixed at pass 0, entries
fixed at pass 2 or later and entries without a fixed point within the passes; and so that, under beam 0 and beam 2, every entry
fixed at a pass k > 0 is one whose seam report says `settled`.  The second condition is a choice of material, not a property of the
rule: the first time through, the decoder enters the body with s_0 and not with the s_k the kept pass was planned from, and about
half of the seeds tried for a short body gave an entry that is fixed and not settled (DESIGN.md section 24;
tests/test_spu_seam_ref.py keeps one such body as a counter-example).  Both conditions are asserted there, from the statement alone.

Test infrastructure only: shared by the seam tests."""
import functools

import numpy as np

import spu_bank_corpus as B
import spu_seam_ref as S

MIXED_SETTINGS = B.MIXED_SETTINGS
SEED = 2406

# (samples, where the loop point falls, enable_loop, partials, amplitude, noise amplitude, seed)
RECIPES = (
    [(samples, kind, True, 1 + (k + j) % 4, (100, 900, 6000, 32000, 2500)[(k + j) % 5], (0, 40, 0, 300)[(k + 2 * j) % 4], 10 * k + j)
     for k, samples in enumerate((28, 29, 56, 300, 1125)) for j, kind in enumerate(("zero", "inside", "last"))] +
    [(300, "none", False, 2, 4000, 20, 100),            # no loop
     (300, "beyond", True, 3, 12000, 0, 101),           # a loop point behind the end
     (1125, "inside", False, 2, 800, 50, 102),          # a loop point without enable_loop
     (300, "none", True, 4, 20000, 100, 103),           # enable_loop without a loop point
     (1125, "none", True, 1, 100, 0, 104),
     (300, "inside", True, 4, 15000, 200, 105),
     (1125, "zero", True, 3, 3000, 0, 106),
     (1125, "last", True, 2, 28000, 500, 107),
     (29, "zero", True, 1, 100, 0, 108)])
# Seeds of their own for three entries (see the module's text: every entry fixed at a pass k > 0 is also settled)
for _i, _seed in ((1, 323), (10, 502), (20, 700)):
    RECIPES[_i] = RECIPES[_i][:6] + (_seed,)


def entries():
    out = []
    for k, (samples, kind, enable_loop, _, _, _, _) in enumerate(RECIPES):
        freq = (22050, 11025)[k % 2]
        out.append(B.entry(samples, freq, B.loop_ms(kind, samples, freq), enable_loop, "s%d" % k))
    return B.placed(out)


def material(samples, first, partials, amplitude, noise, seed):
    """`samples` samples whose part from `first` on is one period of everything in it"""
    rng = np.random.default_rng(SEED * 1000 + seed)
    n = samples - first
    i = np.arange(samples) - first
    x = np.zeros(samples)
    for c, w in zip(rng.choice(np.arange(1, max(2, n // 6) + 1), partials, replace=partials > max(2, n // 6)), rng.uniform(0.3, 1.0, partials)):
        x += w * np.sin(2 * np.pi * c * i / n + rng.uniform(0, 2 * np.pi))
    x *= amplitude / max(np.abs(x).max(), 1e-9)
    if noise:
        x += rng.integers(-noise, noise + 1, n)[i % n]
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def synth(ents):
    """the PCM buffer: every entry's material at its offset, 0x5A5A elsewhere.  The period starts at the loop-start block the entry
    names (whether or not the settings make it the seam block)"""
    pcm = np.full(B.pcm_elements(ents) + 2, 0x5A5A, np.int16)
    for e, (samples, _, _, partials, amplitude, noise, seed) in zip(ents, RECIPES):
        start = e["loop"] * e["freq"] // 28000 if e["loop"] >= 0 else 0
        first = 28 * start if 28 * start < samples else 0
        pcm[e["pcm_offset"]:e["pcm_offset"] + samples] = material(samples, first, partials, amplitude, noise, seed)
    return pcm


@functools.lru_cache(maxsize=None)
def bank():
    ents = entries()
    return ents, synth(ents)


@functools.lru_cache(maxsize=None)
def expected(k, beam, mode):
    """MIXED_SETTINGS[k]: (the bank's bytes, the restated plan, the seam blocks, the outcomes or None): the framing is the reference's
    (tests/spu_bank_corpus.py), the data blocks the statement's"""
    ents, pcm = bank()
    s = MIXED_SETTINGS[k]
    framed, p = B.ref_bank(s, ents, pcm)
    seams = [S.seam_block(s, e) for e in ents]
    if beam < 2 and mode == S.OFF:
        return framed, p, seams, None
    blocks, outcome = S.encode_entries([S.padded(e, pcm) for e in ents], seams, beam, mode)
    out = framed.copy()
    for base, blk in zip(p["unit_base"], blocks):
        flags = out[16 * base + 1:16 * (base + len(blk)):16].copy()
        out[16 * base:16 * (base + len(blk))] = blk.reshape(-1)
        out[16 * base + 1:16 * (base + len(blk)):16] = flags
    out.setflags(write=False)
    return out, p, seams, outcome
