"""The sound-bank tests' banks ("psxhip SPU bank v1"): the entry lists, a restatement of the layout rule in
Python, the expected bank bytes -- ref_spu_file of tests/golden/make_spufile_golden.py per entry (the REFERENCE's encoder driven
through the reference's framing loop), placed by the restated plan -- and the corruptions the check kernel has to name.

Test infrastructure only: shared by tests/test_spu_bank_plan_cpu.py, tests/test_spu_bank_lanes_cpu.py and tests/test_gpu_spu_bank.py."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np

import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_spufile_golden as G  # noqa: E402

SPU, VAG = 2, 3
HEADER, DUMMY, FLAGS, TRAP, PADDING = 1, 2, 4, 8, 16
LOOP_REPEAT, LOOP_START, LOOP_TRAP = 3, 6, 5
TILE = 4096


def entry(samples, freq=44100, loop=-1, enable_loop=False, name="", pcm_offset=0):
    return dict(pcm_offset=pcm_offset, samples=samples, freq=freq, loop=loop, enable_loop=bool(enable_loop), name=name)


def settings(fmt=SPU, alignment=64, no_dummy=False, bank_alignment=16, beam=0):
    return dict(fmt=fmt, alignment=alignment, no_dummy=bool(no_dummy), bank_alignment=bank_alignment, beam=beam)


def placed(entries, gap=3):
    """the entries with PCM offsets of their own: one behind the other, `gap` samples apart (odd: offsets of both parities)"""
    out, at = [], 1
    for e in entries:
        out.append(dict(e, pcm_offset=at))
        at += e["samples"] + gap
    return out


def pcm_elements(entries):
    return max([e["pcm_offset"] + e["samples"] for e in entries] + [0])


def blocks_of(e):
    return -(-e["samples"] // 28)


def loop_ms(kind, samples, freq):
    """a loop point in milliseconds that falls on no block (none), block 0, a middle block, the last block, or behind the end"""
    blocks = -(-samples // 28)
    block = {"zero": 0, "inside": blocks // 2, "last": max(blocks - 1, 0)}.get(kind)
    if kind == "none":
        return -1
    if kind == "beyond":
        return -(-blocks * 28000 // freq) + 5
    ms = -(-block * 28000 // freq)
    assert kind == "inside" or ms * freq // 28000 == block, "a millisecond is more than a block at this rate"
    return ms


def mixed_entries():
    """about 40 entries: every length of the sweep with every kind of loop point, loops on and off (samples == 0 both ways), names of
    0, 5 and 16 characters, three rates; a few longer ones behind them"""
    out, k = [], 0
    names, freqs = ["", "snare", "sixteen_chars_xy"], [11025, 22050, 44100]
    for samples in (0, 1, 27, 28, 29, 56, 1125):
        for kind in ("none", "zero", "inside", "last", "beyond"):
            freq = freqs[k % 3] if kind != "last" else freqs[k % 2]      # (at 44100 Hz a millisecond steps over blocks)
            out.append(entry(samples, freq, loop_ms(kind, samples, freq), k % 2 == 0, names[(k // 2) % 3]))
            k += 1
    out.append(entry(300, 44100, loop_ms("inside", 300, 44100), True, "tom"))
    out.append(entry(2000, 22050, loop_ms("last", 2000, 22050), False, "long_name_of_16c"))
    out.append(entry(0, 11025, -1, True, "empty"))
    out.append(entry(0, 11025, 0, False, ""))
    out.append(entry(8000, 11025, loop_ms("inside", 8000, 11025), True, "pad"))
    return placed(out)


def synth(entries, seed=41):
    """a PCM buffer that holds every entry's samples at its offset (the material of oracle/synth.c, a kind per entry), 0x5A5A elsewhere"""
    pcm = np.full(pcm_elements(entries) + 2, 0x5A5A, np.int16)
    for i, e in enumerate(entries):
        if e["samples"]:
            pcm[e["pcm_offset"]:e["pcm_offset"] + e["samples"]] = O.synth_pcm(seed, i, 0, e["samples"], i % 5)
    return pcm


# ---- the rule, restated
def file_size(s, e):
    body = (int(not s["no_dummy"]) + blocks_of(e) + int(not e["enable_loop"])) * 16
    return (48 if s["fmt"] == VAG else 0) + -(-body // s["alignment"]) * s["alignment"]


def plan(s, entries):
    """offsets, sizes, total, and per entry the numbers of psxhip_spu_bank_row_t (without the header bytes), the unit base and tiles"""
    offsets, sizes, at = [], [], 0
    for e in entries:
        offsets.append(at)
        sizes.append(file_size(s, e))
        at = -(-(at + sizes[-1]) // s["bank_alignment"]) * s["bank_alignment"]
    total, rows, base, tiles = at, [], [], []
    for i, e in enumerate(entries):
        blocks, hw, dummy = blocks_of(e), 3 if s["fmt"] == VAG else 0, int(not s["no_dummy"])
        start = e["loop"] * e["freq"] // 28000 if e["loop"] >= 0 else -1
        end = (offsets[i + 1] if i + 1 < len(entries) else total) // 16
        rows.append((offsets[i] // 16, hw, dummy, blocks, int(not e["enable_loop"]), end, start if 0 <= start < blocks else -1,
                     int(e["enable_loop"] and blocks > 0)))
        base.append(offsets[i] // 16 + hw + dummy)
        frame_words = end - offsets[i] // 16 - blocks
        tiles += [(i, 0, w, min(TILE, frame_words - w)) for w in range(0, frame_words, TILE)]
        tiles += [(i, 1, b, min(TILE, blocks - b)) for b in range(0, blocks, TILE)]
    return dict(offsets=offsets, sizes=sizes, total=total, rows=rows, unit_base=base, tiles=tiles)


# ---- the expected bytes
class _OracleAsRef:
    """oracle/adpcm_oracle.c behind the reference's signature, where oracle/_ref is absent (a machine without the reference tree); the
    oracle is held to the reference build by tests/test_adpcm_oracle.py"""
    @staticmethod
    def psx_audio_spu_encode(state, samples, n, pitch, out):
        st = state._obj
        c = O.Chan(st.prev1, st.prev2)
        ln = O.lib().orc_spu_encode(C.byref(c), samples, n, pitch, out)
        st.prev1, st.prev2 = c.prev1, c.prev2
        return ln


@contextlib.contextmanager
def _encoder():
    """ref_spu_file asks oracle_lib.ref() for its encoder: the reference build when it is there"""
    if O.ref() is not None:
        yield
        return
    keep, O.ref = O.ref, lambda: _OracleAsRef
    try:
        yield
    finally:
        O.ref = keep


def ref_file(s, e, pcm):
    """the reference's file for one entry (psx_audio_spu_encode 28 samples a call inside the framing loop of filefmt.c:212-293)"""
    x = pcm[e["pcm_offset"]:e["pcm_offset"] + e["samples"]]
    with _encoder():
        return G.ref_spu_file(s["fmt"], x, freq=e["freq"], alignment=s["alignment"], loop_point=e["loop"], enable_loop=e["enable_loop"],
                              no_dummy=s["no_dummy"], name=e["name"])


def ref_bank(s, entries, pcm):
    """the whole bank: every entry's reference file at its offset, zeros between and behind"""
    p = plan(s, entries)
    bank = np.zeros(p["total"], np.uint8)
    for e, at, size in zip(entries, p["offsets"], p["sizes"]):
        f = ref_file(s, e, pcm)
        assert f.size == size, (f.size, size)
        bank[at:at + size] = f
    return bank, p


def data_only(bank, p, fill=0xA5):
    """what the encoder leaves in a buffer that held `fill`: the data blocks alone, byte 1 zero"""
    out = np.full(bank.size, fill, np.uint8)
    for (first, hw, dummy, blocks, *_), base in zip(p["rows"], p["unit_base"]):
        out[16 * base:16 * (base + blocks)] = bank[16 * base:16 * (base + blocks)]
        out[16 * base + 1:16 * (base + blocks):16] = 0
    return out


def corruptions(s, entries, p):
    """[(what, entry, byte offset in the bank, xor mask, the one bit it must raise)]: one per kind, each on an entry that has the thing"""
    out = []
    rows, offs, sizes = p["rows"], p["offsets"], p["sizes"]

    def add(what, cond, at, mask, bit):
        i = next((i for i, r in enumerate(rows) if cond(i, r)), None)       # (a bank without such an entry goes without the corruption)
        if i is not None:
            out.append((what, i, at(i, rows[i]), mask, bit))
    if s["fmt"] == VAG:
        add("header byte", lambda i, r: True, lambda i, r: offs[i] + 0x21, 0x01, HEADER)
        add("frequency field", lambda i, r: r[3] > 2, lambda i, r: offs[i] + 0x12, 0x40, HEADER)
    if not s["no_dummy"]:
        add("dummy byte", lambda i, r: r[3] > 0, lambda i, r: 16 * (r[0] + r[1]) + 9, 0x80, DUMMY)
    add("stray flag on a middle block", lambda i, r: r[3] > 8 and r[6] != r[3] // 2, lambda i, r: 16 * (p["unit_base"][i] + r[3] // 2) + 1, 0x02, FLAGS)
    add("missing LOOP_START", lambda i, r: r[6] >= 0, lambda i, r: 16 * (p["unit_base"][i] + r[6]) + 1, 0x04, FLAGS)
    add("trap byte", lambda i, r: r[4] == 1, lambda i, r: 16 * (p["unit_base"][i] + r[3]) + 1, 0x01, TRAP)
    add("pad byte", lambda i, r: sizes[i] > (48 if s["fmt"] == VAG else 0) + 16 * (r[2] + r[3] + r[4]), lambda i, r: offs[i] + sizes[i] - 1, 0x10, PADDING)
    gaps = [i for i in range(len(rows)) if 16 * rows[i][5] > offs[i] + sizes[i]]
    if gaps:
        i = gaps[len(gaps) // 2]
        out.append(("gap byte", i, 16 * rows[i][5] - 3, 0xFF, PADDING))
    return out


# the bank-level settings the mixed entries are framed under: both formats, dummy on and off, alignments 16 / 64 / 2048, bank
# alignments 16 / 2048
MIXED_SETTINGS = [settings(SPU, 64, False, 16), settings(VAG, 16, False, 2048), settings(SPU, 2048, True, 16), settings(VAG, 64, True, 2048)]
