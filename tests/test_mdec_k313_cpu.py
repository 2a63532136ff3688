"""mdec-k3.13 (NOTEBOOK, "mdec-k3.13"), without a GPU: the arithmetic behind the frame kernel's doubled coefficients and behind the
end-of-block code that rides in front of every DC slot, against the oracle's rules (oracle/mdec_oracle.c), and the listing of the
six product instantiations (stats off) of the frame kernel, built with the flags of tests/test_kernel_resources.py.

* The coefficient tile holds v' = 2 n + b: n = acc >> 17 is the coefficient, b the accumulator's bit below it (acc >> 16 is one
  byte permute; the packed shift that made acc >> 17 of it is gone).  A code-list entry keeps 2 n in its low 17 bits.
* build_list() tests the doubled value against doubled constants, and the quantisers hold half the reciprocal.
* chunk() takes an entry's scan position as e >> 17, and a one-chunk list's lane 0 gets its predecessor 0 from the DPP's zero fill.
* Every DC slot carries an end-of-block code in front, the first one the PREVIOUS macroblock's last: a macroblock's stream lies two
  bits earlier, the two bits in front of the frame's first macroblock are dropped, and the finisher writes the last end-of-block
  code together with the end-of-frame code.

Static figures, (codec, wavefronts): vector instructions from the column read to the coefficient tile's write, and in the innermost
loop around the third v_mfma, parent (commit f6570fe) -> this revision, are in PARENT_* below and printed by the tests."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

import mdec_hard_content as H
import oracle_lib as O
import test_kernel_resources as R
import test_mdec_k311_resources as K
import test_mdec_k312_cpu as K12
import wave_probe_ref as W

sys.path.insert(0, os.path.join(O.ROOT, "tools"))
import gen_tables as G      # noqa: E402

QUANT_SCAN = H.luts()[2].astype(np.int64)          # the quantisation matrix in scan order ([0]: the DC slot's placeholder)


# ---------------------------------------------------------------- the quantiser on doubled operands
def fma32(a, b, c):
    """fp32 fma of float32 arrays: product and sum are exact in float64 at these sizes (a is an integer below 2^15, b has 24
    significant bits, the sum spans fewer than 53 bits), so one rounding to float32 is the fma's"""
    a, b, c = np.asarray(a, np.float32), np.float32(b), np.float32(c)
    return (a.astype(np.float64) * np.float64(b) + np.float64(c)).astype(np.float32)


def quant_parent(mag, d):
    inv = np.float32(1.0) / np.float32(d)
    bias = fma32(np.float32(0.25), inv, np.float32(0.5))
    return np.trunc(fma32(mag, inv, bias)).astype(np.int64)


def quant_doubled(mag2, d):
    """make_quant_doubled() and quant_mag() on |2 n|"""
    inv = np.float32(0.5) * (np.float32(1.0) / np.float32(d))
    bias = fma32(np.float32(0.5), inv, np.float32(0.5))
    return np.trunc(fma32(mag2, inv, bias)).astype(np.int64)


def test_the_halved_reciprocal_on_doubled_operands_is_todays_quantiser_bit_for_bit():
    divisors = sorted({int(q) * s for q in G.QUANT[1:] for s in range(1, 64)} | {16})
    mag = np.arange(0, 8193, dtype=np.int64)
    for d in divisors:
        inv = np.float32(1.0) / np.float32(d)
        half = np.float32(0.5) * inv
        assert np.float64(half) * 2.0 == np.float64(inv)                    # halving a float is exact
        assert fma32(np.float32(0.5), half, np.float32(0.5)) == fma32(np.float32(0.25), inv, np.float32(0.5))      # one bias
        a = fma32(mag, inv, fma32(np.float32(0.25), inv, np.float32(0.5)))
        b = fma32(2 * mag, half, fma32(np.float32(0.5), half, np.float32(0.5)))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), d      # the same float before the truncation
        got = quant_doubled(2 * mag, d)
        assert np.array_equal(got, quant_parent(mag, d)), d
        assert np.array_equal(got, (2 * mag + d) // (2 * d)), d             # the oracle's rounding (mdec.c:447-449 in magnitudes)


def test_the_dc_term_at_divisor_32_on_doubled_operands_is_quant_dc():
    c = np.arange(-8192, 8129, dtype=np.int64)
    q = quant_doubled(np.abs(2 * c), 16)              # (lane 0 of the emit quantiser: divisor 16, held as 1 / 32)
    assert np.float32(0.5) * (np.float32(1.0) / np.float32(16)) == np.float32(1.0) / np.float32(32)
    assert np.array_equal(np.where(c < 0, -q, q), (c + 8 + (c >> 63)) >> 4)
    q12, neg12 = K12.quant16_f32(c)
    assert np.array_equal(q, q12)


# ---------------------------------------------------------------- the list's threshold and the entry
def test_the_doubled_threshold_keeps_what_todays_keeps_and_the_entry_holds_2n():
    v = np.arange(-32768, 32768, dtype=np.int64)            # v' = 2 n + b: every n of an int16 tile slot, both b
    n = v >> 1
    assert np.array_equal(2 * n + (v & 1), v)
    u32 = lambda x: x & 0xFFFFFFFF
    thresholds = sorted({(int(q) * s + 1) >> 1 for q in G.QUANT[1:] for s in range(1, 64)})
    assert thresholds[0] == 8 and thresholds[-1] == (int(max(G.QUANT[1:])) * 63 + 1) >> 1
    for T in [1, 2, 3] + thresholds:
        parent = u32(n + T - 1) >= 2 * T - 1
        assert np.array_equal(parent, np.abs(n) >= T)
        doubled = u32(v + 2 * T - 2) >= 4 * T - 2
        assert np.array_equal(doubled, parent), T
    # the entry: (v' & 0x1FFFE) sign-extended from bit 16 is 2 n; bit 16 is the sign; the SDWA convert reads the low word
    e = u32(v) & 0x1FFFE
    assert np.array_equal(e - ((e & 0x10000) << 1), 2 * n)
    assert np.array_equal((e >> 16) & 1, (n < 0).astype(np.int64))
    inside = np.abs(n) <= 8192
    low = e & 0xFFFF
    assert np.array_equal((low - ((low & 0x8000) << 1))[inside], (2 * n)[inside])
    # (and with the mask left at 17 bits the entry would hold v', not 2 n)
    assert not np.array_equal(u32(v) & 0x1FFFF, e)


# ---------------------------------------------------------------- the range
def fdct(blocks):
    out = np.ascontiguousarray(np.asarray(blocks, np.int16).reshape(-1, 64)).copy()
    for i in range(out.shape[0]):
        O.lib().orc_fdct_islow8(O.ptr(out[i], O.i16p))
    return out.astype(np.int64)


def test_the_largest_coefficient_stays_inside_the_tiles_int16_when_doubled():
    rng = np.random.default_rng(313)
    x = (2 * np.arange(8) + 1) * np.pi / 16
    blocks = [np.full((8, 8), -128), np.full((8, 8), 127)]
    for v in range(8):
        for u in range(8):
            pos = np.cos(x * v)[:, None] * np.cos(x * u)[None, :] >= 0
            blocks += [np.where(pos, 127, -128), np.where(pos, -128, 127)]
    blocks += list(np.where(rng.integers(0, 2, (4000, 8, 8)) > 0, 127, -128))
    blocks += list(rng.integers(-128, 128, (2000, 8, 8)))
    co = fdct(np.array(blocks))
    top = int(np.abs(co).max())
    print("largest |coefficient| over %d extreme blocks: %d (DC %d .. %d)" % (co.shape[0], top, co[:, 0].min(), co[:, 0].max()))
    assert top <= 8192 and co[:, 0].min() == -8192 and co[:, 0].max() == 8128
    assert int(np.abs(co[:, 1:]).max()) > 4096                      # (the extreme blocks are extreme)
    assert -32768 <= 2 * co.min() and 2 * co.max() + 1 <= 32767


# ---------------------------------------------------------------- the chunk
def make_list(n, bits, scale):
    """build_list() at `scale` over a macroblock's coefficients n[6][64] (scan order) with the bits below them: entries
    (2 n & 0x1FFFE) | position << 17 of the kept lanes, lane 0 always"""
    d = QUANT_SCAN * scale
    T = (d + 1) >> 1
    out = []
    for b in range(6):
        v = 2 * n[b] + bits[b]
        keep = ((v + 2 * T - 2) & 0xFFFFFFFF) >= 4 * T - 2
        keep[0] = True
        for k in np.nonzero(keep)[0]:
            out.append(((int(v[k]) & 0x1FFFE) | (int(k) << 17)))
    return np.array(out, dtype=np.int64)


def chunk_model(entries, scale):
    """chunk() at the list's own scale over a list of any length, 64 lanes at a time: the first chunk -- and so every one-chunk
    list -- takes lane 0's predecessor from the zero fill, a later chunk from the carry (the previous chunk's lane 63).
    Returns per block the (run, level) pairs of its AC codes"""
    d = QUANT_SCAN * scale
    blocks, carry = [], 0
    for base in range(0, len(entries), 64):
        e = np.full(64, 63 << 17, np.int64)
        live = np.arange(64) + base < len(entries)
        e[live] = entries[base:base + 64]
        k = e >> 17                                       # nothing above bit 22: no mask
        assert k.max() <= 63
        neg = (e >> 16) & 1
        low = e & 0xFFFF
        mag2 = np.abs(low - ((low & 0x8000) << 1))        # the convert's sign-extended low word; the fma takes |.|
        q = np.array([quant_doubled(np.array([m]), 16 if kk == 0 else d[kk])[0] for m, kk in zip(mag2, k)])
        kprev = np.concatenate([[0 if base == 0 else carry], k[:-1]])
        carry = int(k[63])
        run = k - kprev - 1
        for lane in range(64):
            if not live[lane]:
                continue
            if k[lane] == 0:
                blocks.append([])
            else:
                blocks[-1].append((int(run[lane]), int(-q[lane] if neg[lane] else q[lane])))
    return blocks


def oracle_codes(n, scale):
    d = QUANT_SCAN * scale
    out = []
    for b in range(6):
        lv = np.sign(n[b]) * ((2 * np.abs(n[b]) + d) // (2 * d))
        codes, prev = [], 0
        for k in range(1, 64):
            if lv[k]:
                codes.append((k - prev - 1, int(lv[k])))
                prev = k
        out.append(codes)
    return out


def test_the_chunk_on_doubled_entries_gives_the_oracles_runs_and_levels():
    rng = np.random.default_rng(7)
    lengths, carried = set(), 0
    for trial in range(400):
        amp = [3, 12, 60, 400, 4000][trial % 5]
        scale = [1, 2, 5, 20][(trial // 5) % 4]
        n = rng.integers(-amp, amp + 1, (6, 64))
        if trial % 7 == 0:
            n[:, 1:] = 0                                 # six DC slots and nothing else
        if trial % 11 == 0:
            n[rng.integers(0, 6), 63] = 8192 * (1 if trial & 1 else -1)
        bits = rng.integers(0, 2, (6, 64))
        entries = make_list(n, bits, scale)
        lengths.add(len(entries))
        if len(entries) > 64 and (entries[64] >> 17) != 0:
            carried += 1                                 # a later chunk whose lane 0 is not a DC slot: the carry
        assert chunk_model(entries, scale) == oracle_codes(n, scale), (trial, amp, scale)
    print("list lengths %d .. %d, %d lists with a carried predecessor" % (min(lengths), max(lengths), carried))
    assert min(lengths) == 6 and any(l <= 64 for l in lengths) and any(l > 128 for l in lengths) and carried >= 10
    # lists shorter than a macroblock's six slots, 1 .. 64 entries: the model on a prefix of a list is the prefix of the codes
    n = rng.integers(-60, 61, (6, 64))
    entries = make_list(n, rng.integers(0, 2, (6, 64)), 1)
    assert len(entries) > 64
    full = chunk_model(entries[:64], 1)
    for count in range(1, 65):
        part = chunk_model(entries[:count], 1)
        flat_full = [c for blk in full for c in blk]
        flat_part = [c for blk in part for c in blk]
        assert flat_part == flat_full[:len(flat_part)] and len(part) == int(((entries[:count] >> 17) == 0).sum())


# ---------------------------------------------------------------- where the end-of-block codes live
def put(bits, pos, length, code):
    """OR `length` bits of `code` (MSB first) into the bit array at `pos`; positions below 0 are dropped (the merge's g < 2)"""
    for i in range(length):
        if pos + i >= 0:
            bits[pos + i] |= (code >> (length - 1 - i)) & 1


def streams(mbs, eof):
    """mbs: per macroblock six blocks of (length, code) lists, the first the DC code.  Returns (the oracle's layout: every block's
    codes, then its end-of-block code "10"; the end-of-frame code behind the last -- mdec.c:501-503, 647-651 --, this revision's)"""
    sizes = [sum(l for blk in mb for l, _ in blk) + 12 for mb in mbs]
    total = sum(sizes) + 10
    want = np.zeros(total, np.uint8)
    pos = 0
    for mb in mbs:
        for blk in mb:
            for l, c in blk:
                put(want, pos, l, c)
                pos += l
            put(want, pos, 2, 2)
            pos += 2
    put(want, pos, 10, eof)
    assert pos + 10 == total
    got = np.zeros(total, np.uint8)
    prefix = 0
    for mb, size in zip(mbs, sizes):
        pos = prefix - 2                       # scan_offsets(): two bits earlier
        for blk in mb:
            (l0, c0), rest = blk[0], blk[1:]
            put(got, pos, l0 + 2, (2 << l0) | c0)            # every DC slot carries an end-of-block code in front
            pos += l0 + 2
            for l, c in rest:
                put(got, pos, l, c)
                pos += l
        prefix += size                         # a macroblock's bit count is what it was
        assert pos == prefix - 2
    put(got, total - 12, 12, (2 << 10) | eof)  # the finisher: the last end-of-block code and the end-of-frame code
    return want, got


def test_end_of_block_codes_in_front_of_every_dc_slot_give_the_same_stream():
    rng = np.random.default_rng(4)
    for n_mb in (1, 2, 3, 17, 300):
        for eof in (0x1FF, 0x3FF):
            mbs = []
            for _ in range(n_mb):
                mb = []
                for _ in range(6):
                    l0 = 10 if eof == 0x1FF else int(rng.integers(2, 18))          # v2: 10 bits; v3: a VLC of its own length
                    blk = [(l0, int(rng.integers(0, 1 << l0)))]
                    for _ in range(int(rng.integers(0, 9)) if n_mb < 300 else int(rng.integers(0, 3))):
                        l = int(rng.integers(2, 23))
                        blk.append((l, int(rng.integers(0, 1 << l))))
                    mb.append(blk)
                mbs.append(mb)
            want, got = streams(mbs, eof)
            assert np.array_equal(want, got), (n_mb, eof)


def test_the_new_layout_gives_the_oracles_bytes_on_flat_macroblocks():
    """the real oracle: macroblocks flat at different levels are six DC codes and six end-of-block codes each"""
    for nx, ny in ((1, 1), (3, 2)):
        w, h = 16 * nx, 16 * ny
        lu, ch = np.zeros((h, w), np.uint8), np.zeros((h // 2, w), np.uint8)
        for fy in range(ny):
            for fx in range(nx):
                v = (37 * (fy * nx + fx) + 5) & 255
                lu[fy * 16:fy * 16 + 16, fx * 16:fx * 16 + 16] = v
                ch[fy * 8:fy * 8 + 8, fx * 16:fx * 16 + 16] = 255 - v
        frame = np.concatenate([lu.ravel(), ch.ravel()])
        out, res, rc = O.mdec_encode(0, w, h, frame[None, :], 4096)
        assert rc == 0
        coefs = O.mdec_coefs(w, h, frame).astype(np.int64)                  # (6, raster macroblocks, 64)
        mbs = []
        for fx in range(nx):                                                # encode order: fx outer, fy inner
            for fy in range(ny):
                dc = coefs[:, fy * nx + fx, 0]
                assert not coefs[:, fy * nx + fx, 1:].any()
                mbs.append([[(10, int((c + 8 + (c >> 63)) >> 4) & 0x3FF)] for c in dc])
        _, got = streams(mbs, 0x1FF)
        body = out[0, 8:int(res[0, 1])]
        words = body.reshape(-1, 2)[:, ::-1].ravel()                        # 16-bit words, stored low byte first
        have = np.unpackbits(words)[:got.size]
        assert np.array_equal(have, got), (nx, ny)


# ---------------------------------------------------------------- the listing
needs_hipcc = pytest.mark.skipif(not shutil.which(R.HIPCC), reason="hipcc not installed")

# vector instructions at the parent commit f6570fe, read from its listing (same flags): from the column read to the coefficient
# tile's write at each of the three sites (the two pilot macroblocks, the pass loop; the same in all six shapes), and in the
# innermost loop around the third v_mfma
PARENT_COLUMN_VALU = (29, 29, 28)
PARENT_LOOP_VALU = {(0, 12): 243, (0, 16): 244, (1, 12): 1429, (1, 16): 1433, (2, 12): 1429, (2, 16): 1433}
# what this revision takes out of that loop at least.  The loop's text holds every arm; the doubled coefficients take four packed
# shifts out of the column pass and put one v_and per block in front of the count-only and the dense arm's converts (arms the
# headline does not run); the uniform DC slots take out the last-code logic of every chunk form
LOOP_VALU_CLAIM = {(0, 12): 5, (0, 16): 5, (1, 12): 54, (1, 16): 54, (2, 12): 54, (2, 16): 54}


def valu(lines):
    return sum(1 for ln in lines if re.match(r"\s+v_", ln))


@needs_hipcc
def test_no_packed_shift_between_the_column_read_and_the_coefficient_tiles_write():
    for shape, (lines, _) in K.product_shapes().items():
        for stretch, parent in zip(K12.column_stretches(lines), PARENT_COLUMN_VALU):
            shifts = [ln.strip() for ln in stretch if "v_pk_ashrrev_i16" in ln]
            dots = sum("v_dot2_i32_i16" in ln for ln in stretch)
            print(shape, "column read .. tile write: %d vector instructions (parent %d), v_pk_ashrrev_i16: %s" % (valu(stretch), parent, shifts))
            assert dots == 16, (shape, dots)              # it IS the column pass
            assert not shifts, (shape, shifts)
            assert valu(stretch) <= parent - 4, (shape, valu(stretch))


@needs_hipcc
def test_the_pass_loop_issues_fewer_vector_instructions_than_the_parents():
    for shape, (lines, _) in K.product_shapes().items():
        a, b, _ = K.pass_loop(lines)
        v = valu(lines[a:b + 1])
        print(shape, "vector instructions in the loop of lines %d..%d: %d (parent %d)" % (a, b, v, PARENT_LOOP_VALU[shape]))
        assert v <= PARENT_LOOP_VALU[shape] - LOOP_VALU_CLAIM[shape], (shape, v)


@needs_hipcc
def test_product_shapes_have_no_scratch_and_stay_inside_their_ceilings():
    for (codec, waves), (_, u) in K.product_shapes().items():
        print((codec, waves), "VGPRs", u["VGPRs"], "spilled SGPRs", u["SGPRs Spill"])
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0", ((codec, waves), u)
        assert int(u["VGPRs"]) <= (80 if waves == 12 else 128), ((codec, waves), u)
        assert int(u["SGPRs Spill"]) <= R.SGPR_CEILINGS[(codec, waves)][0], ((codec, waves), u)
