"""mdec-k3.12 (NOTEBOOK, "mdec-k3.12"): the frame kernel's column pass lost its two half-swaps and, in v2, the DC quantiser.

* The lanes fetch a block's pixel rows in butterfly order (0, 1, 2, 3, 7, 6, 5, 4), so the column pass's pairs (d7, d6) and
  (d5, d4) are dwords of the transpose tile as they stand.
* The v2 DC term leaves the column pass raw and is quantised in the chunk by the fp32 quantiser every list entry goes through,
  with the divisor 16 in lane 0 of the pass's emit quantiser.

Without a GPU: the arithmetic of both against the oracle (oracle/mdec_oracle.c), and the listing of the six product instantiations
(stats off) of the frame kernel, built with the flags of tests/test_kernel_resources.py.

Static figures, VGPRs / spilled SGPRs per (codec, wavefronts), parent (commit 002230c) -> this revision:
  (0, 12) 80 / 85 -> 80 / 80     (0, 16) 86 / 80 -> 85 / 76
  (1, 12), (2, 12) 79 / 132 -> 78 / 129     (1, 16), (2, 16) 81 / 128 -> 81 / 126
and vector + scalar instructions in the pass loop's macroblock (the innermost loop around the third v_mfma), (0, 12): 251 + 118 ->
243 + 116; from the column read to the coefficient tile's write 36 + 7 -> 28 + 5."""
import re
import shutil

import numpy as np
import pytest

import oracle_lib as O
import test_kernel_resources as R
import test_mdec_k311_resources as K

BUTTERFLY = [0, 1, 2, 3, 7, 6, 5, 4]


# ---------------------------------------------------------------- the DC quantiser
def quant16_f32(c):
    """the chunk's quantiser on a DC slot, in float32 as the kernel evaluates it: trunc(fma(|c|, 1/16, 0.5 + 0.25/16)).  |c| / 16
    and the bias 0.515625 are dyadic numbers with far fewer than 24 bits at this size, so the product and the sum are exact in
    float32 and plain arithmetic IS the fma.  Returns (magnitude, sign bit)"""
    c = np.asarray(c, dtype=np.int64)
    inv = np.float32(1.0) / np.float32(16.0)
    bias = np.float32(0.5) + np.float32(0.25) * inv
    prod = np.abs(c).astype(np.float32) * inv
    assert prod.dtype == np.float32 and np.array_equal(prod.astype(np.float64) * 16.0, np.abs(c).astype(np.float64))       # exact
    s = prod + bias
    assert s.dtype == np.float32 and np.array_equal(s.astype(np.float64), prod.astype(np.float64) + float(bias))       # exact
    return np.trunc(s).astype(np.int64), (c < 0).astype(np.int64)


def test_the_fp32_quantiser_at_divisor_16_is_the_dc_quantiser():
    c = np.arange(-32768, 32768, dtype=np.int64)
    q, neg = quant16_f32(c)
    assert np.array_equal(np.where(neg == 1, -q, q), (c + 8 + (c >> 63)) >> 4)          # quant_dc(), mdec.c:447-449
    # the quantiser's proven domain (tests/test_mdec_oracle.py::test_fp32_reciprocal_quantiser_is_exact): N = 2|n| + d < 2^17
    assert 2 * 8192 + 16 < 2 ** 17


def dc_block_pixels(total):
    """64 pixels whose sum is `total` (0 .. 64 * 255), as flat as that allows"""
    base, extra = divmod(int(total), 64)
    px = np.full(64, base, np.uint8)
    px[:extra] += 1
    return px.reshape(8, 8)


def test_the_chunks_dc_code_is_the_oracles_dc_field_over_the_whole_range():
    """every DC term a block can have, -8192 .. 8128 (the sum of 64 samples - 128), in one frame: the oracle's v2 stream, read back
    by the oracle's reader, against ((q ^ -negbit) + negbit) & 0x3FF of the fp32 quantiser"""
    nx, ny = 55, 50
    w, h = nx * 16, ny * 16
    values = np.arange(-8192, 8129)
    assert values.size <= nx * ny * 6
    want_dc = np.zeros((nx * ny, 6), np.int64)                # [raster macroblock][block: Cr, Cb, Y1..Y4]
    lu, ch = np.zeros((h, w), np.uint8), np.zeros((h // 2, w), np.uint8)
    for i in range(nx * ny * 6):
        c = int(values[i % values.size])
        mb, b = divmod(i, 6)
        fy, fx = divmod(mb, nx)
        want_dc[mb, b] = c
        px = dc_block_pixels(c + 8192)
        if b < 2:               # NV21: Cr at the even bytes of a chroma row, Cb at the odd ones
            ch[fy * 8:fy * 8 + 8, fx * 16 + b:fx * 16 + 16:2] = px
        else:
            y0, x0 = fy * 16 + ((b - 2) >> 1) * 8, fx * 16 + ((b - 2) & 1) * 8
            lu[y0:y0 + 8, x0:x0 + 8] = px
    frame = np.concatenate([lu.ravel(), ch.ravel()])
    coefs = O.mdec_coefs(w, h, frame)                                      # (6, macroblocks in raster order, 64)
    assert np.array_equal(coefs[:, :, 0].T.astype(np.int64), want_dc)      # the DC term is the sum of the level-shifted samples
    budget = 1 << 20
    out, res, rc = O.mdec_encode(0, w, h, frame[None, :], budget)
    assert rc == 0
    rc, levels, _, version, _ = O.mdec_decode(w, h, out[0, :int(res[0, 1])])
    assert rc == 0 and version == 2
    got = levels[:, 0].astype(np.int64).reshape(nx, ny, 6)                 # encode order: fx outer, fy inner
    got = got.transpose(1, 0, 2).reshape(nx * ny, 6)
    q, neg = quant16_f32(want_dc)
    code = ((q ^ -neg) + neg) & 0x3FF
    assert np.array_equal(code, got & 0x3FF)
    assert np.array_equal(code - ((code & 0x200) << 1), got)               # ... and as the signed 10-bit field the reader returns
    assert q.max() == 512 and np.where(neg == 1, -q, q).min() == -512 and np.where(neg == 1, -q, q).max() == 508       # the clamp at -512 / 510 never binds
    for flat, dc, field in ((0, -8192, 0x200), (128, 0, 0), (255, 8128, 0x1FC)):
        qq, nn = quant16_f32([64 * flat - 8192])
        assert 64 * flat - 8192 == dc and int(((qq ^ -nn) + nn)[0] & 0x3FF) == field


# ---------------------------------------------------------------- the row order
K_ = dict(k298=2446, k390=3196, k541=4433, k765=6270, k899=7373, k1175=9633, k1501=12299, k1847=15137, k1961=16069,
          k2053=16819, k2562=20995, k3072=25172)
A_, B_, C_ = K_["k541"] + K_["k765"], K_["k541"], K_["k541"] - K_["k1847"]
ODD = {
    7: (K_["k298"] - K_["k899"] - K_["k1961"] + K_["k1175"], K_["k1175"], K_["k1175"] - K_["k1961"], K_["k1175"] - K_["k899"]),
    5: (K_["k1175"], K_["k2053"] - K_["k2562"] - K_["k390"] + K_["k1175"], K_["k1175"] - K_["k2562"], K_["k1175"] - K_["k390"]),
    3: (K_["k1175"] - K_["k1961"], K_["k1175"] - K_["k2562"], K_["k3072"] - K_["k2562"] - K_["k1961"] + K_["k1175"], K_["k1175"]),
    1: (K_["k1175"] - K_["k899"], K_["k1175"] - K_["k390"], K_["k1175"], K_["k1501"] - K_["k899"] - K_["k390"] + K_["k1175"]),
}


def forms(s07, s16, s25, s34, o0, o1, o2, o3, column):
    """the islow butterfly's eight outputs as the kernel's linear forms (tests/test_mdec_oracle.py::test_dct_linear_forms)"""
    sh = 17 if column else 9
    rnd = 1 << (sh - 1)
    out = [None] * 8
    if column:
        out[0] = (s07 + s16 + s25 + s34 + 8) >> 4
        out[4] = (s07 - s16 - s25 + s34 + 8) >> 4
    else:
        out[0] = (s07 + s16 + s25 + s34 - 8 * 128) * 16
        out[4] = (s07 - s16 - s25 + s34) * 16
    out[2] = (s07 * A_ + s16 * B_ - s25 * B_ - s34 * A_ + rnd) >> sh
    out[6] = (s07 * B_ + s16 * C_ - s25 * C_ - s34 * B_ + rnd) >> sh
    for k, (c0, c1, c2, c3) in ODD.items():
        out[k] = (o0 * c0 + o1 * c1 + o2 * c2 + o3 * c3 + rnd) >> sh
    return np.stack(out, axis=-1).astype(np.int16).astype(np.int64)


def swap(pair):
    """v_alignbit_b32(x, x, 16): the halves of a packed pair change places"""
    return pair[1], pair[0]


def column_form(P0, P1, R0, R1):
    """fdct8_col_acc_k() on packed pairs (low half, high half): S = P + R, D = P - R per half, then the forms"""
    for lo, hi in (P0, P1, R0, R1):
        assert np.abs(lo).max() < 32768 and np.abs(hi).max() < 32768
    s07, s16 = P0[0] + R0[0], P0[1] + R0[1]
    s25, s34 = P1[0] + R1[0], P1[1] + R1[1]
    o3, o2 = P0[0] - R0[0], P0[1] - R0[1]
    o1, o0 = P1[0] - R1[0], P1[1] - R1[1]
    return forms(s07, s16, s25, s34, o0, o1, o2, o3, True)


def column_parent(t):
    """the parent's column pass: the tile's column holds rows 0..7; q.w and q.z are swapped and change places"""
    q = [(t[..., 2 * i], t[..., 2 * i + 1]) for i in range(4)]
    return column_form(q[0], q[1], swap(q[3]), swap(q[2]))


def column_k312(t):
    """this revision's: the tile's column holds rows 0, 1, 2, 3, 7, 6, 5, 4; the four dwords go in as they stand"""
    q = [(t[..., 2 * i], t[..., 2 * i + 1]) for i in range(4)]
    return column_form(q[0], q[1], q[2], q[3])


def test_rows_in_butterfly_order_need_no_half_swaps():
    rng = np.random.default_rng(12)
    # columns of the transpose tile: row-pass outputs are int16; output 0 is 16 x (row sum - 1024) in [-16384, 16256], the others
    # stay below 2^15 in magnitude; sums and differences of two must fit the packed int16 add (checked in column_form's callers'
    # range by the oracle comparison below), so the random columns keep to +-16383
    cols = rng.integers(-16383, 16384, (200000, 8)).astype(np.int64)
    cols[0], cols[1], cols[2] = 16383, -16383, np.array([16383, -16383] * 4)
    want = column_parent(cols)
    assert np.array_equal(column_k312(cols[:, BUTTERFLY]), want)
    # (and the permutation matters: the unswapped form on rows in natural order is another transform)
    assert not np.array_equal(column_k312(cols), want)


def test_the_permuted_column_pass_gives_the_oracles_coefficients():
    """whole blocks: row pass on raw pixels per row, rows stored in butterfly order, the unswapped column form -- against
    orc_fdct_islow8 on the level-shifted block"""
    rng = np.random.default_rng(13)
    blocks = rng.integers(0, 256, (4000, 8, 8)).astype(np.int64)
    blocks[0], blocks[1] = 0, 255
    blocks[2] = np.arange(8)[:, None] * 36                              # a vertical ramp
    for j in range(8):                                                   # one bright row at each position
        blocks[3 + j] = 16
        blocks[3 + j, j] = 240
    blocks[11:500] = np.where(rng.integers(0, 2, (489, 8, 8)) > 0, 255, 0)
    d = blocks
    rows = forms(d[..., 0] + d[..., 7], d[..., 1] + d[..., 6], d[..., 2] + d[..., 5], d[..., 3] + d[..., 4],
                 d[..., 3] - d[..., 4], d[..., 2] - d[..., 5], d[..., 1] - d[..., 6], d[..., 0] - d[..., 7], False)   # [block][row][output c]
    tile = rows[:, BUTTERFLY, :].transpose(0, 2, 1)                      # [block][column c][j]: the lane with lane & 7 == j holds row BUTTERFLY[j]
    got = column_k312(tile).transpose(0, 2, 1)                           # [block][row r][column c]
    want = (blocks - 128).astype(np.int16).reshape(-1, 64).copy()
    for i in range(want.shape[0]):
        O.lib().orc_fdct_islow8(O.ptr(want[i], O.i16p))
    assert np.array_equal(got.reshape(-1, 64), want.astype(np.int64))


# ---------------------------------------------------------------- the listing
needs_hipcc = pytest.mark.skipif(not shutil.which(R.HIPCC), reason="hipcc not installed")


def column_stretches(lines):
    """per v_mfma of a kernel (two pilot macroblocks, the pass loop): the lines from the column read behind it to the coefficient
    tile's write"""
    out = []
    for site in [i for i, ln in enumerate(lines) if "v_mfma" in ln]:
        rd = next(i for i in range(site, len(lines)) if re.match(r"\s+ds_read2_b64\s", lines[i]))
        assert "offset1:1" in lines[rd] and rd - site < 120, (site, rd, lines[rd])
        wr = next(i for i in range(rd, len(lines)) if re.match(r"\s+ds_write_b128\s", lines[i]))
        assert wr - rd < 120, (rd, wr)
        out.append(lines[rd:wr + 1])
    assert len(out) == 3
    return out


@needs_hipcc
def test_no_half_swap_between_the_column_read_and_the_coefficient_tiles_write():
    for shape, (lines, _) in K.product_shapes().items():
        for stretch in column_stretches(lines):
            swaps = [ln.strip() for ln in stretch if "v_alignbit_b32" in ln]
            dots = sum("v_dot2_i32_i16" in ln for ln in stretch)
            print(shape, "column read .. tile write: %d lines, %d v_dot2, v_alignbit: %s" % (len(stretch), dots, swaps))
            assert dots == 16, (shape, dots)              # it IS the column pass
            assert not swaps, (shape, swaps)


@needs_hipcc
def test_no_dc_clamp_in_the_v2_pass_loop():
    for (codec, waves), (lines, _) in K.product_shapes().items():
        if codec != 0:
            continue
        a, b, _ = K.pass_loop(lines)
        clamps = [ln.strip() for ln in lines[a:b + 1] if "v_med3_i32" in ln]
        assert not clamps, ((codec, waves), clamps)


@needs_hipcc
def test_product_shapes_have_no_scratch_and_stay_inside_their_ceilings():
    """(the diagnostics instantiations of the 12-wavefront shapes carry scratch, as they did before: they are not measured)"""
    for (codec, waves), (_, u) in K.product_shapes().items():
        print((codec, waves), "VGPRs", u["VGPRs"], "spilled SGPRs", u["SGPRs Spill"])
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0", ((codec, waves), u)
        assert int(u["VGPRs"]) <= (80 if waves == 12 else 128), ((codec, waves), u)
        assert int(u["SGPRs Spill"]) <= R.SGPR_CEILINGS[(codec, waves)][0], ((codec, waves), u)
