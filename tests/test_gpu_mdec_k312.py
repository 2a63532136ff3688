"""Cases for mdec-k3.12 (NOTEBOOK, "mdec-k3.12"): the frame kernel's lanes fetch a block's pixel rows in butterfly order (0, 1, 2, 3,
7, 6, 5, 4), so that the column pass needs no half-swaps, and the v2 DC term leaves the column pass raw and is quantised in the
chunk, by the quantiser every list entry goes through (divisor 16 in lane 0 of the pass's emit quantiser).

Every output byte and every result word is compared with the CPU oracle, on two launches of one context (cold and warm), for all
three codecs, in both workgroup shapes (32 frames: 16 wavefronts, 600 frames: 12, as tests/test_gpu_mdec_k311.py picks them), under
one and two launch lanes, as a launch with one budget and as a launch with a budget per frame.

Geometry: 16x16, 48x16, 16x48, 64x64 and 256x128 (the smallest frame with a checkpoint in both workgroup shapes).

Content for the DC term: flat frames of 0, 128 and 255 (DC -8192, 0 and 8128: codes 0x200, 0 and 0x1FC), noise +-4, +-8 and +-40, and
frames of quiet noise around a dark and a bright level per block in which every block's sum is moved onto a rounding tie of the
division by 16.  Before anything runs on the device the oracle's coefficients have to show at least 32 blocks with DC = 8 (mod 16) of
each sign among a geometry's frames.

Content for the row order: a vertical ramp, and one bright row at each of the eight positions of a block -- in luma, in Cr and (at
another position) in Cb.  No two rows of such a block are alike, so a wrong order cannot cancel.

Long lists: noise +-40 at the budgets of scales 1 and 2, noise +-8 and +-6 at the budget of scale 3, at 256x128 (v2): code lists of
several 64-entry chunks, whose DC slots pass through the multi-chunk form of the chunk and through the recompaction of a list made
at the count scale (which leaves one chunk of the +-6 lists and more than one of the +-8 lists)."""
import numpy as np
import pytest

import mdec_hard_content as H
import oracle_lib as O
import test_gpu_mdec_k310 as K
import test_gpu_mdec_k311 as K11
import test_gpu_mdec_sampled_count as S

pytestmark = pytest.mark.gpu

GEOMETRIES = [(16, 16), (48, 16), (16, 48), (64, 64), (256, 128)]
CODECS = [0, 1, 2]
SHAPES = K.SHAPES              # 32 frames: the 16-wavefront shape, 600: the 12-wavefront shape
MIN_TIES = 32


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---------------------------------------------------------------- content
def block_view(lu, ch, fx, fy, b):
    """the 8x8 samples of block b (Cr, Cb, Y1..Y4) of macroblock (fx, fy), as a view into the NV21 planes"""
    if b < 2:
        return ch[fy * 8:fy * 8 + 8, fx * 16 + b:fx * 16 + 16:2]
    y0, x0 = fy * 16 + ((b - 2) >> 1) * 8, fx * 16 + ((b - 2) & 1) * 8
    return lu[y0:y0 + 8, x0:x0 + 8]


def tie_frame(w, h, seed):
    """noise +-8 around 96 or 160 (alternating from block to block), one sample of every block moved so that the block's DC term --
    the sum of its samples - 128 -- is 8 (mod 16): a rounding tie of the division by 16, negative in the dark blocks, positive
    in the bright ones"""
    rng = np.random.default_rng(seed)
    lu, ch = np.zeros((h, w), np.uint8), np.zeros((h // 2, w), np.uint8)
    i = seed
    for fy in range(h // 16):
        for fx in range(w // 16):
            for b in range(6):
                v = block_view(lu, ch, fx, fy, b)
                px = (96 if i & 1 else 160) + rng.integers(-8, 9, (8, 8))
                dc = int(px.sum()) - 8192
                px[0, 0] += (16 - dc) % 16 - 8                     # -8 .. 7 and = 8 - dc (mod 16): stays inside a byte
                v[:, :] = px
                i += 1
    return K.nv21(w, h, lu, ch)


def ramp_frame(w, h):
    """every block a vertical ramp: row j at 20 + 30 j (Cb runs the other way)"""
    lu = np.broadcast_to((20 + 30 * (np.arange(h) % 8))[:, None], (h, w))
    ch = np.zeros((h // 2, w), np.int64)
    ch[:, 0::2] = (20 + 30 * (np.arange(h // 2) % 8))[:, None]
    ch[:, 1::2] = (230 - 30 * (np.arange(h // 2) % 8))[:, None]
    return K.nv21(w, h, lu, ch)


def bright_row_frame(w, h, j):
    """row j of every luma block and of every Cr block at 235, row (j + 3) % 8 of every Cb block; everything else at 30"""
    lu, ch = np.full((h, w), 30, np.uint8), np.full((h // 2, w), 30, np.uint8)
    lu[np.arange(h) % 8 == j, :] = 235
    ch[np.arange(h // 2) % 8 == j, 0::2] = 235
    ch[np.arange(h // 2) % 8 == (j + 3) % 8, 1::2] = 235
    return K.nv21(w, h, lu, ch)


def dc_ties(w, h, frames):
    """(blocks with DC = 8 (mod 16) and DC > 0, the same with DC < 0) over the frames, from the oracle's coefficients"""
    pos = neg = 0
    for f in frames:
        dc = O.mdec_coefs(w, h, f)[:, :, 0].astype(np.int64).ravel()
        tie = dc % 16 == 8
        pos += int((tie & (dc > 0)).sum())
        neg += int((tie & (dc < 0)).sum())
    return pos, neg


def contents(w, h):
    nblk = 6 * (w // 16) * (h // 16)
    out = [("flat %d" % v, K.flat(w, h, v)) for v in (0, 128, 255)]
    out += [("noise +-%d" % amp, O.synth_frames(w, h, 1, seed=120 + amp, amp=amp)[0]) for amp in (4, 8, 40)]
    out += [("vertical ramp", ramp_frame(w, h))]
    out += [("bright row %d" % j, bright_row_frame(w, h, j)) for j in range(8)]
    # tie frames: seeds are drawn until the geometry's frames hold enough ties of each sign (a 16x16 frame has six blocks)
    seed = 0
    while seed == 0 or min(dc_ties(w, h, [f for _, f in out])) < MIN_TIES:
        out.append(("ties #%d" % seed, tie_frame(w, h, 500 + seed)))
        seed += 1
        assert seed <= 2 * MIN_TIES // max(nblk // 2, 1) + 2, seed
    return out


def check_inputs(w, h, frames):
    """conditions on the inputs, from the oracle alone"""
    named = dict(frames)
    pos, neg = dc_ties(w, h, [f for _, f in frames])
    assert pos >= MIN_TIES and neg >= MIN_TIES, (pos, neg)
    for v, dc in ((0, -8192), (128, 0), (255, 8128)):
        assert (O.mdec_coefs(w, h, named["flat %d" % v])[:, :, 0] == dc).all()
    return pos, neg


def cases(codec, w, h):
    """(rows for a launch with a budget per frame, rows for a launch with one budget)"""
    cap = S.CAP
    frames = contents(w, h)
    pos, neg = check_inputs(w, h, frames)
    per_frame = []
    needs = {name: O.mdec_need(codec, w, h, f) for name, f in frames}
    for name, f in frames:
        need = needs[name]
        # the exact fit of scales 1, 2, 4, 9 and 20 and one 16-bit word short of scale 3: the three finest that the context has room for
        budgets = sorted({(int(need[s]) + 1) & ~1 for s in (1, 2, 4, 9, 20)} | {int(need[3]) - 2})
        for b in [x for x in budgets if 8 < x <= cap][-3:]:
            per_frame.append(K11.row(codec, "%s %dx%d at %d" % (name, w, h, b), w, h, f, b, "per-frame"))
    # one budget for all: noise +-8 at scale 3
    u = min(max((int(needs["noise +-8"][3]) + 1) & ~1, 10), cap)
    uniform = [K11.row(codec, "%s %dx%d at %d" % (name, w, h, u), w, h, f, u, "uniform") for name, f in frames]
    assert all(r.res is not None for r in uniform if not r.name.startswith("noise +-40"))
    return per_frame, uniform, (pos, neg)


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_dc_terms_and_row_order_give_the_oracles_bytes(torch_cuda, w, h, codec):
    from psxavenc_amd.mdec import query_geometry
    assert query_geometry(codec, w, h, S.CAP).fits
    per_frame, uniform, ties = S.shared(("k312", codec, w, h), lambda: cases(codec, w, h))
    print("%dx%d codec %d: %d frames, DC ties %d positive / %d negative, per-frame answers %s, uniform answers %s"
          % (w, h, codec, len(uniform), ties[0], ties[1], sorted({r.scale for r in per_frame}), sorted({r.scale for r in uniform})))
    for n in SHAPES:
        for lanes in (1, 2):
            K11.launch_twice(torch_cuda, codec, w, h, K.repeat(per_frame, n, 12 * n + lanes), S.CAP, lanes, False)
            K11.launch_twice(torch_cuda, codec, w, h, [uniform[i % len(uniform)] for i in range(n)], S.CAP, lanes, True)


# ---------------------------------------------------------------- long lists
def list_lengths(w, h, frame, scale):
    """entries of every macroblock's code list made at `scale`: the six DC slots and the coefficients that quantise to non-zero"""
    quant = H.luts()[2]
    mag = H.frame_blocks(w, h, frame)                       # (6 x macroblocks, 64), scan order
    d = quant * scale
    nz = (2 * mag + d) // (2 * d) != 0
    nz[:, 0] = False
    return 6 + nz.sum(axis=1).reshape(6, -1).sum(axis=0)


def long_rows(w, h, cap):
    rows, kinds = [], set()
    for amp, scales in ((40, (1, 2)), (8, (3,)), (6, (3,))):
        f = O.synth_frames(w, h, 1, seed=300 + amp, amp=amp)[0]
        for p in scales:
            rows.append(S.Row("noise +-%d at scale %d" % (amp, p), w, h, f, K.fit_budget(w, h, f, p, cap), "long", p))
            assert rows[-1].scale == p
            at = list_lengths(w, h, f, p)
            if (at > 128).any():
                kinds.add("an emit list of three chunks and more")
            if p > 1:
                below = list_lengths(w, h, f, p - 1)
                if ((below > 64) & (below <= 128) & (at > 64)).any():
                    kinds.add("a count list of two chunks that stays longer than one after the recompaction")
                if ((below > 64) & (below <= 128) & (at <= 64)).any():
                    kinds.add("a count list of two chunks that is one after the recompaction")
    # conditions on the inputs: from the oracle's coefficients and the tables
    assert len(kinds) == 3, kinds
    return rows


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("n", SHAPES)
def test_dc_slots_in_lists_of_several_chunks(torch_cuda, n, lanes):
    w, h, cap = 256, 128, 65536
    from psxavenc_amd.mdec import query_geometry
    assert query_geometry(0, w, h, cap).fits
    base = S.shared(("k312 long", w, h), lambda: long_rows(w, h, cap))
    K.launch_twice(torch_cuda, w, h, K.repeat(base, n, 7 * n + lanes), cap, lanes, False)
    K.launch_twice(torch_cuda, w, h, [base[0]] * n, cap, lanes, True)
