"""Inputs and plain-numpy answers for tests/cpu/wave_probe.hip: what every cross-lane operation of a 64-lane wavefront must give,
written down lane by lane from the definitions (HIP's __shfl family, the gfx9 DPP controls, ballot / mbcnt), without any of the
project's code.  tests/test_wave_model_cpu.py holds the stand-in's wavefront model to these bytes, tests/test_gpu_wave_probe.py the
MI355X.

Test infrastructure only."""
import numpy as np

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
LANES = np.arange(64)


def make_input(seed=7):
    rng = np.random.default_rng(seed)
    rows = [rng.integers(-2 ** 24, 2 ** 24, 64) for _ in range(6)]
    rows += [np.zeros(64, np.int64), np.full(64, INT_MIN // 64), np.full(64, INT_MAX // 64), LANES.copy(), -LANES,
             np.where(LANES & 1, INT_MAX // 64, INT_MIN // 64), rng.integers(0, 2, 64), np.ones(64, np.int64)]
    for at in range(64):            # a single non-zero lane in every position, of either sign and both parities
        one = np.zeros(64, np.int64)
        one[at] = (INT_MAX - at) if at & 1 else (INT_MIN + at)
        rows.append(one)
    x = np.array(rows, dtype=np.int64).astype(np.int32)
    n = x.shape[0]
    y = rng.integers(-2 ** 63, 2 ** 63 - 1, (n, 64), dtype=np.int64)
    y[6] = 0
    y[7] = -2 ** 63
    y[8] = 2 ** 63 - 1
    y[9] = LANES                    # the minimum in lane 0, in lane 63 ...
    y[10] = -LANES
    for at in range(64):            # ... and in every position, with the runner-up one above it
        y[14 + at] = 5
        y[14 + at, at] = 4
    masks = [(0, 0), (2 ** 64 - 1, 2 ** 64 - 1), (1, 1), (2 ** 63, 2 ** 63), (2 ** 32, 2 ** 31), (2 ** 31, 2 ** 32), (0x8000000080000001, 0x0001000000010000)]
    masks += [(1 << at, 2 ** 64 - 1 - (1 << at)) for at in (1, 15, 16, 30, 33, 47, 62)]
    rnd = lambda: int(rng.integers(0, 2 ** 64, dtype=np.uint64))
    masks += [(rnd(), rnd()) for _ in range(6)]
    masks += [(rnd() & rnd() & rnd(), rnd() & rnd() & rnd() & rnd()) for _ in range(4)]          # sparse
    masks = np.array(masks, dtype=np.uint64)
    tiles = rng.integers(INT_MIN, INT_MAX, (3, 256), dtype=np.int64).astype(np.int32)
    atom = rng.integers(0, 2 ** 32, (3, 256), dtype=np.int64).astype(np.uint32)
    atom[1, 17] = 0
    atom[2, 200] = 0xFFFFFFFF
    return x, y, masks, tiles, atom


def to_bytes(x, y, masks, tiles, atom):
    head = np.array([x.shape[0], masks.shape[0], tiles.shape[0], atom.shape[0]], dtype=np.int32)
    return b"".join(a.tobytes() for a in (head, x, y, masks, tiles, atom))


def take(v, src, keep=None):
    """lane l of every row reads lane src[l]; where keep[l], its own value"""
    out = v[:, src % 64]
    return out if keep is None else np.where(keep[None, :], v, out)


def shfl_up(v, d, width=64):
    return take(v, LANES - d, (LANES & (width - 1)) < d)


def shfl_down(v, d, width=64):
    return take(v, LANES + d, (LANES & (width - 1)) + d >= width)


def dpp(old, v, ctrl, row_mask, bank_mask, bound_ctrl):
    """v_mov_b32 with a DPP control: rows of 16 lanes, banks of 4.  The lane reads v of the lane the control names; a lane whose row
    or bank is masked out keeps old; a lane whose source is shifted in from outside the row reads 0 with bound_ctrl and keeps old
    without; a lane of a row the broadcast does not reach reads its own v (the MI355X's answer, tests/test_gpu_wave_probe.py)"""
    out = np.array(old, dtype=np.int32).copy()
    for l in range(64):
        row, in_row = l >> 4, l & 15
        if ctrl <= 0xFF:
            src = (l & ~3) | ((ctrl >> (2 * (l & 3))) & 3)
        elif 0x111 <= ctrl <= 0x11F:
            src = l - (ctrl & 15) if in_row >= (ctrl & 15) else None
        elif ctrl == 0x140:
            src = (l & ~15) | (15 - in_row)
        elif ctrl == 0x141:
            src = (l & ~7) | (7 - (l & 7))
        elif ctrl == 0x142:
            src = row * 16 - 1 if row > 0 else l
        elif ctrl == 0x143:
            src = 31 if row > 1 else l
        else:
            raise ValueError(ctrl)
        if not (row_mask >> row) & 1 or not (bank_mask >> (in_row >> 2)) & 1:
            continue
        if src is None:
            if bound_ctrl:
                out[:, l] = 0
            continue
        out[:, l] = v[:, src]
    return out


def popcount(m):
    return bin(int(m)).count("1")


def expected(x, y, masks, tiles, atom):
    n = x.shape[0]
    wide = x.astype(np.int64)
    scan, total = np.cumsum(wide, axis=1), wide.sum(axis=1)
    assert np.abs(scan).max() <= INT_MAX + 1 and scan.min() >= INT_MIN, "the inputs keep every partial sum inside 32 bits"
    odd_bits = (x & 1).astype(np.uint64)
    odd = (odd_bits << LANES.astype(np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    below = np.cumsum(odd_bits.astype(np.int64), axis=1) - odd_bits.astype(np.int64)
    zero, old = np.zeros_like(x), np.broadcast_to((-1000 - LANES).astype(np.int32), x.shape)
    rep = lambda col: np.repeat(np.asarray(col)[:, None], 64, axis=1)
    out32 = [scan, rep(total), below, rep(x[:, 0]), rep((x != 0).any(axis=1)), rep([popcount(m) for m in odd])]
    out32 += [shfl_up(x, d) for d in (0, 1, 2, 31, 32, 63, 64)] + [shfl_down(x, d) for d in (0, 1, 2, 31, 32, 63, 64)]
    out32 += [take(x, LANES ^ m) for m in (1, 5, 32, 63)]
    out32 += [take(x, LANES * 0), take(x, LANES * 0 + 63), take(x, LANES * 7 + 3), take(x, LANES + 65),
              np.take_along_axis(x, (x & 63).astype(np.int64), axis=1)]
    out32 += [shfl_up(x, 3, 16), shfl_down(x, 3, 16), take(x, LANES ^ 9), take(x, (LANES & ~15) | 5)]
    out32 += [rep(x[:, 0]), rep(x[:, 37]), rep(x[:, 63])]
    out32 += [dpp(zero, x, 0xB1, 0xF, 0xF, True), dpp(zero, x, 0x4E, 0xF, 0xF, True), dpp(old, x, 0x1B, 0x5, 0x9, False),
              dpp(zero, x, 0x111, 0xF, 0xF, True), dpp(zero, x, 0x112, 0xF, 0xF, True), dpp(zero, x, 0x113, 0xF, 0xF, True),
              dpp(zero, x, 0x114, 0xF, 0xE, False), dpp(zero, x, 0x118, 0xF, 0xC, False), dpp(old, x, 0x111, 0xF, 0xF, False),
              dpp(old, x, 0x11F, 0xF, 0xF, False), dpp(zero, x, 0x140, 0xF, 0xF, True), dpp(zero, x, 0x141, 0xF, 0xF, True),
              dpp(zero, x, 0x142, 0xA, 0xF, False), dpp(zero, x, 0x143, 0xC, 0xF, False), dpp(old, x, 0x142, 0xF, 0xF, False),
              dpp(old, x, 0x143, 0xF, 0xF, False), dpp(old, x, 0x114, 0xF, 0xE, True)]
    out32 = np.stack([np.asarray(a).astype(np.int64).astype(np.int32) for a in out32])
    assert out32.shape == (53, n, 64)
    flipped = y.view(np.uint64) ^ np.uint64(2 ** 63)
    out64 = np.stack([rep(odd), rep(flipped.min(axis=1)), shfl_up(y, 1).view(np.uint64), shfl_up(y, 64).view(np.uint64), shfl_down(y, 1).view(np.uint64),
                      shfl_down(y, 33).view(np.uint64), take(y, LANES ^ 32).view(np.uint64), take(y, LANES * 5 + 1).view(np.uint64)]).astype(np.uint64)
    m32, m64 = np.zeros((8, masks.shape[0], 64), np.int32), np.zeros((masks.shape[0], 64), np.uint64)
    for i, (pred, other) in enumerate(masks):
        pred, other = int(pred), int(other)
        m32[0, i] = np.array(pred & 0xFFFFFFFF, dtype=np.int64).astype(np.int32)
        m32[1, i] = np.array(pred >> 32, dtype=np.int64).astype(np.int32)
        m64[i] = pred
        for l in range(64):
            m32[2, i, l] = 5 + popcount(other & ((1 << l) - 1))
            m32[3, i, l] = popcount(other & ((1 << l) - 1))
        m32[4, i] = popcount(other)
        m32[5, i] = (other & -other).bit_length()                  # 1-based position of the lowest set bit, 0 for none
        m32[6, i] = 64 - other.bit_length()
        m32[7, i] = 1 if pred else 0
    t1 = tiles[:, (np.arange(256) & 15) * 16 + (np.arange(256) >> 4)]
    tiles_out = t1[:, 255 - np.arange(256)]
    a = atom.astype(np.int64).ravel()
    signed = atom.view(np.int32).astype(np.int64).ravel()
    u32 = lambda v: int(v) & 0xFFFFFFFF
    or_bits = 0
    for v in a[(a & 7) == 0]:
        or_bits |= 1 << (int(v) >> 27)
    lds_or = 0
    for g in range(atom.shape[0]):
        lds_or |= 0xFFFFFFFF & int(atom[g, 0])
    res = [u32(((a & 0xFFFF) - 30000).sum()), u32((a >> 12).sum()), int((a << 8).sum()), u32(1000000 - (a & 0xFFF).sum()), int(a.min()),
           u32(min(signed.min(), INT_MAX)), int(a.max()), u32(max(signed.max(), INT_MIN)), or_bits, u32((a & 0xFF).sum()), int(a.max()),
           int(a.min()), lds_or]
    res = np.array(res, dtype=np.uint64)
    return b"".join(v.tobytes() for v in (out32, out64, m32, m64, tiles_out.astype(np.int32), res))


SECTIONS = ("out32", "out64", "m32", "m64", "tiles", "atomics")


def describe(got, want, x, masks, tiles):
    """where two outputs differ first, in the terms of wave_probe.hip's slots"""
    if len(got) != len(want):
        return "%d bytes instead of %d" % (len(got), len(want))
    at = next(i for i, (p, q) in enumerate(zip(got, want)) if p != q)
    n, m = x.shape[0], masks.shape[0]
    sizes = (53 * n * 64 * 4, 8 * n * 64 * 8, 8 * m * 64 * 4, m * 64 * 8, tiles.size * 4, 13 * 8)
    item = (4, 8, 4, 8, 4, 8)
    per = (n * 64, n * 64, m * 64, m * 64, 256, 1)
    for name, size, it, p in zip(SECTIONS, sizes, item, per):
        if at < size:
            k = at // it
            return "%s: slot %d, row %d, lane %d (byte %d)" % (name, k // p, k % p // 64 if p > 1 else 0, k % 64 if p > 1 else 0, at)
        at -= size
    return "behind the end"
