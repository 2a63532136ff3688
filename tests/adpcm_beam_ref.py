""""psxhip ADPCM beam v1" (DESIGN.md section 22), the statement: `encode_unit` is the rule in its plainest form -- Python integers,
explicit lists and a stable sort -- and `encode_units_np` the same rule with numpy over many units at once, which the tests hold
equal to it.  Test infrastructure only; nothing here knows the library.

Per unit: the carried state (p1, p2), 28 samples (zeros at and past the chain's sample_limit), filter_count 5 or 4, the shift range
R = 12 (4-bit codes) or 8 (8-bit codes), the beam width B in 1 .. 4."""
import numpy as np

K1, K2 = (0, 60, 115, 98, 122), (0, 0, -52, -55, -60)
SAT = (1 << 32) - 1


def shift_range(bits):
    return 12 if bits == 4 else 8


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def min_shift(x, p1, p2, f, R):
    """find_min_shift, libpsxav/adpcm.c:39-79: the history continues with raw samples"""
    lo = hi = 0
    for xi in x:
        r = xi - ((K1[f] * p1 + K2[f] * p2 + 32) >> 6)
        lo, hi = min(lo, r), max(hi, r)
        p1, p2 = xi, p1
    rs = 0
    while rs < R and (hi >> rs) > (0x7FFF >> R):
        rs += 1
    while rs < R and (lo >> rs) < (-0x8000 >> R):
        rs += 1
    return R - rs


def candidates(x, p1, p2, FC, R):
    """the reference's candidates in its loop order (adpcm.c:158-183)"""
    out = []
    for f in range(FC):
        m = min_shift(x, p1, p2, f, R)
        out += [(f, s) for s in range(max(0, m - 1), min(R, m + 1) + 1)]
    return out


def candidate(x, p1, p2, f, s, R, B, stats=None):
    """-> (e, codes, y) of the candidate's result, and its slot"""
    lo, hi = -0x8000 >> R, 0x7FFF >> R
    slots = [(0, p1, p2, [], [])]                              # (e, p1, p2, codes, decoded)
    for xi in x:
        pool, anchor = [], None
        for j, (e, a, b, codes, ys) in enumerate(slots):
            pv = (K1[f] * a + K2[f] * b + 32) >> 6
            q0 = clamp((((xi - pv) << s) + (1 << (R - 1))) >> R, lo, hi)
            for d in (0, -1, 1):
                q = q0 + d
                if q < lo or q > hi:
                    if stats is not None:
                        stats.add("rail_lo" if q < lo else "rail_hi")
                    continue
                y = clamp(((q * (1 << R)) >> s) + pv, -32768, 32767)
                child = (min(e + (y - xi) ** 2, SAT), y, a, codes + [q], ys + [y])
                if j == 0 and d == 0:
                    anchor = child
                else:
                    pool.append(child)
        pool.sort(key=lambda c: c[0])                          # stable: ties go to the earlier child
        if stats is not None and B > 1 and len(pool) >= B and pool[B - 2][0] == pool[B - 1][0]:
            stats.add("tie")                                   # the pool's order decided which child was kept
        slots = [anchor] + pool[:B - 1]
    best = min(range(len(slots)), key=lambda j: (slots[j][0], j))
    if stats is not None and slots[0][0] == SAT:
        stats.add("saturated")
    return slots[best][0], slots[best][3], slots[best][4], best


def pack_record(header, codes, bits):
    rec = np.zeros(16 if bits == 4 else 32, np.uint8)
    rec[0] = header
    c = np.asarray(codes, np.int64)
    if bits == 4:
        rec[2:] = (c[0::2] & 0x0F) | ((c[1::2] & 0x0F) << 4)
    else:
        rec[4:] = c & 0xFF
    return rec


def encode_unit(x, p1, p2, FC, bits, B, stats=None):
    """-> (record, e, (new p1, new p2), (f, s, slot)): the first candidate in loop order with the smallest e by strict <"""
    R = shift_range(bits)
    x = [int(v) for v in x]
    best = None
    for f, s in candidates(x, p1, p2, FC, R):
        e, codes, ys, slot = candidate(x, p1, p2, f, s, R, B, stats)
        if best is None or e < best[0]:
            best = (e, codes, ys, f, s, slot)
    e, codes, ys, f, s, slot = best
    return pack_record((s & 15) | (f << 4), codes, bits), e, (ys[27], ys[26]), (f, s, slot)


def encode_chain(x, state, n_units, FC, bits, B, stats=None):
    """x: the chain's samples, zeros behind its limit -> (records, e per unit, state after every unit (n, 2), (f, s, slot) per unit)"""
    rec = np.zeros((n_units, 16 if bits == 4 else 32), np.uint8)
    err, after, pick = np.zeros(n_units, np.uint32), np.zeros((n_units, 2), np.int32), np.zeros((n_units, 3), np.int32)
    p1, p2 = int(state[0]), int(state[1])
    for u in range(n_units):
        rec[u], err[u], (p1, p2), pick[u] = encode_unit(x[28 * u:28 * u + 28], p1, p2, FC, bits, B, stats)
        after[u] = (p1, p2)
    return rec, err, after, pick


# ---- the same rule over N units at once ---------------------------------------------------------------------------------------------
def _min_shift_np(x, p1, p2, f, R):
    lo, hi = np.zeros(len(x), np.int64), np.zeros(len(x), np.int64)
    a, b = p1.copy(), p2.copy()
    for i in range(28):
        r = x[:, i] - ((K1[f] * a + K2[f] * b + 32) >> 6)
        lo, hi = np.minimum(lo, r), np.maximum(hi, r)
        a, b = x[:, i], a
    rs = np.zeros(len(x), np.int64)
    for _ in range(R):
        rs += (rs < R) & ((hi >> rs) > (0x7FFF >> R))
    for _ in range(R):
        rs += (rs < R) & ((lo >> rs) < (-0x8000 >> R))
    return R - rs


def encode_units_np(x, p1, p2, FC, bits, B, stats=None):
    """x (N, 28), p1, p2 (N,) -> (records (N, record bytes), e (N,) uint32, new states (N, 2), picks (N, 3): f, s, slot).
    Every candidate of every unit is a row of its own; the unit's result is the first row in loop order with the smallest e"""
    R = shift_range(bits)
    x = np.asarray(x, np.int64).reshape(-1, 28)
    N = len(x)
    p1, p2 = np.asarray(p1, np.int64), np.asarray(p2, np.int64)
    lo, hi = -0x8000 >> R, 0x7FFF >> R
    INF = np.int64(1) << 40
    # rows: unit-major, then the candidates in loop order (filter, then shift m - 1, m, m + 1); shifts outside 0 .. R are not candidates
    ms = np.stack([_min_shift_np(x, p1, p2, f, R) for f in range(FC)], axis=1)                     # (N, FC)
    s_all = (ms[:, :, None] + np.array([-1, 0, 1])).reshape(N, FC * 3)
    valid = (s_all >= 0) & (s_all <= R)
    nc = FC * 3
    s = np.where(valid, s_all, 0).reshape(-1, 1)
    f_all = np.tile(np.repeat(np.arange(FC), 3), N)
    k1, k2 = np.array(K1)[f_all][:, None], np.array(K2)[f_all][:, None]
    xr = np.repeat(x, nc, axis=0)
    M = N * nc
    e = np.zeros((M, 4), np.int64)
    a, b = np.zeros((M, 4), np.int64), np.zeros((M, 4), np.int64)
    a[:, 0], b[:, 0] = np.repeat(p1, nc), np.repeat(p2, nc)
    live = np.zeros((M, 4), bool)
    live[:, 0] = True
    codes = np.zeros((M, 4, 28), np.int64)
    rows = np.arange(M)[:, None]
    for i in range(28):
        xi = xr[:, i:i + 1]
        pv = (k1 * a + k2 * b + 32) >> 6
        q0 = np.clip((((xi - pv) << s) + (1 << (R - 1))) >> R, lo, hi)
        q = np.stack([q0, q0 - 1, q0 + 1], axis=2).reshape(M, 12)                   # slot rising, then d = 0, -1, +1
        ok = np.repeat(live, 3, axis=1) & (q >= lo) & (q <= hi)
        y = np.clip(((q << R) >> s) + np.repeat(pv, 3, axis=1), -32768, 32767)
        ee = np.minimum(np.repeat(e, 3, axis=1) + (y - xi) ** 2, SAT)
        key = np.where(ok, ee, INF)
        key[:, 0] = -1                                                              # the anchor's d = 0 child is slot 0 whatever its error
        full = np.argsort(key, axis=1, kind="stable")
        order = full[:, :4]
        if stats is not None:                                                       # what the candidates' rows met (tests' non-vacuity)
            vr, lp = valid.reshape(-1, 1), np.repeat(live, 3, axis=1)
            pool = np.take_along_axis(key, full, 1)[:, 1:]
            for name, hit in (("rail_lo", vr & lp & (q < lo)), ("rail_hi", vr & lp & (q > hi)), ("saturated", vr[:, 0] & (ee[:, 0] == SAT)),
                              ("tie", vr[:, 0] & (pool[:, B - 2] == pool[:, B - 1]) & (pool[:, B - 1] < INF)) if B > 1 else ("tie", np.zeros(1, bool))):
                if hit.any():
                    stats.add(name)
        taken = np.take_along_axis(ok, order, 1)
        taken[:, B:] = False
        parent = order // 3
        e = np.where(taken, np.take_along_axis(ee, order, 1), 0)
        na = np.where(taken, np.take_along_axis(y, order, 1), 0)
        b = np.where(taken, np.take_along_axis(a, parent, 1), 0)
        a = na
        codes = codes[rows, parent]
        codes[:, :, i] = np.take_along_axis(q, order, 1)
        live = taken
    res = np.where(live, e, INF)
    slot = np.argmin(res, axis=1)                                                   # the first of equal minima: the lowest slot
    ce = np.where(valid.reshape(-1), res[np.arange(M), slot], INF).reshape(N, nc)
    win = np.argmin(ce, axis=1)                                                     # the first candidate in loop order with the minimum
    r = np.arange(N) * nc + win
    best_e = ce[np.arange(N), win]
    c = codes[r, slot[r]]
    st = np.stack([a[r, slot[r]], b[r, slot[r]]], axis=1)
    pick = np.stack([f_all[r], s[r, 0], slot[r]], axis=1)
    rec = np.zeros((N, 16 if bits == 4 else 32), np.uint8)
    rec[:, 0] = (pick[:, 1] & 15) | (pick[:, 0] << 4)
    if bits == 4:
        rec[:, 2:] = (c[:, 0::2] & 0x0F) | ((c[:, 1::2] & 0x0F) << 4)
    else:
        rec[:, 4:] = c & 0xFF
    return rec, best_e.astype(np.uint32), st.astype(np.int32), pick.astype(np.int32)


def encode_chains_np(xs, states, n_units, FC, bits, B, stats=None):
    """many chains side by side, unit after unit: xs (C, >= 28 max n), states (C, 2), n_units (C,)
    -> (records (C, max n, record bytes), e (C, max n), state after every unit (C, max n, 2), picks (C, max n, 3))"""
    n_units = np.asarray(n_units)
    C, n = len(xs), int(n_units.max()) if len(n_units) else 0
    rec = np.zeros((C, n, 16 if bits == 4 else 32), np.uint8)
    err, after, pick = np.zeros((C, n), np.uint32), np.zeros((C, n, 2), np.int32), np.zeros((C, n, 3), np.int32)
    st = np.asarray(states, np.int64).reshape(C, 2).copy()
    for u in range(n):
        on = np.nonzero(n_units > u)[0]
        r, e, s, pk = encode_units_np(np.asarray(xs)[on, 28 * u:28 * u + 28], st[on, 0], st[on, 1], FC, bits, B, stats)
        rec[on, u], err[on, u], after[on, u], pick[on, u] = r, e, s, pk
        st[on] = s
    return rec, err, after, pick
