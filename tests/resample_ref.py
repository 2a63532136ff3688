"""The statement of "psxhip audio front-end v1"  in plain numpy int64: the checker for psxhip_resampler_*.

Test infrastructure, written from the specification, not from the kernel.  The coefficient table is the one thing taken from
the library (psxhip_resampler_design, pure host); test_resampler_design.py holds that table to the formula.  Everything after it
is integer arithmetic, so any output can be computed straight from the input: whole streams for the bit-exact tests, and single
indices of long jobs for spot checks."""
import math

import numpy as np

PCM_S16, PCM_S16P, PCM_S32, PCM_S32P, PCM_F32, PCM_F32P = range(6)


def params(src, dst):
    """(L, M, P, T, H, factor) of the closed forms (section 10, step 3)"""
    g = math.gcd(src, dst)
    L, M = dst // g, src // g
    if src == dst:
        return L, M, 1, 0, 0, 1.0
    factor = min(0.97 * dst / src, 1.0)
    T = int(math.ceil(32.0 / factor))
    T += T & 1
    return L, M, (L if L <= 1024 else 1024), T, T // 2, factor


def to_int16(fmt, x):
    """step 1: one channel (or an interleaved buffer) of the source format -> int16"""
    x = np.asarray(x)
    if fmt in (PCM_S16, PCM_S16P):
        return x.astype(np.int16)
    if fmt in (PCM_S32, PCM_S32P):
        return np.clip((x.astype(np.int64) + 32768) >> 16, -32768, 32767).astype(np.int16)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(x.astype(np.float32) * np.float32(32768.0))
        v = np.where(np.isnan(v), np.float32(0), v)
        return np.clip(v, -32768, 32767).astype(np.int16)


def mix(x, m):
    """step 2: x (n, S) int16, m (D, S) Q14 -> (n, D) int16"""
    s = x.astype(np.int64) @ np.asarray(m, np.int64).T
    return np.clip((s + 8192) >> 14, -32768, 32767).astype(np.int16)


def positions(n, L, M, P):
    """output indices n -> (input index i, phase)"""
    n = np.asarray(n, np.int64)
    pos = n * M
    i, r = pos // L, pos % L
    ph = r if P == L else (r * P) // L
    return i, ph


def filter_windows(win, ph, coef):
    """win (K, T, D) int16: y[i - H + 1 + k] of each output; ph (K,) -> (K, D) int16"""
    h = coef[ph].astype(np.int64)                                     # (K, T)
    S = np.einsum("kt,ktd->kd", h, win.astype(np.int64))
    return np.clip((S + 16384) >> 15, -32768, 32767).astype(np.int16)


def total_outputs(src, dst, n, flush):
    L, M, P, T, H, _ = params(src, dst)
    if src == dst:
        return n
    if flush:
        return -(-n * L // M)
    return 0 if n <= H else -(-(n - H) * L // M)


def resample_mixed(y, src, dst, coef, flush=True, first=0, count=None):
    """step 3 over a whole mixed stream y (N, D): outputs first .. first + count - 1 (default: all that exist)"""
    L, M, P, T, H, _ = params(src, dst)
    N = y.shape[0]
    if src == dst:
        return y[first:first + (N - first if count is None else count)].copy()
    if count is None:
        count = total_outputs(src, dst, N, flush) - first
    out = np.zeros((count, y.shape[1]), np.int16)
    pad = np.concatenate([np.zeros((H, y.shape[1]), np.int16), y, np.zeros((H + 1, y.shape[1]), np.int16)])
    step = max(1, (1 << 22) // max(1, T * y.shape[1]))
    for a in range(0, count, step):
        n = np.arange(first + a, first + min(count, a + step), dtype=np.int64)
        i, ph = positions(n, L, M, P)
        idx = (i - H + 1)[:, None] + np.arange(T)[None, :] + H          # into pad
        out[a:a + n.size] = filter_windows(pad[idx], ph, coef)
    return out


def statement(fmt, planes, src_channels, src_rate, dst_rate, m, coef, flush=True):
    """the whole chain: planes = list of src_channels arrays (planar) or [interleaved array] -> (n_out, D) int16"""
    if fmt & 1:
        x = np.stack([to_int16(fmt, p) for p in planes], axis=1)
    else:
        x = to_int16(fmt, planes[0]).reshape(-1, src_channels)
    return resample_mixed(mix(x, m), src_rate, dst_rate, coef, flush=flush)


# ---------------------------------------------------------------- the formula the table is rounded from (double)
def taps_double(src, dst):
    """(P, T) float64: h_phi[k] normalised to sum 1 (before rounding)"""
    L, M, P, T, H, factor = params(src, dst)
    ph = np.arange(P, dtype=np.float64)[:, None]
    k = np.arange(T, dtype=np.float64)[None, :]
    x = k - (H - 1) - ph / P
    w = np.clip(1.0 - (x / H) ** 2, 0.0, None)
    h = factor * np.sinc(factor * x) * np.i0(9.0 * np.sqrt(w)) / np.i0(9.0)
    return h / h.sum(axis=1, keepdims=True)
