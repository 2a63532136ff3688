"""The statement of "psxhip disc finish v1" and "psxhip disc check v1"  in numpy: what the disc finisher's
kernels (psxavenc_amd/csrc/disc_kernels.hip) are tested against, byte for byte.

A source is Source(data, size, file, channel, data_subheader): data a (n, >= size) uint8 array, one sector per row, of which the
first `size` bytes are the sector (the rest is junk that nothing reads); size 2352, 2336 or 2048.  A layout is (slot_source, start_lba).
The ECC is written twice: ecc_closed (the closed form of the specification, vectorised over sectors) and ecc_solve (one codeword at
a time: syndromes of the codeword with zero parity, then the 2 x 2 system by elimination); syndromes() evaluates any sector.
"""
from collections import namedtuple

import numpy as np

SYNC, HEADER, SUBHEADER, EDC, ECC_P, ECC_Q, EDC_ABSENT = 1, 2, 4, 8, 16, 32, 64
LBA_LIMIT = 450000
SUMMARY_FIELDS = ("n_sectors", "n_form1", "n_form2", "n_bad", "n_sync", "n_header", "n_subheader", "n_edc", "n_ecc_p", "n_ecc_q",
                  "n_edc_absent", "reserved")
SYNC_BYTES = np.array([0] + [0xFF] * 10 + [0], np.uint8)

Source = namedtuple("Source", "data size file channel data_subheader", defaults=(-1, -1, (0, 0, 0x08, 0)))


class Invalid(ValueError):
    """what the library answers with PSXHIP_EINVAL"""


# ---- GF(2^8), polynomial 0x11D, alpha = 2
GF_EXP = np.zeros(512, np.int64)
GF_LOG = np.zeros(256, np.int64)
_v = 1
for _i in range(255):
    GF_EXP[_i] = _v
    GF_LOG[_v] = _i
    _v <<= 1
    if _v & 0x100:
        _v ^= 0x11D
GF_EXP[255:510] = GF_EXP[0:255]
GF_MUL = np.zeros((256, 256), np.uint8)          # GF_MUL[a, b] = a * b
for _a in range(1, 256):
    GF_MUL[_a, 1:] = GF_EXP[GF_LOG[_a] + GF_LOG[1:256]]
GF_INV3 = int(GF_EXP[255 - GF_LOG[3]])


def gf_mul(a, b):
    return int(GF_MUL[a, b])


def gf_div(a, b):
    assert b != 0
    return 0 if a == 0 else int(GF_EXP[(GF_LOG[a] - GF_LOG[b]) % 255])


# ---- the codewords: indices into d[0..2235] (sector bytes 0xC ..), data symbols then the two parity symbols
P_IDX = np.array([[m + 86 * i for i in range(24)] + [2064 + m, 2064 + 86 + m] for m in range(86)])                          # (86, 26)
Q_DATA_IDX = np.array([[((m >> 1) * 86 + (m & 1) + 88 * i) % 2236 for i in range(43)] for m in range(52)])                 # (52, 43)
P_W = np.array([int(GF_EXP[25 - i]) for i in range(26)])           # alpha^(n-1-i)
Q_W = np.array([int(GF_EXP[44 - i]) for i in range(45)])


def _d_of(sectors):
    """d[0..2235 + 104]: sector bytes 0xC .. 0x92F with the header taken as zero (Q appended so that one array serves both codes)"""
    d = sectors[:, 0xC:0x930].copy()
    d[:, 0:4] = 0
    return d


def _xor_reduce(a, axis):
    return np.bitwise_xor.reduce(a, axis=axis)


def ecc_closed(sectors):
    """P and Q of (n, 2352) form-1 sectors by the closed form: A = sum c_i, B = sum alpha^(n-1-i) c_i over the data symbols, first parity
    byte (A ^ B) / 3, second that ^ A.  Writes P (0x81C..0x8C7) then Q (0x8C8..0x92F) in place; Q reads the P just written."""
    d = _d_of(sectors)
    c = d[:, P_IDX[:, :24]]                                    # (n, 86, 24)
    a = _xor_reduce(c, 2)
    b = _xor_reduce(GF_MUL[P_W[:24][None, None, :], c], 2)
    p0 = GF_MUL[GF_INV3, a ^ b]
    sectors[:, 0x81C:0x81C + 86] = p0
    sectors[:, 0x81C + 86:0x8C8] = p0 ^ a
    d = _d_of(sectors)
    c = d[:, Q_DATA_IDX]                                       # (n, 52, 43)
    a = _xor_reduce(c, 2)
    b = _xor_reduce(GF_MUL[Q_W[:43][None, None, :], c], 2)
    q0 = GF_MUL[GF_INV3, a ^ b]
    sectors[:, 0x8C8:0x8C8 + 52] = q0
    sectors[:, 0x8C8 + 52:0x930] = q0 ^ a
    return sectors


def _solve_codeword(data):
    """the two parity symbols (x, y) that give the codeword data + [x, y] zero syndromes at alpha^0 and alpha^1"""
    n = len(data) + 2
    s0 = s1 = 0
    for c in list(data) + [0, 0]:          # Horner: the polynomial sum c_i z^(n-1-i) at z = 1 and z = alpha
        s0 ^= int(c)
        s1 = gf_mul(s1, 2) ^ int(c)
    assert n in (26, 45)
    # x + y = s0;  alpha x + y = s1: eliminate y
    x = gf_div(s0 ^ s1, 1 ^ 2)
    y = s0 ^ x
    return x, y


def ecc_solve(sector):
    """P and Q of ONE 2352-byte form-1 sector, codeword by codeword (in place)"""
    d = _d_of(sector[None, :])[0]
    for m in range(86):
        x, y = _solve_codeword(d[P_IDX[m, :24]])
        sector[0x81C + m], sector[0x81C + 86 + m] = x, y
    d = _d_of(sector[None, :])[0]
    for m in range(52):
        x, y = _solve_codeword(d[Q_DATA_IDX[m]])
        sector[0x8C8 + m], sector[0x8C8 + 52 + m] = x, y
    return sector


def syndromes(sectors):
    """(n, 86, 2) and (n, 52, 2): sum c_i and sum alpha^(n-1-i) c_i of every P and Q codeword, parity symbols included"""
    d = _d_of(sectors)
    cp = d[:, P_IDX]
    q = sectors[:, 0x8C8:0x930]
    cq = np.concatenate([d[:, Q_DATA_IDX], q[:, :52, None], q[:, 52:, None]], axis=2)
    sp = np.stack([_xor_reduce(cp, 2), _xor_reduce(GF_MUL[P_W[None, None, :], cp], 2)], axis=2)
    sq = np.stack([_xor_reduce(cq, 2), _xor_reduce(GF_MUL[Q_W[None, None, :], cq], 2)], axis=2)
    return sp, sq


# ---- EDC: polynomial 0xD8018001 reflected, zero init, no final xor (cdrom.c:28-41)
EDC_TAB = np.zeros(256, np.uint32)
for _i in range(256):
    _v = _i
    for _k in range(8):
        _v = (_v >> 1) ^ (0xD8018001 if _v & 1 else 0)
    EDC_TAB[_i] = _v


def edc(spans):
    """EDC of every row of an (n, k) uint8 array"""
    c = np.zeros(spans.shape[0], np.uint32)
    for i in range(spans.shape[1]):
        c = (c >> np.uint32(8)) ^ EDC_TAB[(c ^ spans[:, i]) & np.uint32(0xFF)]
    return c


def _put_le32(sectors, at, words):
    for k in range(4):
        sectors[:, at + k] = (words >> np.uint32(8 * k)) & np.uint32(0xFF)


def _get_le32(sectors, at):
    w = np.zeros(sectors.shape[0], np.uint32)
    for k in range(4):
        w |= sectors[:, at + k].astype(np.uint32) << np.uint32(8 * k)
    return w


def bcd(v):
    return v + (v // 10) * 6


def header(lba):
    t = lba + 150
    return [bcd(t // 4500), bcd((t // 75) % 60), bcd(t % 75), 2]


# ---- the schedule
def plan(slot_source, sources):
    period = len(slot_source)
    if not 1 <= period <= 64 or len(sources) > 64:
        raise Invalid("period or source count")
    counts = [0] * len(sources)
    for s in slot_source:
        if not -1 <= s < len(sources):
            raise Invalid("slot names no source")
        if s >= 0:
            counts[s] += 1
    rounds = 0
    for s, src in enumerate(sources):
        n = src.data.shape[0]
        if src.size not in (2352, 2336, 2048) or not -1 <= src.file <= 255 or not -1 <= src.channel <= 31:
            raise Invalid("source")
        if src.size == 2048 and src.data_subheader[2] & 0x20:
            raise Invalid("a 2048-byte source is never form 2")
        if n and not counts[s]:
            raise Invalid("a source with sectors owns no slot")
        if n:
            rounds = max(rounds, -(-n // counts[s]))
    return period * rounds


def schedule(slot_source, sources, j):
    """(source, sector number) of output sector j of the schedule, or None for the null sector"""
    period = len(slot_source)
    q = j % period
    s = slot_source[q]
    if s < 0:
        return None
    count = sum(1 for x in slot_source if x == s)
    rank = sum(1 for x in slot_source[:q] if x == s)
    k = (j // period) * count + rank
    return (s, k) if k < sources[s].data.shape[0] else None


def finish(slot_source, start_lba, sources, first_out=0, n_out=None):
    """the image's sectors first_out .. first_out + n_out - 1 as an (n_out, 2352) uint8 array"""
    total = plan(slot_source, sources)
    if n_out is None:
        n_out = total - first_out
    if start_lba < 0 or first_out < 0 or n_out < 0 or (n_out and start_lba + first_out + n_out - 1 + 150 >= LBA_LIMIT):
        raise Invalid("lba")
    out = np.zeros((n_out, 2352), np.uint8)
    for i in range(n_out):
        j = first_out + i
        sec = out[i]
        sec[0:12] = SYNC_BYTES
        sec[12:16] = header(start_lba + j)
        at = schedule(slot_source, sources, j)
        if at is None:
            sub = [0, 0, 0x20, 0]
            body = None
        else:
            src = sources[at[0]]
            row = src.data[at[1], :src.size]
            if src.size == 2048:
                sub, body = list(src.data_subheader), np.concatenate([np.zeros(24, np.uint8), row])      # body: as if a raw sector
            else:
                body = np.concatenate([np.zeros(2352 - src.size, np.uint8), row])
                sub = [int(x) for x in body[0x10:0x14]]
            if src.file >= 0:
                sub[0] = src.file
            if src.channel >= 0:
                sub[1] = (sub[1] & 0xE0) | (src.channel & 0x1F)
        sec[0x10:0x14] = sub
        sec[0x14:0x18] = sub
        end = 0x92C if sub[2] & 0x20 else 0x818
        if body is not None:
            sec[0x18:end] = body[0x18:end]
    form2 = (out[:, 0x12] & 0x20) != 0
    if form2.any():
        part = out[form2]
        _put_le32(part, 0x92C, edc(part[:, 0x10:0x92C]))
        out[form2] = part
    if (~form2).any():
        part = out[~form2]
        _put_le32(part, 0x818, edc(part[:, 0x10:0x818]))
        out[~form2] = ecc_closed(part)
    return out


def check(image, start_lba=-1):
    """status bits per sector of an (n, 2352) uint8 array, and the summary as a dict"""
    n = image.shape[0]
    st = np.zeros(n, np.int32)
    if n == 0:
        return st, dict.fromkeys(SUMMARY_FIELDS, 0)
    st[(image[:, :12] != SYNC_BYTES).any(axis=1)] |= SYNC
    if start_lba >= 0:
        want = np.array([header(start_lba + j) for j in range(n)], np.uint8)
        st[(image[:, 12:16] != want).any(axis=1)] |= HEADER
    else:
        msf = image[:, 12:15]
        st[(image[:, 15] != 2) | ((msf & 0x0F) > 9).any(axis=1) | ((msf >> 4) > 9).any(axis=1)] |= HEADER
    st[(image[:, 0x10:0x14] != image[:, 0x14:0x18]).any(axis=1)] |= SUBHEADER
    form2 = (image[:, 0x12] & 0x20) != 0
    if form2.any():
        part = image[form2]
        stored, want = _get_le32(part, 0x92C), edc(part[:, 0x10:0x92C])
        bits = np.where(stored == 0, EDC_ABSENT, np.where(stored != want, EDC, 0)).astype(np.int32)
        st[form2] |= bits
    if (~form2).any():
        part = image[~form2]
        bits = np.where(_get_le32(part, 0x818) != edc(part[:, 0x10:0x818]), EDC, 0).astype(np.int32)
        sp, sq = syndromes(part)
        bits |= np.where(sp.reshape(len(part), -1).any(axis=1), ECC_P, 0).astype(np.int32)
        bits |= np.where(sq.reshape(len(part), -1).any(axis=1), ECC_Q, 0).astype(np.int32)
        st[~form2] |= bits
    summary = dict(n_sectors=n, n_form1=int((~form2).sum()), n_form2=int(form2.sum()), n_bad=int((st != 0).sum()), reserved=0)
    for name, bit in (("n_sync", SYNC), ("n_header", HEADER), ("n_subheader", SUBHEADER), ("n_edc", EDC), ("n_ecc_p", ECC_P),
                      ("n_ecc_q", ECC_Q), ("n_edc_absent", EDC_ABSENT)):
        summary[name] = int(((st & bit) != 0).sum())
    return st, summary
