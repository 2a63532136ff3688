""""psxhip ADPCM decode v1"  in numpy / Python integers: the statement the decoder's C++ core
(psxavenc_amd/csrc/adpcm_decode_core.h) and kernels are held to -- the role tests/mdec_recon_ref.py plays for the MDEC decoder.
It is itself pinned to the reference's encoder (tests/test_adpcm_decode_ref.py): decoding a unit the reference encoded gives the
reference's (prev1, prev2), and the squared error against the unit's input its mse (libpsxav/adpcm.c:120-136).

Integers only; >> is arithmetic.  A record is PSXHIP_ADPCM_RECORD_SIZE(bits) bytes: 4-bit = an SPU block (header, loop flags,
14 bytes of two codes, even sample low); 8-bit = header, 3 unused bytes, 28 codes."""
import numpy as np

K1 = (0, 60, 115, 98, 122)
K2 = (0, 0, -52, -55, -60)
FLAG_FILTER, FLAG_SHIFT = 1, 2


def record_bytes(bits):
    return 16 if bits == 4 else 32


def unpack_codes(record, bits):
    """the 28 codes of one record as unsigned numbers of `bits` bits"""
    record = np.asarray(record, np.uint8)
    if bits == 4:
        b = record[2:16].astype(np.int64)
        return np.stack([b & 15, b >> 4], axis=1).reshape(28)
    return record[4:32].astype(np.int64)


def decode_unit(record, bits, filter_count, p1, p2):
    """-> (28 int64 samples, p1, p2, flags)"""
    R = 12 if bits == 4 else 8
    h = int(record[0])
    s = h & 15
    f = h >> 4
    if filter_count == 4:
        f &= 3
    flags = 0
    if f >= 5:
        k1 = k2 = 0
        flags |= FLAG_FILTER
    else:
        k1, k2 = K1[f], K2[f]
    if s > R:
        flags |= FLAG_SHIFT
    out = np.zeros(28, np.int64)
    for i, c in enumerate(unpack_codes(record, bits)):
        t = (int(c) << R) & 0xFFFF
        t = (t - 0x10000 if t & 0x8000 else t) >> s
        d = t + ((k1 * p1 + k2 * p2 + 32) >> 6)
        d = max(-32768, min(32767, d))
        out[i] = d
        p2, p1 = p1, d
    return out, p1, p2, flags


def decode_chain(records, bits, filter_count, state=(0, 0)):
    """records: (n, record_bytes) uint8 in chain order -> (28 n int16 samples, (p1, p2), n flag bytes)"""
    records = np.asarray(records, np.uint8).reshape(-1, record_bytes(bits))
    p1, p2 = int(state[0]), int(state[1])
    pcm = np.zeros(28 * len(records), np.int16)
    flags = np.zeros(len(records), np.uint8)
    for u, r in enumerate(records):
        out, p1, p2, flags[u] = decode_unit(r, bits, filter_count, p1, p2)
        pcm[28 * u:28 * u + 28] = out
    return pcm, (p1, p2), flags


def unit_sse(decoded, original):
    """sum of squared errors per unit of 28 samples, as Python-exact uint64 (a unit can pass 2^32); `original` is zero-padded"""
    a = np.asarray(decoded, np.int64)
    b = np.zeros(a.size, np.int64)
    o = np.asarray(original, np.int64)[:a.size]
    b[:o.size] = o
    return ((a - b) ** 2).reshape(-1, 28).sum(axis=1).astype(np.uint64)


def xa_sector_records(sector, bits):
    """one XA sector (2336 or 2352 bytes) -> its 18 * U unit records in encode order (U = 8 for 4-bit, 4 for 8-bit): the inverse of
    the reference's sound-group layout (adpcm.c:193-233)"""
    sector = np.asarray(sector, np.uint8)
    data = sector[len(sector) - 2336 + 8:][:18 * 128].reshape(18, 128)
    upg = 8 if bits == 4 else 4
    rec = np.zeros((18, upg, record_bytes(bits)), np.uint8)
    for g in range(18):
        grp = data[g]
        words = grp[16:].reshape(28, 4)
        for n in range(upg):
            if bits == 4:
                rec[g, n, 0] = grp[n if n < 4 else n + 4]
                nib = (words[:, n >> 1] >> (4 * (n & 1))) & 15
                rec[g, n, 2:] = nib[0::2] | (nib[1::2] << 4)
            else:
                rec[g, n, 0] = grp[n]
                rec[g, n, 4:] = words[:, n]
    return rec.reshape(18 * upg, record_bytes(bits))


def decode_xa(sectors, sector_size, bits, stereo, states=None):
    """sectors: bytes of whole sectors -> (pcm int16, interleaved L,R when stereo; [(p1, p2)] per channel)"""
    sectors = np.asarray(sectors, np.uint8).reshape(-1, sector_size)
    ch = 2 if stereo else 1
    rec = np.concatenate([xa_sector_records(s, bits) for s in sectors])
    st = [(0, 0)] * ch if states is None else [tuple(int(v) for v in s) for s in states]
    out = np.zeros((len(rec) // ch * 28, ch), np.int16)
    for c in range(ch):
        out[:, c], st[c], _ = decode_chain(rec[c::ch], bits, 4, st[c])
    return out.reshape(-1), st


def fixed_point_stream(n_units):
    """filter 1, shift 12, all codes 0: 0, 8 and -7 are all fixed points of (60 p + 32) >> 6 -- a wrong start state survives for ever"""
    rec = np.zeros((n_units, 16), np.uint8)
    rec[:, 0] = 0x1C
    return rec


def random_records(seed, bits, n):
    """records of seeded random bytes whose headers cover all 256 values"""
    rng = np.random.default_rng(seed)
    rec = rng.integers(0, 256, (n, record_bytes(bits))).astype(np.uint8)
    assert n >= 256
    rec[:256, 0] = rng.permutation(256).astype(np.uint8)
    return rec
