"""The ADPCM encoder's adversarial chain tables, shared by tests/test_adpcm_encode_corpus.py (CPU) and tests/test_gpu_adpcm_chains.py:
what psxhip_adpcm_chain_t (include/psxav_hip.h) promises, laid out so that a wrong read or a wrong write changes bytes and never
leaves an allocation.  Everything here is a pure function of its parameters and uses numpy and the CPU oracle only.

A case is (coding, layout, n_chains).  Chain c of every case has the same content, start state and unit count; the layout decides
where its samples and records lie:
  odd        pitch 1, chains 3 samples apart from element 1 on (every alignment), sample_limit cycling through the full span,
             28 (n - 1) + 5, 28 (n - 1) + 1, 0 and a value past the last unit
  pairs      pitch 2, unit_stride 2: chains 2p and 2p + 1 interleave both ways (the XA stereo shape), their lengths differ
  quads      groups of 3 chains at pitch 3 and of 4 chains at pitch 4 in turn, unit_stride = pitch (the SPUI multi-channel shape)
  scattered  unit_base in descending chain order, unit_stride 3: two of every three records belong to nobody
Every sample no chain may read -- the gaps, and everything at or past a chain's sample_limit -- is poison (32767 / -32768 in turn);
the record buffer is filled with a canary byte and has 64 records of it behind the last record.  The expected image is written by
orc_adpcm_encode_unit, unit by unit, from a zero-padded copy of the chain's samples gathered by (offset, pitch, limit)."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np

import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adpcm_chain_corpus_ref.npz")

SEED = 47
CODINGS = [(5, 4), (4, 4), (4, 8)]                      # (filter_count, bits): SPU, XA 4-bit, XA 8-bit
LAYOUTS = ["odd", "pairs", "quads", "scattered"]
CHAIN_COUNTS = [1, 3, 4, 5, 6, 9, 11, 64, 65, 130]
UNIT_COUNTS = (33, 0, 7, 1, 2)
MAX_CHAINS, MAX_UNITS = 130, 33
CANARY = 0xA5
TAIL_RECORDS = 64
POISON = (32767, -32768)
N_KINDS = 11
XA_LAYOUTS = [(fmt, stereo, bits) for fmt in (0, 1) for stereo in (0, 1) for bits in (4, 8)]
XA_SECTORS = 5

# psxhip_adpcm_chain_t; the GPU test checks it against psxavenc_amd.adpcm.CHAIN_DTYPE
CHAIN_DTYPE = np.dtype([("sample_offset", "<i8"), ("pitch", "<i4"), ("sample_limit", "<i4"), ("n_units", "<i4"), ("unit_stride", "<i4")])

_STATES = [(0, 0), (1, -1), (-1, 1), (32767, 32767), (-32768, -32768), (32767, -32768), (-32768, 32767), (0, 32767), (-32768, 0),
           None, (32767, 0), None]                       # None: random int16


def record_bytes(bits):
    return 16 if bits == 4 else 32


def shift_range(bits):
    return 12 if bits == 4 else 8


def content(c, n):
    """n samples of chain c: the six kinds of synth_pcm, then rails, full-scale alternation, spikes over +-40 noise, a constant rail,
    and a loud square wave that decays into silence (ties between candidates)"""
    kind = c % N_KINDS
    rng = np.random.default_rng(SEED * 1000 + c)
    i = np.arange(n)
    if kind < 6:
        return O.synth_pcm(SEED, c, 0, n, kind)
    if kind == 6:
        x = rng.choice(np.array([-32768, -1, 0, 1, 32767]), n)
    elif kind == 7:
        x = np.where((i // (1 + 2 * (c % 2))) % 2 == 0, 32767, -32768)
    elif kind == 8:
        x = np.where(rng.random(n) < 0.05, rng.choice(np.array([-32768, 32767]), n), rng.integers(-40, 40, n))
    elif kind == 9:
        x = np.full(n, 32767 if c % 2 else -32768)
    else:
        x = np.where((i // 9) % 2 == 0, 30000, -30000) * (i < 40)
    return x.astype(np.int16)


def start_state(c):
    s = _STATES[c % len(_STATES)]
    if s is None:
        s = tuple(int(v) for v in np.random.default_rng(SEED * 77 + c).integers(-32768, 32768, 2))
    return s


def unit_count(c):
    """mixed inside every wavefront of 4 chains or 5 chunks; chain 0 has the longest"""
    return UNIT_COUNTS[(c + c // 5) % 5]


# ---- the oracle, unit by unit ----------------------------------------------------------------------------------------------------
_TAP1, _TAP2 = (0, 60, 115, 98, 122), (0, 0, -52, -55, -60)


def _bind():
    L = O.lib()
    cp, u8 = C.POINTER(O.Chan), C.POINTER(C.c_uint8)
    L.orc_adpcm_encode_unit.argtypes = [cp, O.i16p, C.c_int, C.c_int, C.c_int, C.c_int, u8]
    L.orc_adpcm_encode_unit.restype = C.c_uint8
    L.orc_adpcm_trial.argtypes = [cp, O.i16p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u8]
    L.orc_adpcm_trial.restype = C.c_uint64
    L.orc_adpcm_find_min_shift.argtypes = [cp, O.i16p, C.c_int, C.c_int, C.c_int, C.c_int]
    return L


def pack_record(header, codes, bits):
    """a unit's record as store_record / store_spu_block (adpcm_kernels.hip) write it.  4 bits: an SPU block -- header, 0, fourteen
    bytes of two codes each, the even sample low.  8 bits: header, three zero bytes, the 28 codes."""
    rec = np.zeros(record_bytes(bits), np.uint8)
    rec[0] = header
    if bits == 4:
        rec[2:] = (codes[0::2] & 0x0F) | ((codes[1::2] & 0x0F) << 4)
    else:
        rec[4:] = codes
    return rec


def _clamped(header, codes, state, bits):
    """whether the decoder's sum leaves int16 somewhere in the unit (adpcm.c:118-124), and the state behind it"""
    rng = shift_range(bits)
    f, sh = header >> 4, header & 15
    p1, p2 = state
    hit = False
    for q in codes.tolist():
        step = (q << rng) & 0xFFFF
        step = (step - 0x10000 if step & 0x8000 else step) >> sh
        dec = step + ((_TAP1[f] * p1 + _TAP2[f] * p2 + 32) >> 6)
        if dec > 32767 or dec < -32768:
            hit = True
            dec = max(-32768, min(32767, dec))
        p1, p2 = dec, p1
    return hit, (p1, p2)


def encode_units(x, state, n_units, filter_count, bits, stats=False):
    """x: the chain's samples, zeros behind its limit (at least 28 n_units of them).
    -> (records (n, record bytes), state after every unit (n, 2) int32, per-unit coverage rows when asked for:
    (filter, shift, tie, saturated loser, clamped))"""
    L = _bind()
    rng = shift_range(bits)
    x = np.ascontiguousarray(x[:28 * n_units], dtype=np.int16)
    st = O.Chan(int(state[0]), int(state[1]))
    rec = np.zeros((n_units, record_bytes(bits)), np.uint8)
    after = np.zeros((n_units, 2), np.int32)
    rows = np.zeros((n_units, 5), np.int32)
    codes = (C.c_uint8 * 28)()
    scratch = (C.c_uint8 * 28)()
    for u in range(n_units):
        px = O.ptr(x[28 * u:], O.i16p)
        before = (st.prev1, st.prev2)
        if stats:
            errs = []
            for f in range(filter_count):
                m = L.orc_adpcm_find_min_shift(C.byref(st), px, 28, 1, f, rng)
                for s in range(max(m - 1, 0), min(m + 1, rng) + 1):
                    trial = O.Chan(*before)
                    errs.append(int(L.orc_adpcm_trial(C.byref(trial), px, 28, 1, f, s, rng, scratch)))
        h = int(L.orc_adpcm_encode_unit(C.byref(st), px, 28, 1, filter_count, rng, codes))
        cc = np.frombuffer(codes, np.uint8).copy()
        rec[u] = pack_record(h, cc, bits)
        after[u] = (st.prev1, st.prev2)
        if stats:
            hit, end = _clamped(h, cc, before, bits)
            assert end == (st.prev1, st.prev2), "the decode restated here disagrees with the oracle"
            rows[u] = (h >> 4, h & 15, errs.count(min(errs)) > 1, max(errs) >= 1 << 32 and min(errs) < 1 << 32, hit)
    return rec, after, rows


@functools.lru_cache(maxsize=None)
def _chain(filter_count, bits, c, valid, stats=False):
    """chain c with `valid` samples in front of the zeros"""
    n = unit_count(c)
    x = np.zeros(28 * n, np.int16)
    x[:valid] = content(c, 28 * MAX_UNITS)[:valid]
    return encode_units(x, start_state(c), n, filter_count, bits, stats)


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
def table(off, pitch, limit, n, stride):
    ch = np.zeros(len(off), CHAIN_DTYPE)
    ch["sample_offset"], ch["pitch"], ch["sample_limit"], ch["n_units"], ch["unit_stride"] = off, pitch, limit, n, stride
    return ch


def layout(name, n_chains):
    """-> (chains, unit_base, sample buffer, n_records)"""
    n = np.array([unit_count(c) for c in range(n_chains)], np.int64)
    span = 28 * n
    limit = span.copy()
    if name == "odd":
        off = 1 + np.concatenate([[0], np.cumsum(span + 3)[:-1]])
        for c in range(n_chains):
            limit[c] = (span[c], max(span[c] - 23, 0), max(span[c] - 27, 0), 0, span[c] + 45)[c % 5]
        chains = table(off, 1, limit, n, 1)
        base = np.concatenate([[0], np.cumsum(n)[:-1]])
        n_records = int(n.sum())
    elif name == "pairs":
        pair = np.arange(n_chains) // 2
        longest = np.array([n[2 * p:2 * p + 2].max() for p in range((n_chains + 1) // 2)], np.int64)
        region = np.concatenate([[0], np.cumsum(2 * 28 * longest + 6)[:-1]])
        rec0 = np.concatenate([[0], np.cumsum(2 * longest)[:-1]])
        chains = table(region[pair] + np.arange(n_chains) % 2, 2, limit, n, 2)
        base = rec0[pair] + np.arange(n_chains) % 2
        n_records = int(2 * longest.sum())
    elif name == "quads":
        off, base, pitch = [], [], []
        at = rec = c = 0
        g = 0
        while c < n_chains:
            p = 3 if g % 2 == 0 else 4
            members = list(range(c, min(c + p, n_chains)))
            longest = int(n[members].max())
            for k, m in enumerate(members):
                off.append(at + k)
                base.append(rec + k)
                pitch.append(p)
            at += p * 28 * longest + 5
            rec += p * longest
            c += p
            g += 1
        chains = table(off, pitch, limit, n, pitch)
        base = np.array(base)
        n_records = rec
    else:
        assert name == "scattered"
        off = np.concatenate([[0], np.cumsum(span + 5)[:-1]])
        chains = table(off, 1, limit, n, 3)
        behind = np.concatenate([np.cumsum(n[::-1])[::-1][1:], [0]])          # units of the chains after c
        base = 3 * behind + 1
        n_records = int(3 * n.sum())
    total = int((chains["sample_offset"] + chains["pitch"] * np.maximum(span, chains["sample_limit"])).max()) + 64
    buf = np.where(np.arange(total) % 2 == 0, POISON[0], POISON[1]).astype(np.int16)
    for c in range(n_chains):
        valid = valid_samples(chains[c])
        buf[int(chains["sample_offset"][c]) + int(chains["pitch"][c]) * np.arange(valid)] = content(c, 28 * MAX_UNITS)[:valid]
    return chains, base.astype(np.int32), buf, n_records


def valid_samples(chain):
    return int(min(chain["sample_limit"], 28 * chain["n_units"]))


class Case:
    """one (coding, layout, chain count): the tables, the sample buffer, the start states, the expected record image (n_records +
    TAIL_RECORDS records, canary where nothing is written) and the expected end states"""

    def __init__(self, filter_count, bits, name, n_chains, stats=False):
        self.filter_count, self.bits, self.layout, self.n_chains = filter_count, bits, name, n_chains
        self.chains, self.unit_base, self.samples, self.n_records = layout(name, n_chains)
        self.start = np.array([start_state(c) for c in range(n_chains)], np.int32).reshape(n_chains, 2)
        self.image = np.full((self.n_records + TAIL_RECORDS, record_bytes(bits)), CANARY, np.uint8)
        self.final = self.start.copy()
        self.owner = np.full(self.n_records + TAIL_RECORDS, -1, np.int32)
        self.rows = []
        for c in range(n_chains):
            rec, after, rows = _chain(filter_count, bits, c, valid_samples(self.chains[c]), stats)
            idx = int(self.unit_base[c]) + int(self.chains["unit_stride"][c]) * np.arange(len(rec))
            assert (self.owner[idx] == -1).all() and (idx < self.n_records).all(), "two chains own one record"
            self.owner[idx] = c
            self.image[idx] = rec
            if len(rec):
                self.final[c] = after[-1]
            self.rows.append((c, rows, after))

    def chain_records(self, c):
        n, s = int(self.chains["n_units"][c]), int(self.chains["unit_stride"][c])
        return self.image[int(self.unit_base[c]) + s * np.arange(n)]

    def cut(self, cuts):
        """the tables of the two halves of every chain, cut behind unit cuts[c]: (chains, unit_base) twice"""
        cuts = np.asarray(cuts, np.int64)
        a, b = self.chains.copy(), self.chains.copy()
        a["n_units"] = cuts
        b["n_units"] = self.chains["n_units"] - cuts
        b["sample_offset"] = self.chains["sample_offset"] + 28 * cuts * self.chains["pitch"]
        b["sample_limit"] = np.maximum(self.chains["sample_limit"] - 28 * cuts, 0)
        return (a, self.unit_base), (b, (self.unit_base + cuts * self.chains["unit_stride"]).astype(np.int32))


@functools.lru_cache(maxsize=None)
def case(filter_count, bits, name, n_chains):
    return Case(filter_count, bits, name, n_chains)


def coverage(filter_count, bits):
    """the coverage rows of every unit of the coding's corpus (all layouts at MAX_CHAINS; only `odd` has limits of its own):
    (filter, shift, tie, saturated loser, clamped, started from a rail state)"""
    out = []
    seen = set()
    for name in ("odd", "pairs"):
        k = Case(filter_count, bits, name, MAX_CHAINS, stats=True)
        for c, rows, after in k.rows:
            key = (c, valid_samples(k.chains[c]))
            if key in seen or not len(rows):
                continue
            seen.add(key)
            before = np.concatenate([k.start[c:c + 1], after[:-1]])
            rail = ((before == 32767) | (before == -32768)).any(axis=1)
            out.append(np.concatenate([rows, rail[:, None].astype(np.int32)], axis=1))
    return np.concatenate(out)


# ---- what the reference can express ------------------------------------------------------------------------------------------------
def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def spu_key(name, n_chains):
    return "spu_%s_%d" % (name, n_chains)


def spu_ours(name, n_chains):
    """(blocks of every chain in chain order, end states) of the expected image"""
    k = case(5, 4, name, n_chains)
    return np.concatenate([k.chain_records(c) for c in range(n_chains)]), k.final


def spu_reference(name, n_chains):
    """the same through the reference's psx_audio_spu_encode, reading the poisoned buffer itself with the chain's pitch: the valid
    samples in one call, the units of zeros behind them in a second one that carries the state"""
    k = case(5, 4, name, n_chains)
    blocks, final = [], k.start.copy()
    for c in range(n_chains):
        n, valid = int(k.chains["n_units"][c]), valid_samples(k.chains[c])
        st = O.RefChan(0, 0, int(k.start[c, 0]), int(k.start[c, 1]))
        out = np.zeros((0,), np.uint8)
        if valid:
            out, st = O.ref_spu_encode(k.samples[int(k.chains["sample_offset"][c]):], int(k.chains["pitch"][c]), st, valid)
        done = out.size // 16
        if done < n:
            more, st = O.ref_spu_encode(np.zeros(28 * (n - done), np.int16), 1, st)
            out = np.concatenate([out, more])
        blocks.append(out.reshape(-1, 16))
        final[c] = (st.prev1, st.prev2)
    return np.concatenate(blocks), final


def xa_key(fmt, stereo, bits):
    return "xa_f%d_s%d_b%d" % (fmt, stereo, bits)


def xa_start(stereo):
    return np.array([[32767, -32768], [-1234, 777]][:2 if stereo else 1], np.int32)


@functools.lru_cache(maxsize=None)
def xa_stream(stereo, bits):
    """XA_SECTORS whole sectors of one stream as the `pairs` layout holds a stereo pair (a lone chain at pitch 1 when mono):
    (pcm, chains, unit_base, records in encode order, end states).  The first k sectors' records are a prefix."""
    ch = 2 if stereo else 1
    per = 18 * (8 if bits == 4 else 4) // ch * XA_SECTORS                  # units per channel
    pcm = np.zeros(28 * per * ch, np.int16)
    rec = np.zeros((per * ch, record_bytes(bits)), np.uint8)
    start = xa_start(stereo)
    final = start.copy()
    for c in range(ch):
        x = content(2 + 6 * c if bits == 4 else 8 - 8 * c, 28 * per)    # noise | spikes, the other side spikes | loud tones
        pcm[c::ch] = x
        rec[c::ch], after, _ = encode_units(x, start[c], per, 4, bits)
        final[c] = after[-1]
    chains = table(np.arange(ch), ch, 28 * per, per, ch)
    return pcm, chains, np.arange(ch, dtype=np.int32), rec, final


def sound_groups(rec, bits):
    """18 x 128 bytes per sector from records in encode order (adpcm.c:193-233, 317-318)"""
    upg = 8 if bits == 4 else 4
    g = np.zeros((len(rec) // upg, 128), np.uint8)
    for u in range(upg):
        r = rec[u::upg]
        if bits == 4:
            g[:, (u & 3) + ((u & 4) << 1)] = r[:, 0]
            codes = np.stack([r[:, 2:] & 0x0F, r[:, 2:] >> 4], axis=2).reshape(len(r), 28)
            g[:, 0x10 + (u >> 1):0x80:4] |= codes << (4 * (u & 1))
        else:
            g[:, u] = r[:, 0]
            g[:, 0x10 + u:0x80:4] = r[:, 4:]
    g[:, 4:8] = g[:, 0:4]
    g[:, 12:16] = g[:, 8:12]
    return g.reshape(-1, 18 * 128)


def xa_sectors(fmt, stereo, bits, use_ref, lba=0):
    """the stream's sectors from the reference (or the restatement) in one call: ((XA_SECTORS, sector size), end states (ch, 2))"""
    pcm, _, _, _, _ = xa_stream(stereo, bits)
    s = O.XaSettings(fmt, stereo, 37800, bits, 1, 2)
    start = xa_start(stereo)
    n = pcm.size // (2 if stereo else 1)
    if use_ref:
        st = O.RefState()
        st.left.prev1, st.left.prev2 = int(start[0, 0]), int(start[0, 1])
        if stereo:
            st.right.prev1, st.right.prev2 = int(start[1, 0]), int(start[1, 1])
        data, st = O.ref_xa_encode(s, pcm, n, lba=lba, state=st)
    else:
        st = O.State(O.Chan(int(start[0, 0]), int(start[0, 1])), O.Chan(*(int(v) for v in start[-1])))
        data, st = O.xa_encode(s, pcm, n, lba=lba, state=st)
    final = np.array([[st.left.prev1, st.left.prev2], [st.right.prev1, st.right.prev2]], np.int32)[:2 if stereo else 1]
    return data.reshape(XA_SECTORS, -1), final


def xa_group_bytes(sectors, fmt):
    o = 8 if fmt == 0 else 24
    return sectors[:, o:o + 18 * 128]


_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
        assert _golden["meta"].tolist() == [SEED, MAX_CHAINS, MAX_UNITS, N_KINDS, XA_SECTORS], "the fixture was made for other parameters"
    return _golden
