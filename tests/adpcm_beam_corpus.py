"""The beam encoder's corpus, shared by the CPU tests of "psxhip ADPCM beam v1" and tests/test_gpu_adpcm_beam.py: the chains of
tests/adpcm_encode_corpus.py -- every content kind with the adversarial start states, in its four layouts -- and a few chains more
whose content makes the rule's corners happen, with the statement's records, errors and states for them (tests/adpcm_beam_ref.py's
numpy form, computed once per coding and beam; the CPU tests hold it equal to the plain form).  numpy and the CPU oracle only."""
import ctypes as C
import functools

import numpy as np

import adpcm_beam_ref as B
import adpcm_decode_ref as R
import adpcm_encode_corpus as K
import oracle_lib as O

CODINGS = K.CODINGS
BEAMS = (1, 2, 3, 4)
N_CORPUS = 24                    # chains 0 .. 23 of the encoder corpus: all 11 content kinds, all 12 start states
N_CHAINS = N_CORPUS + 4
EXTRA_UNITS = 6


def unit_count(c):
    return K.unit_count(c) if c < N_CORPUS else EXTRA_UNITS


def start_state(c):
    return K.start_state(c) if c < N_CORPUS else ((0, 0), (300, -200), (32767, 32767), (-32768, -32768))[c - N_CORPUS]


def content(c, n):
    """the encoder corpus's content, then: silence (every pool child of a step ties with its mirror image), a quiet sine over a slow
    ramp (delayed decisions pay), a signal that sits just below the positive rail and one just above the negative rail (the greedy
    code is hi or lo, the child beyond it is dropped)"""
    if c < N_CORPUS:
        return K.content(c, n)
    i = np.arange(n)
    rng = np.random.default_rng(K.SEED * 31 + c)
    if c == N_CORPUS:
        x = np.zeros(n)
    elif c == N_CORPUS + 1:
        x = 900 * np.sin(i * 0.37) + 5000 * np.sin(i * 0.021) + rng.integers(-30, 30, n)
    elif c == N_CORPUS + 2:
        x = 32767 - rng.integers(0, 3000, n) * (i % 5 == 0)
    else:
        x = -32768 + rng.integers(0, 3000, n) * (i % 5 == 0)
    return np.asarray(x).astype(np.int16)


def samples(c, valid=None):
    """chain c's samples with zeros from `valid` on"""
    n = 28 * unit_count(c)
    x = np.zeros(max(n, 28), np.int16)
    valid = n if valid is None else min(valid, n)
    x[:valid] = content(c, 28 * K.MAX_UNITS)[:valid]
    return x


@functools.lru_cache(maxsize=None)
def expected(filter_count, bits, beam, with_stats=False):
    """every chain of the corpus side by side: (records (C, 33, record bytes), e (C, 33), state after every unit (C, 33, 2),
    picks (C, 33, 3), what the candidates met)"""
    xs = np.zeros((N_CHAINS, 28 * K.MAX_UNITS), np.int16)
    for c in range(N_CHAINS):
        x = samples(c)
        xs[c, :len(x)] = x
    stats = set() if with_stats else None
    out = B.encode_chains_np(xs, [start_state(c) for c in range(N_CHAINS)], [unit_count(c) for c in range(N_CHAINS)], filter_count, bits, beam, stats)
    return out + (stats,)


MAX_CASE_CHAINS = 9


@functools.lru_cache(maxsize=None)
def _layout_chains(filter_count, bits, beam, odd):
    """the statement for chains 0 .. 8 of the encoder corpus as its layouts cut them: `odd` has sample limits of its own, the other
    layouts give every chain its full span.  A chain's records do not depend on the case's chain count: computed once, shared"""
    chains = K.layout("odd" if odd else "pairs", MAX_CASE_CHAINS)[0]
    xs = np.zeros((MAX_CASE_CHAINS, 28 * K.MAX_UNITS), np.int16)
    for c in range(MAX_CASE_CHAINS):
        v = K.valid_samples(chains[c])
        xs[c, :v] = K.content(c, 28 * K.MAX_UNITS)[:v]
    start = [K.start_state(c) for c in range(MAX_CASE_CHAINS)]
    return B.encode_chains_np(xs, start, chains["n_units"].astype(np.int64), filter_count, bits, beam)[:3]


@functools.lru_cache(maxsize=None)
def case(filter_count, bits, beam, name, n_chains):
    """the encoder corpus's case (its tables, sample buffer and start states) with the statement's image: records with the canary where
    nothing is written, the end states, the errors (canary words where nothing is written)"""
    assert n_chains <= MAX_CASE_CHAINS
    k = K.Case.__new__(K.Case)
    k.filter_count, k.bits, k.layout, k.n_chains = filter_count, bits, name, n_chains
    k.chains, k.unit_base, k.samples, k.n_records = K.layout(name, n_chains)
    k.start = np.array([K.start_state(c) for c in range(n_chains)], np.int32).reshape(n_chains, 2)
    n = k.chains["n_units"].astype(np.int64)
    rec, err, after = _layout_chains(filter_count, bits, beam, name == "odd")
    k.image = np.full((k.n_records + K.TAIL_RECORDS, K.record_bytes(bits)), K.CANARY, np.uint8)
    k.err = np.full(k.n_records + K.TAIL_RECORDS, K.CANARY * 0x01010101, np.uint32)
    k.final = k.start.copy()
    for c in range(n_chains):
        idx = int(k.unit_base[c]) + int(k.chains["unit_stride"][c]) * np.arange(n[c])
        k.image[idx], k.err[idx] = rec[c, :n[c]], err[c, :n[c]]
        if n[c]:
            k.final[c] = after[c, n[c] - 1]
    return k


def oracle_unit(x, state, filter_count, bits):
    """-> (record, state after, squared error) of the reference's encoder for one unit"""
    L = K._bind()
    st = O.Chan(int(state[0]), int(state[1]))
    codes = (C.c_uint8 * 28)()
    xx = np.ascontiguousarray(x, np.int16)
    h = int(L.orc_adpcm_encode_unit(C.byref(st), O.ptr(xx, O.i16p), 28, 1, filter_count, K.shift_range(bits), codes))
    rec = K.pack_record(h, np.frombuffer(codes, np.uint8).copy(), bits)
    dec, _, _, _ = R.decode_unit(rec, bits, filter_count, int(state[0]), int(state[1]))
    return rec, (st.prev1, st.prev2), int(((np.asarray(dec, np.int64) - xx.astype(np.int64)) ** 2).sum())
