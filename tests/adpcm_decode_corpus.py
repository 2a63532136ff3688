"""The ADPCM decoder's test material, shared by its CPU and GPU tests: the signals (pure functions of the parameters below), how
they are encoded unit by unit / sector by sector, and the fixture tests/golden/adpcm_decode_ref.npz that holds what the REFERENCE's
encoder reported for them -- (prev1, prev2, mse) after every SPU unit, the channel states after every XA sector
(tests/golden/make_adpcm_decode_golden.py)."""
import os

import numpy as np

import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adpcm_decode_ref.npz")

SPU_UNITS = 100
XA_SECTORS = 2
SEED = 31
KINDS = 6                        # what oracle/synth.c offers
XA_LAYOUTS = [(fmt, stereo, bits) for fmt in (0, 1) for stereo in (0, 1) for bits in (4, 8)]


def signal_names():
    return ["kind%d" % k for k in range(KINDS)] + ["fullscale", "square"]


def signal(name, n, channel=0):
    """n int16 samples of signal `name`: every kind of synth_pcm, full-scale uniform noise and a +-30000 square wave (those two drive
    the clamp and filter 0)"""
    if name.startswith("kind"):
        k = int(name[4:])
        return O.synth_pcm(SEED, k + 8 * channel, 0, n, k)
    if name == "fullscale":
        return np.random.default_rng(1234 + channel).integers(-32768, 32768, n).astype(np.int16)
    assert name == "square"
    return np.where((np.arange(n) // (25 + 6 * channel)) % 2 == 0, 30000, -30000).astype(np.int16)


def xa_samples_per_sector(stereo, bits):
    return ((112 if bits == 8 else 224) >> (1 if stereo else 0)) * 18


def xa_pcm(name, stereo, bits, sectors=XA_SECTORS):
    """interleaved L,R when stereo; whole sectors"""
    n = xa_samples_per_sector(stereo, bits) * sectors
    if not stereo:
        return signal(name, n)
    out = np.zeros(2 * n, np.int16)
    out[0::2] = signal(name, n, 0)
    out[1::2] = signal(name, n, 1)
    return out


def spu_encode_units(pcm, use_ref):
    """unit by unit, the state carried: -> (blocks (n, 16) uint8, per unit (prev1, prev2, mse | -1))"""
    n = len(pcm) // 28
    st = O.RefChan() if use_ref else O.Chan(0, 0)
    blocks = np.zeros((n, 16), np.uint8)
    rep = np.zeros((n, 3), np.int64)
    for u in range(n):
        if use_ref:
            blocks[u], st = O.ref_spu_encode(pcm[28 * u:28 * u + 28], state=st)
            rep[u] = (st.prev1, st.prev2, st.mse)
        else:
            blocks[u], st = O.spu_encode(pcm[28 * u:28 * u + 28], state=st)
            rep[u] = (st.prev1, st.prev2, -1)
    return blocks, rep


def xa_encode_sectors(pcm, fmt, stereo, bits, use_ref, sectors=XA_SECTORS):
    """sector by sector, the state carried: -> (sectors (n, size) uint8, per sector (l1, l2, r1, r2))"""
    s = O.XaSettings(fmt, stereo, 37800, bits, 1, 2)
    sps, ch = xa_samples_per_sector(stereo, bits), 2 if stereo else 1
    size = 2336 if fmt == 0 else 2352
    st = O.RefState() if use_ref else O.State()
    out = np.zeros((sectors, size), np.uint8)
    rep = np.zeros((sectors, 4), np.int32)
    for k in range(sectors):
        part = pcm[k * sps * ch:(k + 1) * sps * ch]
        data, st = (O.ref_xa_encode if use_ref else O.xa_encode)(s, part, sps, lba=k, state=st)
        assert data.size == size
        out[k] = data
        rep[k] = (st.left.prev1, st.left.prev2, st.right.prev1, st.right.prev2)
    return out, rep


def xa_key(name, fmt, stereo, bits):
    return "xa_%s_f%d_s%d_b%d" % (name, fmt, stereo, bits)


_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
        assert _golden["meta"].tolist() == [SEED, SPU_UNITS, XA_SECTORS, KINDS], "the fixture was made for other parameters"
    return _golden
