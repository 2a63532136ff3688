"""The statement "psxhip ADPCM decode v1" (tests/adpcm_decode_ref.py) against the reference's encoder, which contains the decoder:
libpsxav/adpcm.c:120-124 reconstructs every sample, :135-136 carries the last two as the chain's state, and because qerr is never
updated (:131-132) state->mse after a call is the winning unit's sum of squared errors.  So every unit the reference encodes gives
three numbers a decoder plus a squared-error sum must reproduce.  They are recorded in tests/golden/adpcm_decode_ref.npz; with the
reference build present (oracle/_ref) the live values are compared with the recording as well, and the reference's own bytes are
what is decoded -- without it the bytes come from this repository's restatement of the encoder (oracle/), the numbers from the
recording.  Never skips."""
import numpy as np
import pytest

import adpcm_decode_corpus as DC
import adpcm_decode_ref as R


@pytest.mark.parametrize("name", DC.signal_names())
def test_spu_units_decode_to_the_reference_state_and_mse(oracle, name):
    want = DC.golden()["spu_" + name]
    pcm = DC.signal(name, 28 * DC.SPU_UNITS)
    live = oracle.ref() is not None
    blocks, rep = DC.spu_encode_units(pcm, live)
    if live:
        assert np.array_equal(rep, want), "the reference build disagrees with the recording"
    assert np.array_equal(rep[:, :2], want[:, :2])
    p1 = p2 = 0
    for u in range(DC.SPU_UNITS):
        out, p1, p2, flags = R.decode_unit(blocks[u], 4, 5, p1, p2)
        sse = int(R.unit_sse(out, pcm[28 * u:28 * u + 28])[0])
        assert (p1, p2, sse) == tuple(int(v) for v in want[u]), (name, u)
        assert flags == 0
    if name in ("fullscale", "square"):
        assert (blocks[:, 0] >> 4 == 0).any(), "filter 0 is not reached"
    if name == "fullscale":
        assert int(want[:, 2].max()) > 0


@pytest.mark.parametrize("fmt,stereo,bits", DC.XA_LAYOUTS)
def test_xa_sectors_decode_to_the_reference_states(oracle, fmt, stereo, bits):
    live = oracle.ref() is not None
    for name in DC.signal_names():
        want = DC.golden()[DC.xa_key(name, fmt, stereo, bits)]
        sectors, rep = DC.xa_encode_sectors(DC.xa_pcm(name, stereo, bits), fmt, stereo, bits, live)
        assert np.array_equal(rep, want), (name, "the encoder disagrees with the recording")
        st = [(0, 0), (0, 0)][:2 if stereo else 1]
        for k in range(DC.XA_SECTORS):
            pcm, st = R.decode_xa(sectors[k], sectors.shape[1], bits, stereo, st)
            got = [st[0][0], st[0][1]] + ([st[1][0], st[1][1]] if stereo else [0, 0])
            assert got == want[k].tolist(), (name, k)
            assert pcm.size == DC.xa_samples_per_sector(stereo, bits) * (2 if stereo else 1)


def test_the_clamp_is_driven():
    """the encoder keeps what it writes inside the rails (its search minimises the error), so clean material never decodes to one;
    the records of random bytes that the core and the kernels are held to (R.random_records) do reach both, for both code sizes"""
    for bits, filter_count in ((4, 5), (8, 4)):
        pcm, _, _ = R.decode_chain(R.random_records(7 + bits, bits, 300), bits, filter_count)
        assert pcm.max() == 32767 and pcm.min() == -32768


def test_fixed_points_of_filter_one():
    """filter 1, shift 12, all codes 0: 0, 8 and -7 all stay where they are -- a chain entered at (1000, 1000) settles at 8, one
    entered at silence stays at 0, one entered at (-1000, -1000) settles at -7"""
    rec = R.fixed_point_stream(256)
    for start, end in (((0, 0), 0), ((1000, 1000), 8), ((-1000, -1000), -7)):
        pcm, st, _ = R.decode_chain(rec, 4, 5, start)
        assert st == (end, end) and (pcm[28 * 8:] == end).all(), (start, st)
