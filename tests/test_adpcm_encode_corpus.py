"""The encoder's chain corpus (tests/adpcm_encode_corpus.py) on the CPU: its expected bytes equal the reference's own code wherever the
reference can express the case -- live when oracle/_ref is there, and always through the recorded tests/golden/adpcm_chain_corpus_ref.npz
-- its tables and poison are what they claim, and its content reaches the places where the kernels have code of their own.  The other
geometries rest on orc_adpcm_encode_unit, which tests/test_adpcm_oracle.py holds to the reference."""
import importlib.util
import os

import numpy as np
import pytest

import adpcm_encode_corpus as EC
import oracle_lib as O


# ---- against the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.LAYOUTS)
def test_spu_cases_equal_the_reference(name):
    """every SPU chain of every case, at its pitch, offset, limit and start state, through psx_audio_spu_encode"""
    for n_chains in EC.CHAIN_COUNTS:
        blocks, final = EC.spu_ours(name, n_chains)
        assert np.array_equal(EC.digest(blocks, final), EC.golden()[EC.spu_key(name, n_chains)]), (name, n_chains)
        if O.ref() is not None:
            want, want_final = EC.spu_reference(name, n_chains)
            assert np.array_equal(blocks, want) and np.array_equal(final, want_final), (name, n_chains)


@pytest.mark.parametrize("fmt,stereo,bits", EC.XA_LAYOUTS)
def test_xa_streams_equal_the_reference(fmt, stereo, bits):
    """whole sectors of a stereo pair (the `pairs` shape) or a mono chain through psx_audio_xa_encode: the sound groups packed from the
    expected records, and the end states"""
    _, chains, base, rec, final = EC.xa_stream(stereo, bits)
    groups = EC.sound_groups(rec, bits)
    assert np.array_equal(EC.digest(groups, final), EC.golden()[EC.xa_key(fmt, stereo, bits)])
    for use_ref in ([False, True] if O.ref() is not None else [False]):
        sectors, want_final = EC.xa_sectors(fmt, stereo, bits, use_ref)
        assert np.array_equal(EC.xa_group_bytes(sectors, fmt), groups) and np.array_equal(final, want_final), use_ref
    ch = 2 if stereo else 1
    assert chains["pitch"].tolist() == chains["unit_stride"].tolist() == [ch] * ch and base.tolist() == list(range(ch))


def test_the_fixture_regenerates_from_the_reference_build():
    golden_dir = os.path.dirname(EC.GOLDEN)
    assert os.path.getsize(EC.GOLDEN) <= os.path.getsize(os.path.join(golden_dir, "adpcm_decode_ref.npz"))
    if O.ref() is None:
        return
    spec = importlib.util.spec_from_file_location("make_adpcm_chain_corpus_golden",
                                                  os.path.join(golden_dir, "make_adpcm_chain_corpus_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    fresh, kept = G.build(), EC.golden()
    assert sorted(fresh) == sorted(kept)
    for k in fresh:
        assert np.array_equal(fresh[k], kept[k]), k


# ---- the tables ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.LAYOUTS)
def test_layouts_are_what_they_claim(name):
    for n_chains in EC.CHAIN_COUNTS:
        k = EC.case(4, 8, name, n_chains)
        ch = k.chains
        assert len(ch) == n_chains and ch["n_units"].tolist() == [EC.unit_count(c) for c in range(n_chains)]
        # everything a chain may read lies inside the buffer, nothing is read by two chains, and the rest is poison
        reader = np.full(k.samples.size, -1, np.int32)
        for c in range(n_chains):
            span = int(ch["sample_offset"][c]) + int(ch["pitch"][c]) * np.arange(28 * int(ch["n_units"][c]))
            assert span.size == 0 or span.max() < k.samples.size - 32
            idx = span[:EC.valid_samples(ch[c])]
            assert (reader[idx] == -1).all()
            reader[idx] = c
            assert np.array_equal(k.samples[idx], EC.content(c, 28 * EC.MAX_UNITS)[:idx.size])
            assert (reader[span[idx.size:]] == -1).all()                           # behind the limit: nobody's
        free = np.nonzero(reader == -1)[0]
        assert np.array_equal(k.samples[free], np.where(free % 2 == 0, EC.POISON[0], EC.POISON[1]))
        # records: inside, owned once (the constructor asserts it), canary elsewhere and behind
        nobody = k.owner == -1
        assert (k.image[nobody] == EC.CANARY).all() and nobody[k.n_records:].all() and nobody[k.n_records:].size == EC.TAIL_RECORDS
        assert (~nobody).sum() == int(ch["n_units"].sum())
        assert np.array_equal(k.final[ch["n_units"] == 0], k.start[ch["n_units"] == 0])
        if name == "odd":
            assert (ch["pitch"] == 1).all() and ch["sample_offset"][0] == 1
            if n_chains >= 65:
                assert set((ch["sample_offset"] % 8).tolist()) == set(range(8))
                lim, span = ch["sample_limit"], 28 * ch["n_units"]
                assert ((lim > span) & (span > 0)).any() and ((lim == 0) & (span > 0)).any() and (lim == span - 23).any() and (lim == span - 27).any()
        elif name == "pairs":
            assert (ch["pitch"] == 2).all() and (ch["unit_stride"] == 2).all()
        elif name == "quads":
            assert np.array_equal(ch["pitch"], ch["unit_stride"]) and set(ch["pitch"].tolist()) == ({3, 4} if n_chains > 3 else {3})
        else:
            assert (ch["unit_stride"] == 3).all() and (np.diff(k.unit_base[ch["n_units"] > 0]) < 0).all()
            assert nobody[:k.n_records].sum() == 2 * (~nobody).sum()
    # unit counts are mixed inside every group of four chains and of five
    n = [EC.unit_count(c) for c in range(EC.MAX_CHAINS)]
    assert all(len(set(n[i:i + 4])) == 4 for i in range(0, 128, 4)) and set(n) == {0, 1, 2, 7, 33}


def test_start_states_cover_the_int16_range():
    s = {EC.start_state(c) for c in range(EC.MAX_CHAINS)}
    assert {(0, 0), (1, -1), (-1, 1), (32767, 32767), (-32768, -32768), (32767, -32768), (-32768, 32767)} <= s
    assert all(-32768 <= v <= 32767 for p in s for v in p) and len(s) > 20


def test_eight_bit_records_keep_bytes_1_to_3_zero():
    """pinned in include/psxav_hip.h"""
    k = EC.case(4, 8, "pairs", 11)
    assert (k.image[k.owner >= 0][:, 1:4] == 0).all()
    assert (EC.case(4, 4, "pairs", 11).image[k.owner >= 0][:, 1] == 0).all()


# ---- coverage: computed from the oracle alone (orc_adpcm_trial gives every candidate's error) ------------------------------------
@pytest.mark.parametrize("filter_count,bits", EC.CODINGS)
def test_the_corpus_reaches_the_kernels_own_code(filter_count, bits):
    r = EC.coverage(filter_count, bits)
    assert set(r[:, 0].tolist()) == set(range(filter_count)), "every filter index wins somewhere"
    assert len(set(r[:, 1].tolist())) >= 8, "at least 8 distinct shifts win"
    assert r[:, 2].any(), "a unit where two candidates tie for the minimum: loop order decides"
    assert r[:, 3].any(), "a unit where some candidate's true error is >= 2^32 (the kernel's saturating sum) and the winner's is not"
    assert r[:, 4].any(), "a unit with a clamped decoded sample"
    assert (r[:, 4] & r[:, 5]).any(), "... that starts from a rail state"
