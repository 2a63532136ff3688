"""The ADPCM decoder on the GPU (include/psxav_hip.h) against the statement tests/adpcm_decode_ref.py -- which
tests/test_adpcm_decode_ref.py pins to the reference's encoder -- and against the encoder's own kernels: records -> PCM byte for byte
in every layout, chunked == serial == statement, the round trip in HBM with the per-unit squared error equal to the reference's mse,
sectors there and back, the squared-error kernel against numpy, the host conveniences.

The decode kernel works in rounds of 4 units per lane (kRound): unit counts one below, at and above it are in every list."""
import numpy as np
import pytest

import adpcm_decode_corpus as DC
import adpcm_decode_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANARY = 0x5A5A
MAX_CHAINS, MAX_UNITS = 130, 100
CODINGS = [(5, 4), (4, 4), (4, 8)]


def dev():
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# ---- the statement's answers, computed once and shared ---------------------------------------------------------------------------
_pool = {}


def pool(filter_count, bits):
    """MAX_CHAINS chains of MAX_UNITS records of random bytes (every header value), their start states, and the statement's decode:
    (records (c, u, bytes), states (c, 2), pcm (c, 28 u), flags (c, u)).  A chain's first n units are a prefix of it."""
    key = (filter_count, bits)
    if key not in _pool:
        rec = R.random_records(100 + bits + filter_count, bits, MAX_CHAINS * MAX_UNITS).reshape(MAX_CHAINS, MAX_UNITS, -1)
        rng = np.random.default_rng(5)
        states = rng.integers(-32768, 32768, (MAX_CHAINS, 2)).astype(np.int32)
        states[0] = 0
        pcm = np.zeros((MAX_CHAINS, 28 * MAX_UNITS), np.int16)
        flags = np.zeros((MAX_CHAINS, MAX_UNITS), np.uint8)
        for c in range(MAX_CHAINS):
            pcm[c], _, flags[c] = R.decode_chain(rec[c], bits, filter_count, states[c])
        _pool[key] = (rec, states, pcm, flags)
    return _pool[key]


def state_after(pcm_row, start, n):
    return (int(start[0]), int(start[1])) if n == 0 else (int(pcm_row[28 * n - 1]), int(pcm_row[28 * n - 2]))


def layout(n_chains, n_units, pitch):
    """chain tables of the two layouts: pitch 1 -- a chain's samples contiguous, chains 3 samples apart (so that their alignment
    varies), records contiguous per chain; pitch 2 -- chains in pairs, samples and records of a pair interleaved both ways.  The last
    unit of every third chain is cut by sample_limit at 28 u + 5."""
    from psxavenc_amd.adpcm import make_chains
    c = np.arange(n_chains)
    span = 28 * n_units
    if pitch == 1:
        off, base, stride = c * (span + 3) + 1, c * n_units, 1
        total = n_chains * (span + 3) + 8
    else:
        off, base, stride = (c // 2) * (2 * span + 6) + (c % 2), (c // 2) * 2 * n_units + (c % 2), 2
        total = ((n_chains + 1) // 2) * (2 * span + 6) + 8
    limit = np.full(n_chains, span, np.int64)
    if n_units:
        limit[c % 3 == 1] = 28 * (n_units - 1) + 5
    n_records = ((n_chains + 1) // 2) * 2 * n_units if pitch == 2 else n_chains * n_units
    return make_chains(off, pitch, limit, n_units, stride), base.astype(np.int32), total, n_records


def scatter_records(rec, chains, base, n_records):
    out = np.zeros((max(n_records, 1), rec.shape[2]), np.uint8)
    for c in range(len(chains)):
        n, s = int(chains["n_units"][c]), int(chains["unit_stride"][c])
        out[base[c] + s * np.arange(n)] = rec[c, :n]
    return out


def expected_samples(pcm, chains, total):
    want = np.full(total, CANARY, np.int16)
    for c in range(len(chains)):
        lim = min(int(chains["sample_limit"][c]), 28 * int(chains["n_units"][c]))
        want[int(chains["sample_offset"][c]) + int(chains["pitch"][c]) * np.arange(lim)] = pcm[c, :lim]
    return want


# ---- 1. records -> PCM -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", [1, 2])
@pytest.mark.parametrize("n_chains", [1, 3, 64, 65, 130])
@pytest.mark.parametrize("filter_count,bits", CODINGS)
def test_records_decode_byte_for_byte(filter_count, bits, n_chains, pitch):
    from psxavenc_amd import decode_chains_device
    rec, states, pcm, flags = pool(filter_count, bits)
    for n_units in (1, 2, 3, 4, 5, 7, 8, 9, 100):
        chains, base, total, n_records = layout(n_chains, n_units, pitch)
        d_units = to_dev(scatter_records(rec, chains, base, n_records))
        d_samples = torch.full((total,), CANARY, dtype=torch.int16, device=dev())
        d_flags = torch.full((n_records,), 0xEE, dtype=torch.uint8, device=dev())
        d_tail = torch.full((n_chains, 28), CANARY, dtype=torch.int16, device=dev())
        d_states = to_dev(states[:n_chains])
        decode_chains_device(d_units, chains, base, filter_count, bits, d_samples, d_states, d_flags, d_tail)
        where = (filter_count, bits, n_chains, pitch, n_units)
        assert np.array_equal(d_samples.cpu().numpy(), expected_samples(pcm, chains, total)), where     # canaries included
        want_states = [state_after(pcm[c], states[c], n_units) for c in range(n_chains)]
        assert d_states.cpu().numpy().tolist() == [list(s) for s in want_states], where
        got_flags, got_tail = d_flags.cpu().numpy(), d_tail.cpu().numpy()
        for c in range(n_chains):
            assert np.array_equal(got_flags[base[c] + int(chains["unit_stride"][c]) * np.arange(n_units)], flags[c, :n_units]), where
            if c % 3 == 1:
                assert np.array_equal(got_tail[c], pcm[c, 28 * (n_units - 1):28 * n_units]), where
            else:
                assert (got_tail[c] == CANARY).all(), where
    assert set(flags.reshape(-1).tolist()) == ({0, 2} if filter_count == 4 else {0, 1, 2, 3})


@pytest.mark.parametrize("pitch", [1, 2])
@pytest.mark.parametrize("filter_count,bits", CODINGS)
def test_two_calls_that_carry_the_states_equal_one(filter_count, bits, pitch):
    from psxavenc_amd import decode_chains_device
    rec, states, pcm, _ = pool(filter_count, bits)
    n_chains, n_units, n1 = 65, 9, 5
    chains, base, total, n_records = layout(n_chains, n_units, pitch)
    d_units = to_dev(scatter_records(rec, chains, base, n_records))
    d_samples = torch.full((total,), CANARY, dtype=torch.int16, device=dev())
    d_states = to_dev(states[:n_chains])
    first, second = chains.copy(), chains.copy()
    first["n_units"] = n1
    first["sample_limit"] = np.minimum(chains["sample_limit"], 28 * n1)
    second["n_units"] = n_units - n1
    second["sample_offset"] = chains["sample_offset"] + 28 * n1 * pitch
    second["sample_limit"] = chains["sample_limit"] - 28 * n1
    decode_chains_device(d_units, first, base, filter_count, bits, d_samples, d_states)
    decode_chains_device(d_units, second, base + n1 * chains["unit_stride"], filter_count, bits, d_samples, d_states)
    assert np.array_equal(d_samples.cpu().numpy(), expected_samples(pcm, chains, total))
    assert d_states.cpu().numpy().tolist() == [list(state_after(pcm[c], states[c], n_units)) for c in range(n_chains)]


# ---- 2. chunked == serial == statement ------------------------------------------------------------------------------------------
_clean = {}


def clean(name):
    """(blocks (100, 16), the statement's pcm from state (123, -45)) of a corpus signal encoded as SPU"""
    if name not in _clean:
        blocks, _ = DC.spu_encode_units(DC.signal(name, 28 * DC.SPU_UNITS), False)
        _clean[name] = (blocks, R.decode_chain(blocks, 4, 5, (123, -45))[0])
    return _clean[name]


@pytest.mark.parametrize("warmup_units", [0, 1, 8])
@pytest.mark.parametrize("chunk_units", [1, 2, 5, 64])
def test_chunked_equals_serial_equals_statement(chunk_units, warmup_units):
    """tonal (kind 4, kind 0) and noise (kind 2) material, 97 units -- no multiple of any chunk length --, one chain cut mid-unit"""
    from psxavenc_amd import decode_chains_chunked, decode_chains_device
    from psxavenc_amd.adpcm import make_chains
    names, n_units = ["kind4", "kind2", "kind0"], 97
    rec = np.stack([clean(n)[0] for n in names])
    pcm = np.stack([clean(n)[1] for n in names])
    span = 28 * n_units
    chains = make_chains(np.arange(3) * (span + 2), 1, [span, 28 * 50 + 5, span], n_units, 1)
    base = (np.arange(3) * n_units).astype(np.int32)
    d_units = to_dev(scatter_records(rec, chains, base, 3 * n_units))
    total = 3 * (span + 2)
    start = np.array([[123, -45]] * 3, np.int32)
    want = expected_samples(pcm, chains, total)
    got = {}
    for how in ("serial", "chunked"):
        d_samples = torch.full((total,), CANARY, dtype=torch.int16, device=dev())
        d_tail = torch.full((3, 28), CANARY, dtype=torch.int16, device=dev())
        d_states = to_dev(start)
        if how == "serial":
            decode_chains_device(d_units, chains, base, 5, 4, d_samples, d_states, None, d_tail)
        else:
            _, passes = decode_chains_chunked(d_units, chains, base, 5, 4, d_samples, d_states, None, d_tail, chunk_units, warmup_units)
        got[how] = (d_samples.cpu().numpy(), d_states.cpu().numpy(), d_tail.cpu().numpy())
        assert np.array_equal(got[how][0], want), how
        assert got[how][1].tolist() == [list(state_after(pcm[c], start[c], n_units)) for c in range(3)], how
        assert np.array_equal(got[how][2][1], pcm[1, 28 * 50:28 * 51]) and (got[how][2][[0, 2]] == CANARY).all(), how
    assert passes >= 1
    if warmup_units == 0 and chunk_units < 97:
        assert passes >= 2, "a guess from silence on tonal material was not met and repaired"


@pytest.mark.parametrize("warmup_units", [0, 8])
@pytest.mark.parametrize("chunk_units", [1, 2, 5, 64])
def test_chunked_stereo_pairs(chunk_units, warmup_units):
    """interleaved output: a stereo pair (its chunks alternate, L and R of a stretch of time are written together), with the right
    channel cut mid-unit; a lone chain with pitch 2; two chains that interleave but differ in length"""
    from psxavenc_amd import decode_chains_chunked
    from psxavenc_amd.adpcm import make_chains
    names, units = ["kind4", "kind2", "kind0", "square", "fullscale"], [97, 97, 97, 97, 50]
    region = 2 * 28 * 97 + 6
    chains = make_chains([0, 1, region, 2 * region, 2 * region + 1], 2, [28 * 97, 28 * 50 + 5, 28 * 97, 28 * 97, 28 * 50], units, 2)
    base = np.array([0, 1, 194, 388, 389], np.int32)
    rec = np.stack([clean(n)[0] for n in names])
    pcm = np.stack([clean(n)[1] for n in names])
    d_units = to_dev(scatter_records(rec, chains, base, 3 * 194))
    total = 3 * region
    start = np.array([[123, -45]] * 5, np.int32)
    d_samples = torch.full((total,), CANARY, dtype=torch.int16, device=dev())
    d_states = to_dev(start)
    _, passes = decode_chains_chunked(d_units, chains, base, 5, 4, d_samples, d_states, chunk_units=chunk_units, warmup_units=warmup_units)
    assert np.array_equal(d_samples.cpu().numpy(), expected_samples(pcm, chains, total))
    assert d_states.cpu().numpy().tolist() == [list(state_after(pcm[c], start[c], units[c])) for c in range(5)]
    assert passes >= (2 if warmup_units == 0 else 1)


def fixed_point_job(start):
    from psxavenc_amd.adpcm import make_chains
    n_units = 64 * 4
    rec = R.fixed_point_stream(n_units)
    chains, base = make_chains([0], 1, 28 * n_units, n_units, 1), np.zeros(1, np.int32)
    pcm, st, _ = R.decode_chain(rec, 4, 5, (start, start))
    return to_dev(rec), chains, base, pcm, st, to_dev(np.array([[start, start]], np.int32))


@pytest.mark.parametrize("start,end", [(1000, 8), (-1000, -7)])
def test_fixed_point_stream_needs_the_verify_passes(start, end):
    """filter 1, shift 12, all codes 0: every guess from silence stays at 0, the truth settles at 8 (-7).  64 chunks of 4 units"""
    from psxavenc_amd import decode_chains_chunked
    d_units, chains, base, pcm, st, d_states = fixed_point_job(start)
    d_samples = torch.full((pcm.size,), CANARY, dtype=torch.int16, device=dev())
    _, passes = decode_chains_chunked(d_units, chains, base, 5, 4, d_samples, d_states, chunk_units=4, warmup_units=8)
    got = d_samples.cpu().numpy()
    assert np.array_equal(got, pcm)
    assert (got[28 * 8:] == end).all() and st == (end, end)
    assert d_states.cpu().numpy().tolist() == [[end, end]]
    assert passes >= 2


def test_exhausted_max_passes_is_an_error_and_leaves_the_states():
    """the documented behaviour (psxav_hip.h): PSXHIP_EINVAL "not converged", d_states as they were"""
    from psxavenc_amd import _lib, decode_chains_chunked
    d_units, chains, base, pcm, st, d_states = fixed_point_job(1000)
    d_samples = torch.full((pcm.size,), CANARY, dtype=torch.int16, device=dev())
    with pytest.raises(_lib.PsxHipError) as e:
        decode_chains_chunked(d_units, chains, base, 5, 4, d_samples, d_states, chunk_units=4, warmup_units=8, max_passes=3)
    assert e.value.code == _lib.PSXHIP_EINVAL and "not converged after 3" in str(e.value)
    assert d_states.cpu().numpy().tolist() == [[1000, 1000]]
    # ... and the same call with room to finish does
    _, passes = decode_chains_chunked(d_units, chains, base, 5, 4, d_samples, d_states, chunk_units=4, warmup_units=8, max_passes=200)
    assert passes > 3 and np.array_equal(d_samples.cpu().numpy(), pcm)


# ---- 3. round trip in HBM --------------------------------------------------------------------------------------------------------
def round_trip_pcm(n_chains, n_units, with_corpus):
    """chain c's input: the corpus signals first (their mse is recorded), synthetic material of every kind behind them"""
    names = DC.signal_names() if with_corpus else []
    rows = []
    for c in range(n_chains):
        if c < len(names):
            rows.append(DC.signal(names[c], 28 * n_units))
        else:
            rows.append(O.synth_pcm(77, c, 0, 28 * n_units, c % DC.KINDS))
    return np.stack(rows)


@pytest.mark.parametrize("n_chains", [1, 65])
@pytest.mark.parametrize("filter_count,bits,pitch", [(5, 4, 1), (4, 4, 1), (4, 8, 1), (4, 4, 2), (4, 8, 2)])
def test_round_trip_in_hbm(oracle, filter_count, bits, pitch, n_chains):
    """encode -> decode with the SAME chain table -> squared errors: the decoder's final states are the encoder's (which are pinned to
    the reference), and for SPU the per-unit sums are the reference's mse -- live when the reference build is there, recorded otherwise"""
    from psxavenc_amd import adpcm_sse, decode_chains_device, snr_db
    from psxavenc_amd.adpcm import encode_chains_device
    n_units = DC.SPU_UNITS
    spu = filter_count == 5
    src = round_trip_pcm(n_chains, n_units, spu)
    chains, base, total, n_records = layout(n_chains, n_units, pitch)
    chains["sample_limit"] = 28 * n_units
    buf = np.zeros(total, np.int16)
    for c in range(n_chains):
        buf[int(chains["sample_offset"][c]) + pitch * np.arange(28 * n_units)] = src[c]
    d_src = to_dev(buf)
    d_units = torch.zeros((n_records, 16 if bits == 4 else 32), dtype=torch.uint8, device=dev())
    d_units, d_enc_states, _ = encode_chains_device(d_src, chains, base, filter_count, bits, d_units=d_units)
    d_out = torch.full((total,), CANARY, dtype=torch.int16, device=dev())
    d_flags = torch.full((n_records,), 0xEE, dtype=torch.uint8, device=dev())
    d_states = decode_chains_device(d_units, chains, base, filter_count, bits, d_out, None, d_flags)
    assert torch.equal(d_states, d_enc_states)
    d_unit, d_sums = adpcm_sse(d_out, d_src, chains, base, n_records=n_records)
    out = d_out.cpu().numpy()
    unit, sums = d_unit.cpu().numpy().astype(np.uint64), d_sums.cpu().numpy().astype(np.uint64)
    for c in range(n_chains):
        idx = int(chains["sample_offset"][c]) + pitch * np.arange(28 * n_units)
        want = R.unit_sse(out[idx], src[c])
        rec_idx = base[c] + int(chains["unit_stride"][c]) * np.arange(n_units)
        assert np.array_equal(unit[rec_idx], want), c
        assert sums[c].tolist() == [int(want.sum()), int((src[c].astype(np.int64) ** 2).sum())], c
        assert (d_flags.cpu().numpy()[rec_idx] == 0).all()
        if spu and c < len(DC.signal_names()):
            name = DC.signal_names()[c]
            assert np.array_equal(unit[rec_idx], DC.golden()["spu_" + name][:, 2].astype(np.uint64)), name
            if oracle.ref() is not None:
                _, rep = DC.spu_encode_units(src[c], True)
                assert np.array_equal(unit[rec_idx], rep[:, 2].astype(np.uint64)), name
    db = snr_db(d_sums.cpu().numpy())
    # coding nothing (filter 0, all codes 0) is among the encoder's candidates and leaves the signal itself as the error: whatever it
    # chose is no worse, unit by unit
    loud = (src.astype(np.int64) ** 2).sum(axis=1) > 0
    assert (db[loud] >= 0.0).all()


# ---- 4. sectors ------------------------------------------------------------------------------------------------------------------
def xa_settings(fmt, stereo, bits):
    from psxavenc_amd.adpcm import XaSettings
    return XaSettings(fmt, bool(stereo), 37800, bits, 1, 2)


@pytest.mark.parametrize("n_sectors", [1, 2, 5])
@pytest.mark.parametrize("fmt,stereo,bits", DC.XA_LAYOUTS)
def test_assemble_then_disassemble_returns_the_records(fmt, stereo, bits, n_sectors):
    from psxavenc_amd import xa_disassemble
    from psxavenc_amd.adpcm import xa_assemble_device
    upg = 8 if bits == 4 else 4
    rec = R.random_records(40 + bits, bits, max(256, n_sectors * 18 * upg))[:n_sectors * 18 * upg].copy()
    rec[:, 1] = 0                          # what the encoder's records hold outside header and codes
    if bits == 8:
        rec[:, 1:4] = 0
    d_rec = to_dev(rec)
    s = xa_settings(fmt, stereo, bits)
    d_eof = to_dev(np.array([0] * (n_sectors - 1) + [1], np.uint8))
    d_sectors = xa_assemble_device(d_rec, n_sectors, s, first_lba=7, d_eof=d_eof)
    d_back, d_status = xa_disassemble(d_sectors, s)
    torch.cuda.synchronize()
    assert torch.equal(d_back, d_rec)
    assert d_status.cpu().tolist() == [0] * n_sectors          # the last sector carries EOF behind its EDC, as the reference leaves it
    # the statement's disassembly says the same
    sectors = d_sectors.cpu().numpy()
    assert np.array_equal(np.concatenate([R.xa_sector_records(x, bits) for x in sectors]), rec)


@pytest.mark.parametrize("fmt,stereo,bits", DC.XA_LAYOUTS)
def test_reference_sectors_decode_to_the_reference_states(oracle, fmt, stereo, bits):
    """the reference build's sectors when it is there, else the same signals encoded by the library: disassemble + decode sector by
    sector, the states carried, gives the recorded states of the reference after every sector"""
    from psxavenc_amd import decode_chains_device, xa_disassemble
    from psxavenc_amd.adpcm import make_chains, xa_encode_streams
    s = xa_settings(fmt, stereo, bits)
    ch = 2 if stereo else 1
    sps = DC.xa_samples_per_sector(stereo, bits)
    units = 18 * (8 if bits == 4 else 4) // ch
    chains = make_chains(np.arange(ch), ch, sps, units, ch)
    base = np.arange(ch).astype(np.int32)
    for name in DC.signal_names():
        want = DC.golden()[DC.xa_key(name, fmt, stereo, bits)]
        pcm = DC.xa_pcm(name, stereo, bits)
        if oracle.ref() is not None:
            sectors, _ = DC.xa_encode_sectors(pcm, fmt, stereo, bits, True)
        else:
            sectors = xa_encode_streams(s, pcm.reshape(1, -1), sps * DC.XA_SECTORS).reshape(DC.XA_SECTORS, -1)
        d_units, d_status = xa_disassemble(to_dev(sectors), s)
        d_states = torch.zeros((ch, 2), dtype=torch.int32, device=dev())
        d_samples = torch.zeros(sps * ch, dtype=torch.int16, device=dev())
        whole = []
        for k in range(DC.XA_SECTORS):
            decode_chains_device(d_units[k * units * ch:], chains, base, 4, bits, d_samples, d_states)
            got = d_states.cpu().numpy().reshape(-1).tolist() + ([] if stereo else [0, 0])
            assert got == want[k].tolist(), (name, k)
            whole.append(d_samples.cpu().numpy().copy())
        assert np.array_equal(np.concatenate(whole), R.decode_xa(sectors, sectors.shape[1], bits, stereo)[0]), name
        assert d_status.cpu().tolist() == [0] * DC.XA_SECTORS, name


@pytest.mark.parametrize("fmt,stereo,bits", DC.XA_LAYOUTS)
def test_sector_status_bits(fmt, stereo, bits):
    """One flipped byte sets its bit.  A sector that carries an EDC carries it over the subheaders and the sound groups: with the EDC
    intact a flipped byte there sets the EDC bit as well (and the coding byte is half of a subheader copy: flipping one copy sets the
    subheader bit too), so "exactly that bit" is asserted on sectors whose EDC is all zero -- which by itself sets nothing -- with the
    coding byte changed in both copies; on sectors with their EDC the flipped byte must set its bit AND the EDC bit."""
    from psxavenc_amd import xa_disassemble
    from psxavenc_amd.adpcm import xa_encode_streams
    s = xa_settings(fmt, stereo, bits)
    ch = 2 if stereo else 1
    sps = DC.xa_samples_per_sector(stereo, bits)
    sector = xa_encode_streams(s, DC.xa_pcm("kind0", stereo, bits, 1).reshape(1, -1), sps)[0]
    o = 16 if fmt else 0
    edc = len(sector) - 4
    assert sector[edc:].any()
    flips = {"clean": ([], 0), "header copy": ([o + 8 + 5], 1), "second header copy": ([o + 8 + 3 * 128 + 13], 1), "subheader": ([o + 1], 2),
             "coding": ([o + 3, o + 7], 4), "one coding byte": ([o + 3], 2 | 4), "sound data": ([o + 8 + 700], 0)}
    cases, want = [], []
    for name, (where, bit) in flips.items():
        for zero_edc in (False, True):
            x = sector.copy()
            for w in where:
                x[w] ^= 0x10
            if zero_edc:
                x[edc:] = 0
            cases.append(x)
            want.append(bit | (0 if zero_edc or not where else 8))
    x = sector.copy()
    x[edc + 2] ^= 0x01
    cases.append(x)
    want.append(8)
    d_units, d_status = xa_disassemble(to_dev(np.stack(cases)), s)
    assert d_status.cpu().tolist() == want
    # a sector with status bits set is disassembled all the same
    got = d_units.cpu().numpy().reshape(len(cases), -1)
    for x, g in zip(cases, got):
        assert np.array_equal(g, R.xa_sector_records(x, bits).reshape(-1))
    assert ch in (1, 2)


# ---- 5. the squared-error kernel against numpy -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", [1, 2])
def test_sse_kernel_is_exact(pitch):
    from psxavenc_amd import adpcm_sse
    n_chains, n_units = 65, 9
    chains, base, total, n_records = layout(n_chains, n_units, pitch)          # every third chain is cut mid-unit
    rng = np.random.default_rng(9)
    a = rng.integers(-32768, 32768, total).astype(np.int16)
    b = rng.integers(-32768, 32768, total).astype(np.int16)
    # the extremes over whole units: +32767 against -32768 passes 2^32 per unit
    for c, (x, y) in ((0, (32767, -32768)), (2, (-32768, 32767))):
        idx = int(chains["sample_offset"][c]) + pitch * np.arange(28 * n_units)
        a[idx], b[idx] = x, y
    tail = rng.integers(-32768, 32768, (n_chains, 28)).astype(np.int16)
    for with_tail in (True, False):
        d_unit, d_sums = adpcm_sse(to_dev(a), to_dev(b), chains, base, d_a_tail=to_dev(tail) if with_tail else None, n_records=n_records)
        unit, sums = d_unit.cpu().numpy().astype(np.uint64), d_sums.cpu().numpy().astype(np.uint64)
        for c in range(n_chains):
            lim = int(chains["sample_limit"][c])
            idx = int(chains["sample_offset"][c]) + pitch * np.arange(lim)
            aa, bb = np.zeros(28 * n_units, np.int64), np.zeros(28 * n_units, np.int64)
            aa[:lim], bb[:lim] = a[idx], b[idx]
            if with_tail and lim % 28:
                u = lim // 28
                aa[lim:28 * u + 28] = tail[c, lim - 28 * u:]
            want = ((aa - bb) ** 2).reshape(-1, 28).sum(axis=1).astype(np.uint64)
            assert np.array_equal(unit[base[c] + int(chains["unit_stride"][c]) * np.arange(n_units)], want), (c, with_tail)
            assert sums[c].tolist() == [int(want.sum()), int((bb ** 2).sum())], (c, with_tail)
        assert int(unit[base[0]]) == 28 * 65535 ** 2 > 2 ** 32
    _, only_sums = adpcm_sse(to_dev(a), to_dev(b), chains)
    assert only_sums.cpu().numpy().astype(np.uint64)[:, 1].tolist() == sums[:, 1].tolist()


# ---- 6. host conveniences --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_streams", [1, 3])
def test_spu_decode_streams(n_streams):
    from psxavenc_amd import spu_decode_streams
    names = ["kind0", "kind2", "square"][:n_streams]
    blocks = np.stack([clean(n)[0] for n in names]).reshape(n_streams, -1)
    want = [R.decode_chain(blocks[i], 4, 5, (7 * i, -3)) for i in range(n_streams)]
    start = np.array([[7 * i, -3] for i in range(n_streams)], np.int32)
    st = start.copy()
    got = spu_decode_streams(blocks, st)
    assert np.array_equal(got, np.stack([w[0] for w in want])) and st.tolist() == [list(w[1]) for w in want]
    st = start.copy()
    cut = 16 * 37
    two = np.concatenate([spu_decode_streams(blocks[:, :cut], st), spu_decode_streams(blocks[:, cut:], st)], axis=1)
    assert np.array_equal(two, got) and st.tolist() == [list(w[1]) for w in want]


@pytest.mark.parametrize("n_streams", [1, 3])
@pytest.mark.parametrize("fmt,stereo,bits", [(0, 0, 4), (1, 1, 4), (0, 1, 8), (1, 0, 8)])
def test_xa_decode_streams(fmt, stereo, bits, n_streams):
    from psxavenc_amd import xa_decode_streams
    from psxavenc_amd.adpcm import xa_encode_streams
    s = xa_settings(fmt, stereo, bits)
    ch = 2 if stereo else 1
    sps = DC.xa_samples_per_sector(stereo, bits)
    names = ["kind0", "fullscale", "kind5"][:n_streams]
    pcm = np.stack([DC.xa_pcm(n, stereo, bits, 3) for n in names])
    sectors = xa_encode_streams(s, pcm, 3 * sps)
    ssz = sectors.shape[1] // 3
    st = np.zeros((n_streams, 2, 2), np.int32)
    got, status = xa_decode_streams(s, sectors, st)
    assert status.tolist() == [[0, 0, 0]] * n_streams
    for i in range(n_streams):
        want, wst = R.decode_xa(sectors[i], ssz, bits, stereo)
        assert np.array_equal(got[i], want), i
        assert st[i, :ch].tolist() == [list(x) for x in wst], i
    st2 = np.zeros((n_streams, 2, 2), np.int32)
    a, _ = xa_decode_streams(s, sectors[:, :ssz], st2)
    b, _ = xa_decode_streams(s, sectors[:, ssz:], st2)
    assert np.array_equal(np.concatenate([a, b], axis=1), got) and np.array_equal(st2, st)
