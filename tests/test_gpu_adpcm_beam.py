"""The beam encoder ("psxhip ADPCM beam v1") on the device, against its statement (tests/adpcm_beam_ref.py)
byte for byte: the serial call on the encoder corpus's layouts with canaries wherever no chain may write, the chunked call and the
session against the serial call, the host-buffer batches against blocks and sectors the existing packers make of the statement's
records, the device decoder as an independent witness of the reported error and of the per-unit guarantee, and what the entry points
refuse.  The guarantee is per unit from the same state; no test compares whole chains' errors or two beam widths' errors."""
import ctypes as C

import numpy as np
import pytest

import adpcm_beam_corpus as BC
import adpcm_beam_ref as B
import adpcm_decode_ref as R
import adpcm_encode_corpus as K
import oracle_lib as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHAIN_COUNTS = (1, 3, 4, 5, 9)          # below, at and above one workgroup's four rows


def dev():
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def lib():
    from psxavenc_amd import adpcm
    L = adpcm._bind()
    vp, i32 = C.c_void_p, C.c_int
    L.psxhip_adpcm_session_create.argtypes = [C.POINTER(vp), i32, vp, vp, vp, vp, i32, i32, i32, vp, i32, i32, vp]
    return L


# ---- 1. the serial call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", BC.BEAMS)
@pytest.mark.parametrize("filter_count,bits", BC.CODINGS)
def test_serial_call_equals_the_statement(filter_count, bits, beam):
    """the corpus's four layouts, chain counts round one workgroup's rows, unit counts 0, 1, 2, 7 and 33 mixed inside every wavefront,
    sample_limit cutting inside the last unit (`odd`): the WHOLE record buffer, the end states and the error words"""
    from psxavenc_amd import adpcm
    for name in K.LAYOUTS:
        for n_chains in CHAIN_COUNTS:
            k = BC.case(filter_count, bits, beam, name, n_chains)
            d_samples, d_states = to_dev(k.samples), to_dev(k.start)
            d_units = torch.full(k.image.shape, K.CANARY, dtype=torch.uint8, device=dev())
            d_err = torch.full(k.err.shape, K.CANARY * 0x01010101 - (1 << 32), dtype=torch.int32, device=dev())
            adpcm.encode_chains_device(d_samples, k.chains, k.unit_base, filter_count, bits, d_states=d_states, d_units=d_units, beam=beam,
                                       d_unit_err=d_err)
            what = (name, n_chains)
            assert np.array_equal(d_units.cpu().numpy(), k.image), what              # canaries included
            assert np.array_equal(d_states.cpu().numpy(), k.final), what
            assert np.array_equal(d_err.cpu().numpy().view(np.uint32), k.err), what
            assert np.array_equal(d_samples.cpu().numpy(), k.samples), what
            if beam == 1:                                                            # ... and the plain encoder's bytes
                d_plain, d_pstates = torch.full_like(d_units, K.CANARY), to_dev(k.start)
                adpcm.encode_chains_device(d_samples, k.chains, k.unit_base, filter_count, bits, d_states=d_pstates, d_units=d_plain)
                assert torch.equal(d_plain, d_units) and torch.equal(d_pstates, d_states), what


# ---- 2. chunked call and sessions ------------------------------------------------------------------------------------------------
def long_chains():
    """three planar chains of 40 units: tonal (never falls into a guessed state), white noise, silence then a loud square"""
    n = 28 * 40
    i = np.arange(n)
    square = (np.where((i // 9) % 2 == 0, 30000, -30000) * (i >= 28 * 13)).astype(np.int16)
    pcm = np.concatenate([O.synth_pcm(K.SEED, 0, 0, n, 4), O.synth_pcm(K.SEED, 1, 0, n, 2), square])
    chains = K.table(n * np.arange(3), 1, n, 40, 1)
    return pcm, chains, (40 * np.arange(3)).astype(np.int32), np.array([[1000, -1000], [0, 0], [-7, 32767]], np.int32)


@pytest.mark.parametrize("beam", (2, 4))
@pytest.mark.parametrize("filter_count,bits", BC.CODINGS)
def test_chunked_call_and_session_equal_the_serial_call(filter_count, bits, beam):
    from psxavenc_amd import _lib, adpcm
    pcm, chains, base, start = long_chains()
    d_samples = to_dev(pcm)
    shape = (120 + K.TAIL_RECORDS, K.record_bytes(bits))
    d_want, d_wstates = torch.full(shape, K.CANARY, dtype=torch.uint8, device=dev()), to_dev(start)
    adpcm.encode_chains_device(d_samples, chains, base, filter_count, bits, d_states=d_wstates, d_units=d_want, beam=beam)
    want, want_states = d_want.cpu().numpy(), d_wstates.cpu().numpy()
    rec, _, after, _ = B.encode_chains_np(pcm.reshape(3, -1), start, [40] * 3, filter_count, bits, beam)
    assert np.array_equal(want[:120], rec.reshape(120, -1)) and np.array_equal(want_states, after[:, -1]), "the serial call against the statement"
    for chunk_units in (4, 7):
        for warmup_units in (0, 2):
            d_units, d_states = torch.full(shape, K.CANARY, dtype=torch.uint8, device=dev()), to_dev(start)
            _, _, passes = adpcm.encode_chains_device(d_samples, chains, base, filter_count, bits, d_states=d_states, d_units=d_units,
                                                      chunk_units=chunk_units, warmup_units=warmup_units, beam=beam)
            assert passes >= 1
            assert np.array_equal(d_units.cpu().numpy(), want) and np.array_equal(d_states.cpu().numpy(), want_states), (chunk_units, warmup_units)
    # a session: first from wrong start states, then corrected; the width cannot change in between
    d_units = torch.full(shape, K.CANARY, dtype=torch.uint8, device=dev())
    s = adpcm.AdpcmSession(d_samples, chains, base, filter_count, bits, d_units=d_units, chunk_units=7, warmup_units=2, beam=beam)
    try:
        s.run(start[::-1].copy())
        with pytest.raises(_lib.PsxHipError):
            s.set_beam(beam)
        final, _ = s.run(start)
        assert s.passes >= 2
        assert np.array_equal(d_units.cpu().numpy(), want) and np.array_equal(final, want_states)
        s.reset()
        s.set_beam(0)                                                            # after a reset: the plain encoder again
        final, _ = s.run(start)
        d_plain, d_pstates = torch.full(shape, K.CANARY, dtype=torch.uint8, device=dev()), to_dev(start)
        adpcm.encode_chains_device(d_samples, chains, base, filter_count, bits, d_states=d_pstates, d_units=d_plain)
        assert torch.equal(d_units, d_plain) and np.array_equal(final, d_pstates.cpu().numpy())
    finally:
        s.close()


# ---- 3. the host-buffer batches ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", BC.BEAMS)
def test_spu_streams_equal_the_statements_blocks(beam):
    from psxavenc_amd import adpcm
    n = 28 * 5 - 9                                                               # the fifth unit is cut
    pcm = np.stack([BC.content(c, 28 * K.MAX_UNITS)[:n] for c in (0, 6, BC.N_CORPUS + 1)])
    start = np.array([[0, 0], [32767, -32768], [-5, 9]], np.int32)
    xs = np.zeros((3, 28 * 5), np.int16)
    xs[:, :n] = pcm
    rec, _, after, _ = B.encode_chains_np(xs, start, [5] * 3, 5, 4, beam)
    want = adpcm.spu_pack_device(to_dev(rec.reshape(15, 16)), 15).cpu().numpy().reshape(3, 80)
    states = start.copy()
    got = adpcm.spu_encode_streams(pcm, states=states, beam=beam)
    assert np.array_equal(got, want) and np.array_equal(states, after[:, -1])


@pytest.mark.parametrize("bits", (4, 8))
def test_xa_streams_equal_the_statements_sectors(bits):
    from psxavenc_amd import adpcm
    beam, sectors = 4, 2
    per = 18 * (8 if bits == 4 else 4) // 2 * sectors                            # units per channel
    pcm = np.zeros(28 * per * 2, np.int16)
    pcm[0::2], pcm[1::2] = BC.content(0, 28 * per), BC.content(BC.N_CORPUS + 1, 28 * per)
    start = np.array([[100, -100], [-32768, 32767]], np.int32)
    rec, _, after, _ = B.encode_chains_np(np.stack([pcm[0::2], pcm[1::2]]), start, [per] * 2, 4, bits, beam)
    order = np.zeros((per * 2, K.record_bytes(bits)), np.uint8)
    order[0::2], order[1::2] = rec[0], rec[1]
    s = adpcm.XaSettings(adpcm.PSX_AUDIO_XA_FORMAT_XACD, True, 37800, bits, 1, 2)
    want = adpcm.xa_assemble_device(to_dev(order), sectors, s, first_lba=75).cpu().numpy().reshape(1, -1)
    states = start.reshape(1, 2, 2).copy()
    got = adpcm.xa_encode_streams(s, pcm.reshape(1, -1), 28 * per, lbas=[75], states=states, beam=beam)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(states[0], after[:, -1])


# ---- 4. the decoder as a witness ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_count,bits", BC.CODINGS)
def test_decoder_confirms_the_error_and_the_per_unit_guarantee(filter_count, bits):
    """records of the device's beam encode through psxhip_adpcm_decode_chains_device: the squared error of every unit against the
    input is the reported one, and at most the reference encoder's for that unit from the decoded state in front of it"""
    from psxavenc_amd import adpcm, adpcm_decode
    k = BC.case(filter_count, bits, 4, "pairs", 5)
    d_samples, d_states = to_dev(k.samples), to_dev(k.start)
    d_units = torch.full(k.image.shape, K.CANARY, dtype=torch.uint8, device=dev())
    d_err = torch.zeros(k.err.shape, dtype=torch.int32, device=dev())
    adpcm.encode_chains_device(d_samples, k.chains, k.unit_base, filter_count, bits, d_states=d_states, d_units=d_units, beam=4, d_unit_err=d_err)
    d_pcm = torch.zeros(k.samples.shape, dtype=torch.int16, device=dev())
    d_end = adpcm_decode.decode_chains_device(d_units, k.chains, k.unit_base, filter_count, bits, d_pcm, d_states=to_dev(k.start))
    assert torch.equal(d_end, d_states), "the decoder ends where the encoder says it did"
    pcm, err = d_pcm.cpu().numpy().astype(np.int64), d_err.cpu().numpy().view(np.uint32)
    units = 0
    for c in range(k.n_chains):
        n, off, pitch = int(k.chains["n_units"][c]), int(k.chains["sample_offset"][c]), int(k.chains["pitch"][c])
        x = k.samples[off + pitch * np.arange(28 * n)].astype(np.int64)
        y = pcm[off + pitch * np.arange(28 * n)]
        before = tuple(int(v) for v in k.start[c])
        for u in range(n):
            xu, yu = x[28 * u:28 * u + 28], y[28 * u:28 * u + 28]
            e = int(((yu - xu) ** 2).sum())
            at = int(k.unit_base[c]) + u * int(k.chains["unit_stride"][c])
            assert e == int(err[at]), (c, u)
            assert e <= BC.oracle_unit(xu.astype(np.int16), before, filter_count, bits)[2], (c, u)
            before = (int(yu[27]), int(yu[26]))
            units += 1
    assert units > 40


# ---- 5. refusals, and the stream ---------------------------------------------------------------------------------------------------
def test_refusals_and_symbols():
    from psxavenc_amd import _lib
    L = lib()
    k = BC.case(5, 4, 2, "odd", 3)
    d_samples, d_states = to_dev(k.samples), to_dev(k.start)
    d_units = torch.full(k.image.shape, K.CANARY, dtype=torch.uint8, device=dev())
    d_chains, d_base = to_dev(k.chains.view(np.uint8)), to_dev(k.unit_base)
    torch.cuda.synchronize()
    S, CH, BA, ST, U = d_samples.data_ptr(), d_chains.data_ptr(), d_base.data_ptr(), d_states.data_ptr(), d_units.data_ptr()

    def serial(beam=2, s=S, ch=CH, ba=BA, st=ST, u=U, bits=4, err=None):
        return L.psxhip_adpcm_beam_encode_chains_device(0, s, ch, ba, 3, 5, bits, beam, st, u, err, None)

    def chunked(beam=2, u=U, st=ST, chunk_units=4):
        return L.psxhip_adpcm_beam_encode_chains_chunked(0, S, k.chains.ctypes.data, k.unit_base.ctypes.data, 3, 5, 4, st, u, beam, chunk_units, 2, 0, None)

    pcm, st, out = np.zeros(56, np.int16), np.zeros((2, 2), np.int32), np.zeros(64, np.uint8)
    refused = [serial(beam=0), serial(beam=5), chunked(beam=0), chunked(beam=5),                       # the width
               serial(u=U + 4), chunked(u=U + 4), serial(u=U + 2, bits=8), serial(err=U + 2),          # alignment
               serial(s=None), serial(ch=None), serial(ba=None), serial(st=None), serial(u=None), chunked(u=None), chunked(st=None),
               chunked(chunk_units=0),
               L.psxhip_spu_encode_streams_host_beam(0, pcm.ctypes.data, 1, 56, 1, 56, st.ctypes.data, out.ctypes.data, 64, 0),
               L.psxhip_spu_encode_streams_host_beam(0, pcm.ctypes.data, 1, 56, 1, 56, st.ctypes.data, out.ctypes.data, 64, 5),
               L.psxhip_spu_encode_streams_host_beam(0, None, 1, 56, 1, 56, st.ctypes.data, out.ctypes.data, 64, 2),
               L.psxhip_xa_encode_streams_host_beam(0, 0, 1, 37800, 4, 0, 0, pcm.ctypes.data, 1, 56, 28, None, st.ctypes.data, out.ctypes.data, 64, 0, 0),
               L.psxhip_xa_encode_streams_host_beam(0, 0, 1, 37800, 4, 0, 0, pcm.ctypes.data, 1, 56, 28, None, None, out.ctypes.data, 64, 0, 2),
               L.psxhip_adpcm_session_set_beam(None, 2)]
    assert refused == [_lib.PSXHIP_EINVAL] * len(refused), refused
    h = C.c_void_p()
    assert L.psxhip_adpcm_session_create(C.byref(h), 0, S, k.chains.ctypes.data, k.unit_base.ctypes.data, None, 3, 5, 4, U, 4, 2, None) == 0
    L.psxhip_adpcm_session_destroy.argtypes, L.psxhip_adpcm_session_destroy.restype = [C.c_void_p], None
    assert [L.psxhip_adpcm_session_set_beam(h, b) for b in (-1, 5, 4, 0)] == [_lib.PSXHIP_EINVAL, _lib.PSXHIP_EINVAL, 0, 0]
    L.psxhip_adpcm_session_destroy(h)
    torch.cuda.synchronize()
    assert (d_units.cpu().numpy() == K.CANARY).all() and np.array_equal(d_states.cpu().numpy(), k.start) and (out == 0).all()
    L.psxhip_adpcm_beam_kernel_rev.restype = C.c_char_p
    assert L.psxhip_adpcm_beam_kernel_rev() == b"adpcm-beam-k1.0"
    assert serial() == 0                                                         # the same tables, as they should be, are taken
    torch.cuda.synchronize()
    assert np.array_equal(d_units.cpu().numpy(), k.image)


def test_beam_call_is_ordered_on_its_stream():
    """One chain on a non-blocking side stream.  Its first 20 000 units go through the plain serial entry point, which is asynchronous
    and writes d_states when its kernel ends (some tens of milliseconds); the other 9 follow at once through the beam call with the
    same d_states on the same stream, nothing synchronised in between.  A beam call that overtook it -- another stream, the null
    stream -- reads the start state (1000, -1000), not the one at the seam: a pure tone never falls into a common state, every
    record behind the seam would differ from the statement's."""
    L = lib()
    n1, n2 = 20000, 9
    pcm = O.synth_pcm(K.SEED, 0, 0, 28 * (n1 + n2), 4)
    _, seam = O.spu_encode(pcm[:28 * n1], state=O.Chan(1000, -1000))
    rec, _, after, _ = B.encode_chains_np(pcm[None, 28 * n1:], [(seam.prev1, seam.prev2)], [n2], 5, 4, 3)
    d_samples = to_dev(pcm)
    d_units = torch.full((n1 + n2 + K.TAIL_RECORDS, 16), K.CANARY, dtype=torch.uint8, device=dev())
    d_states = to_dev(np.array([[1000, -1000]], np.int32))
    d_head, d_tail = to_dev(K.table([0], 1, 28 * n1, n1, 1).view(np.uint8)), to_dev(K.table([28 * n1], 1, 28 * n2, n2, 1).view(np.uint8))
    d_head_base, d_tail_base = to_dev(np.zeros(1, np.int32)), to_dev(np.array([n1], np.int32))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(side):
        rc1 = L.psxhip_adpcm_encode_chains_device(0, d_samples.data_ptr(), d_head.data_ptr(), d_head_base.data_ptr(), 1, 5, 4, d_states.data_ptr(),
                                                  d_units.data_ptr(), side.cuda_stream)
        done.record(side)
        still_running = not done.query()
        rc2 = L.psxhip_adpcm_beam_encode_chains_device(0, d_samples.data_ptr(), d_tail.data_ptr(), d_tail_base.data_ptr(), 1, 5, 4, 3, d_states.data_ptr(),
                                                       d_units.data_ptr(), None, side.cuda_stream)
    side.synchronize()
    torch.cuda.synchronize()
    print("the first launch was still running when the beam call was made:", still_running)
    assert rc1 == 0 and rc2 == 0
    got = d_units.cpu().numpy()
    assert np.array_equal(got[n1:n1 + n2], rec[0]) and (got[n1 + n2:] == K.CANARY).all()
    assert d_states.cpu().numpy().tolist() == [after[0, -1].tolist()]
