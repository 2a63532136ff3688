"""The ADPCM encoder's device interface -- the chain table psxhip_adpcm_chain_t of include/psxav_hip.h -- on every route that must
produce the same bytes from it: the serial kernel, speculate-and-verify in one call, and persistent sessions that share a record
buffer.  The cases are those of tests/adpcm_encode_corpus.py (tests/test_adpcm_encode_corpus.py holds them to the reference): poison
wherever no chain may read, canaries wherever no chain may write, start states over the whole int16 range, unit counts from 0 to 33
mixed inside every wavefront.  The WHOLE record buffer is compared, and every route runs on the current stream and on a side stream.
Then the calls around the encoder: SPU packing and XA sector assembly against canaries, the ordering of the one-call chunked encode
behind asynchronous work on a non-blocking stream, and the arguments the entry points refuse."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import adpcm_encode_corpus as EC
import oracle_lib as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHUNKINGS = [(1, 0), (2, 1), (5, 8), (7, 3), (64, 16)]       # (chunk_units, warmup_units)
SIDE = [pytest.param(False, id="current"), pytest.param(True, id="side")]


def dev():
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def canary_units(k):
    return torch.full(k.image.shape, EC.CANARY, dtype=torch.uint8, device=dev())


@contextlib.contextmanager
def stream(side):
    """the body's calls go to the current stream or to a fresh (non-blocking) side stream; everything has finished on either side"""
    torch.cuda.synchronize()
    if side:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            yield
        s.synchronize()
    else:
        yield
    torch.cuda.synchronize()


def lib():
    from psxavenc_amd import adpcm
    L = adpcm._bind()
    vp, i32 = C.c_void_p, C.c_int
    L.psxhip_adpcm_encode_chains_chunked.argtypes = [i32, vp, vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, vp]
    L.psxhip_adpcm_session_create.argtypes = [C.POINTER(vp), i32, vp, vp, vp, vp, i32, i32, i32, vp, i32, i32, vp]
    return L


def test_the_corpus_speaks_the_librarys_chain_table():
    from psxavenc_amd import adpcm
    assert EC.CHAIN_DTYPE == adpcm.CHAIN_DTYPE and all(EC.record_bytes(b) == adpcm.record_bytes(b) for b in (4, 8))


# ---- 1. the serial route ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDE)
@pytest.mark.parametrize("n_chains", EC.CHAIN_COUNTS)
@pytest.mark.parametrize("name", EC.LAYOUTS)
@pytest.mark.parametrize("filter_count,bits", EC.CODINGS)
def test_serial_route_equals_the_expected_image(filter_count, bits, name, n_chains, side):
    from psxavenc_amd import adpcm
    k = EC.case(filter_count, bits, name, n_chains)
    d_samples, d_units, d_states = to_dev(k.samples), canary_units(k), to_dev(k.start)
    with stream(side):
        adpcm.encode_chains_device(d_samples, k.chains, k.unit_base, filter_count, bits, d_states=d_states, d_units=d_units)
    assert np.array_equal(d_units.cpu().numpy(), k.image)            # canaries included
    assert np.array_equal(d_states.cpu().numpy(), k.final)
    assert np.array_equal(d_samples.cpu().numpy(), k.samples)


# ---- 2. speculate and verify in one call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDE)
@pytest.mark.parametrize("n_chains", EC.CHAIN_COUNTS)
@pytest.mark.parametrize("name", EC.LAYOUTS)
@pytest.mark.parametrize("filter_count,bits", EC.CODINGS)
def test_chunked_route_equals_the_expected_image(filter_count, bits, name, n_chains, side):
    """chunk size 1 puts a seam behind every unit; a warm-up longer than the units in front of a chunk is clipped at the chain's start;
    64 makes every chain a single chunk"""
    from psxavenc_amd import adpcm
    k = EC.case(filter_count, bits, name, n_chains)
    d_samples = to_dev(k.samples)
    for chunk_units, warmup_units in CHUNKINGS:
        d_units, d_states = canary_units(k), to_dev(k.start)
        with stream(side):
            _, _, passes = adpcm.encode_chains_device(d_samples, k.chains, k.unit_base, filter_count, bits, d_states=d_states, d_units=d_units,
                                                      chunk_units=chunk_units, warmup_units=warmup_units)
        where = (chunk_units, warmup_units, passes)
        assert passes >= 1, where
        assert np.array_equal(d_units.cpu().numpy(), k.image), where
        assert np.array_equal(d_states.cpu().numpy(), k.final), where


# ---- 3. two sessions over one record buffer --------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDE)
@pytest.mark.parametrize("n_chains", EC.CHAIN_COUNTS)
@pytest.mark.parametrize("name", ["pairs", "odd"])
@pytest.mark.parametrize("filter_count,bits", EC.CODINGS)
def test_two_sessions_cut_at_every_chains_own_unit(filter_count, bits, name, n_chains, side):
    """every chain is cut behind a unit of its own (0 and n_units among them); the second session does not know its start states
    (lead_units = the cut, start_known = 0) and is driven to the fixpoint the way the ranks of a time-sharded encode are"""
    from psxavenc_amd import adpcm
    from psxavenc_amd.parallel import simulate_time_sharded
    k = EC.case(filter_count, bits, name, n_chains)
    cuts = np.array([(7 * c + 3) % (int(n) + 1) for c, n in enumerate(k.chains["n_units"])], np.int32)
    (a, a_base), (b, b_base) = k.cut(cuts)
    d_samples, d_units = to_dev(k.samples), canary_units(k)
    with stream(side):
        first = adpcm.AdpcmSession(d_samples, a, a_base, filter_count, bits, d_units=d_units, chunk_units=5, warmup_units=3)
        second = adpcm.AdpcmSession(d_samples, b, b_base, filter_count, bits, d_units=d_units, lead_units=cuts, chunk_units=2, warmup_units=4)
        final = simulate_time_sharded([first, second], k.start)
        first.close()
        second.close()
    assert np.array_equal(d_units.cpu().numpy(), k.image)
    assert np.array_equal(final, k.final)


# ---- 4. the one-call chunked encode behind asynchronous work on a non-blocking stream --------------------------------------------
def test_chunked_call_waits_for_the_states_an_earlier_call_on_its_stream_still_writes():
    """One chain on a side stream (PyTorch's are non-blocking: the null stream does not wait for them).  Its first 20 000 units go
    through the serial entry point, which is asynchronous and updates d_states when its kernel ends; the other 97 follow at once through
    the chunked entry point with the same d_states, nothing synchronised in between.  Records and final state are the oracle's encode of
    the whole chain -- a pure tone, which never falls into a guessed state, so a chunked call that read d_states before the first
    kernel had written them gets every record behind the seam wrong.

    Measured on an MI355X: the first launch takes 34.2 ms (stream events, 1.7 us per unit) and is still running when the second call
    begins.  The assertion depends on neither.  The test also passed before d_states moved to the caller's stream: creating the
    session synchronises that stream (psxhip_adpcm_session_create, behind its table uploads), which happened to order the read."""
    L = lib()
    n1, n2 = 20000, 97
    start = (1000, -1000)
    pcm = O.synth_pcm(EC.SEED, 0, 0, 28 * (n1 + n2), 4)
    want, wst = O.spu_encode(pcm, state=O.Chan(*start))
    d_samples = to_dev(pcm)
    d_units = torch.full((n1 + n2 + EC.TAIL_RECORDS, 16), EC.CANARY, dtype=torch.uint8, device=dev())
    d_states = to_dev(np.array([start], np.int32))
    head = EC.table([0], 1, 28 * n1, n1, 1)
    tail = EC.table([28 * n1], 1, 28 * n2, n2, 1)
    d_head, d_head_base = to_dev(head.view(np.uint8)), to_dev(np.zeros(1, np.int32))
    tail_base = np.array([n1], np.int32)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        t0.record(side)
        rc = L.psxhip_adpcm_encode_chains_device(0, d_samples.data_ptr(), d_head.data_ptr(), d_head_base.data_ptr(), 1, 5, 4,
                                                 d_states.data_ptr(), d_units.data_ptr(), side.cuda_stream)
        t1.record(side)
        still_running = not t1.query()
        passes = L.psxhip_adpcm_encode_chains_chunked(0, d_samples.data_ptr(), tail.ctypes.data, tail_base.ctypes.data, 1, 5, 4,
                                                      d_states.data_ptr(), d_units.data_ptr(), 16, 4, 0, side.cuda_stream)
    side.synchronize()
    torch.cuda.synchronize()
    print("first launch: %.3f ms for %d units, still running when the second call began: %s" % (t0.elapsed_time(t1), n1, still_running))
    assert rc == 0 and passes >= 1
    got = d_units.cpu().numpy()
    bad = np.nonzero((got[:n1 + n2] != want.reshape(-1, 16)).any(axis=1))[0]
    assert bad.size == 0, "%d records differ, the first at unit %d (the seam is at %d)" % (bad.size, bad[0], n1)
    assert (got[n1 + n2:] == EC.CANARY).all()
    assert d_states.cpu().numpy().tolist() == [[wst.prev1, wst.prev2]]


# ---- 5. SPU packing and XA sector assembly ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_blocks", [0, 1, 255, 256, 257])
def test_spu_pack_writes_its_blocks_and_nothing_else(n_blocks):
    L = lib()
    rec = np.random.default_rng(n_blocks).integers(0, 256, (257 + 8, 16)).astype(np.uint8)
    d_rec = to_dev(rec)
    d_out = torch.full((n_blocks + EC.TAIL_RECORDS, 16), EC.CANARY, dtype=torch.uint8, device=dev())
    rc = L.psxhip_spu_pack_device(0, d_rec.data_ptr(), n_blocks, d_out.data_ptr(), torch.cuda.current_stream(dev()).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:n_blocks], rec[:n_blocks]) and (got[n_blocks:] == EC.CANARY).all()
    assert np.array_equal(d_rec.cpu().numpy(), rec)


@pytest.mark.parametrize("n_sectors", [1, 2, 5])
@pytest.mark.parametrize("fmt,stereo,bits", EC.XA_LAYOUTS)
def test_xa_assemble_equals_the_oracles_sectors(fmt, stereo, bits, n_sectors):
    """the expected records of whole sectors (a stereo pair in the `pairs` shape, or a mono chain) -> sectors: every byte of the
    oracle's psx_audio_xa_encode for the same samples, start states and LBA, and canary behind the last sector"""
    L = lib()
    _, _, _, rec, _ = EC.xa_stream(stereo, bits)
    want, _ = EC.xa_sectors(fmt, stereo, bits, False, lba=40)
    want = want[:n_sectors]
    ssz = want.shape[1]
    assert ssz == (2352 if fmt else 2336)
    units = n_sectors * 18 * (8 if bits == 4 else 4)
    d_rec = to_dev(rec[:units])
    d_out = torch.full((n_sectors * ssz + 4096,), EC.CANARY, dtype=torch.uint8, device=dev())
    rc = L.psxhip_xa_assemble_device(0, d_rec.data_ptr(), n_sectors, fmt, stereo, 37800, bits, 1, 2, 40, None, d_out.data_ptr(),
                                     torch.cuda.current_stream(dev()).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:n_sectors * ssz].reshape(n_sectors, ssz), want)
    assert (got[n_sectors * ssz:] == EC.CANARY).all()


@pytest.mark.parametrize("stereo,bits", [(0, 4), (1, 4), (0, 8), (1, 8)])
def test_device_encode_of_whole_sectors_gives_the_expected_records(stereo, bits):
    """the stream the sector test assembles, through the serial kernel: its records and end states"""
    from psxavenc_amd import adpcm
    pcm, chains, base, rec, final = EC.xa_stream(stereo, bits)
    d_units = torch.full((len(rec) + EC.TAIL_RECORDS, EC.record_bytes(bits)), EC.CANARY, dtype=torch.uint8, device=dev())
    d_states = to_dev(EC.xa_start(stereo))
    adpcm.encode_chains_device(to_dev(pcm), chains, base, 4, bits, d_states=d_states, d_units=d_units)
    got = d_units.cpu().numpy()
    assert np.array_equal(got[:len(rec)], rec) and (got[len(rec):] == EC.CANARY).all()
    assert np.array_equal(d_states.cpu().numpy(), final)


# ---- 6. what the entry points refuse (no kernel is launched) -----------------------------------------------------------------------
def test_refusals():
    from psxavenc_amd import _lib
    L = lib()
    k = EC.case(5, 4, "odd", 3)
    d_samples, d_units, d_states = to_dev(k.samples), canary_units(k), to_dev(k.start)
    d_chains, d_base = to_dev(k.chains.view(np.uint8)), to_dev(k.unit_base)
    d_out = torch.full((16, 16), EC.CANARY, dtype=torch.uint8, device=dev())
    torch.cuda.synchronize()
    units, odd = d_units.data_ptr(), d_units.data_ptr() + 4           # 4-byte aligned is not enough for 16-byte records
    assert units % 16 == 0

    def serial(p, bits=4):
        return L.psxhip_adpcm_encode_chains_device(0, d_samples.data_ptr(), d_chains.data_ptr(), d_base.data_ptr(), 3, 5, bits,
                                                   d_states.data_ptr(), p, None)

    def create(p, chunk_units, bits=4):
        h = C.c_void_p()
        rc = L.psxhip_adpcm_session_create(C.byref(h), 0, d_samples.data_ptr(), k.chains.ctypes.data, k.unit_base.ctypes.data, None, 3, 5, bits,
                                           p, chunk_units, 4, None)
        assert (rc == 0) == bool(h.value)
        if h.value:
            L.psxhip_adpcm_session_destroy.argtypes = [C.c_void_p]
            L.psxhip_adpcm_session_destroy.restype = None
            L.psxhip_adpcm_session_destroy(h)
        return rc

    def chunked(p, chunk_units):
        return L.psxhip_adpcm_encode_chains_chunked(0, d_samples.data_ptr(), k.chains.ctypes.data, k.unit_base.ctypes.data, 3, 5, 4,
                                                    d_states.data_ptr(), p, chunk_units, 4, 0, None)

    refused = [serial(None), create(None, 4), chunked(None, 4),                      # a null d_units
               create(units, 0), chunked(units, 0),                                  # chunk_units == 0
               serial(odd), create(odd, 4), chunked(odd, 4),                         # 4-bit records off a 16-byte boundary
               L.psxhip_spu_pack_device(0, odd, 1, d_out.data_ptr(), None),
               L.psxhip_spu_pack_device(0, units, 1, d_out.data_ptr() + 4, None),
               serial(units + 2, 8), create(units + 2, 4, 8)]                        # 8-bit records off a 4-byte boundary
    assert refused == [_lib.PSXHIP_EINVAL] * len(refused)
    assert "16-byte" in L.psxhip_last_error().decode() or "bad argument" in L.psxhip_last_error().decode()
    torch.cuda.synchronize()
    assert (d_units.cpu().numpy() == EC.CANARY).all() and (d_out.cpu().numpy() == EC.CANARY).all()
    assert np.array_equal(d_states.cpu().numpy(), k.start)
    # ... and the same tables at an aligned pointer are taken
    assert create(units, 4) == 0
