"""The sound bank on the GPU ("psxhip SPU bank v1"; include/psxav_hip.h, psxhip_spu_bank_*): the banks of
tests/spu_bank_corpus.py, byte for byte against the reference's files (ref_spu_file of tests/golden/make_spufile_golden.py per
entry, placed by the restated plan) and against what psxhip_spu_file_encode_host writes for every entry on its own; the in-place
chunked path; the beam; the host entry; the check kernel's bits for the corruptions of the CPU test; the decode against
tests/adpcm_decode_ref.py and numpy's integer sums."""
import numpy as np
import pytest
import torch

import adpcm_decode_ref as R
import spu_bank_corpus as B

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 256


def mirror(s, entries, beam=None):
    from psxavenc_amd import spubank
    return (spubank.settings(s["fmt"], s["alignment"], s["no_dummy"], s["bank_alignment"], s["beam"] if beam is None else beam),
            [spubank.entry(e["pcm_offset"], e["samples"], e["freq"], e["loop"], e["enable_loop"], e["name"]) for e in entries])


def make_bank(s, entries, beam=None):
    from psxavenc_amd import SpuBank
    return SpuBank(*mirror(s, entries, beam), device=0)


def host_files(s, entries, pcm):
    """psxhip_spu_file_encode_host per entry, placed by the restated plan"""
    from psxavenc_amd import spufile
    p = B.plan(s, entries)
    bank = np.zeros(p["total"], np.uint8)
    for e, at, size in zip(entries, p["offsets"], p["sizes"]):
        one = spufile.settings(s["fmt"], 1, e["freq"], alignment=s["alignment"], loop_point=e["loop"], enable_loop=e["enable_loop"],
                               no_dummy=s["no_dummy"], name=e["name"])
        f = spufile.encode(one, pcm[e["pcm_offset"]:e["pcm_offset"] + e["samples"]])
        assert f.size == size
        bank[at:at + size] = f
    return bank


def encode_guarded(bank, pcm, stream):
    """one encode_device into a buffer of FILL with guards, on `stream` behind earlier work; the whole buffer as a host array"""
    with torch.cuda.stream(stream):
        busy = torch.ones(1 << 22, device="cuda:0")
        for _ in range(8):
            busy = busy * 1.0001 + 1.0                  # the stream is busy when the library's launches are queued
        d_pcm = torch.from_numpy(pcm).to("cuda:0")
        whole = torch.full((bank.total + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    d_out = whole[GUARD:GUARD + bank.total]
    assert bank.encode_device(d_pcm, d_out, stream=stream) is d_out
    stream.synchronize()
    return whole.cpu().numpy()


def assert_bank(got_whole, want, p, what):
    assert (got_whole[:GUARD] == FILL).all() and (got_whole[GUARD + want.size:] == FILL).all(), "%s: a guard byte was written" % what
    body = got_whole[GUARD:GUARD + want.size]
    if not np.array_equal(body, want):
        first = int(np.flatnonzero(body != want)[0])
        entry = max(i for i, o in enumerate(p["offsets"]) if o <= first)
        raise AssertionError("%s: differs first at byte %d (entry %d, its byte %d)" % (what, first, entry, first - p["offsets"][entry]))


@pytest.fixture(scope="module")
def mixed():
    """the mixed entries, their PCM, and per bank settings (expected bank from the reference's files, restated plan)"""
    entries = B.mixed_entries()
    pcm = B.synth(entries)
    return entries, pcm, [(s,) + B.ref_bank(s, entries, pcm) for s in B.MIXED_SETTINGS]


def test_the_mixed_bank_is_the_reference_files_and_the_one_file_calls(mixed):
    entries, pcm, banks = mixed
    stream = torch.cuda.Stream(device=0)
    other = B.synth(entries, seed=77)
    for k, (s, want, p) in enumerate(banks):
        bank = make_bank(s, entries)
        offsets, sizes, total = bank.layout()
        assert offsets.tolist() == p["offsets"] and sizes.tolist() == p["sizes"] and total == p["total"] == want.size
        first = encode_guarded(bank, pcm, stream)
        assert_bank(first, want, p, "bank %d against the reference's files" % k)
        assert np.array_equal(host_files(s, entries, pcm), want), "psxhip_spu_file_encode_host per entry"
        if k == 1:
            # the context's states are zeroed by every call: other PCM, then the first again
            second = encode_guarded(bank, other, stream)
            assert_bank(second, B.ref_bank(s, entries, other)[0], p, "the second call, other PCM")
            assert not np.array_equal(second, first)
            assert np.array_equal(encode_guarded(bank, pcm, stream), first), "the third call reproduces the first"
        bank.close()


@pytest.mark.parametrize("n,long_samples", [(3, 15000), (12, 115000)])
def test_the_chunked_path_encodes_in_place(n, long_samples):
    """an entry at or past psxhip_adpcm_chunked_threshold(n) units: the chains are cut along time and written where they belong"""
    from psxavenc_amd import _lib
    units = -(-long_samples // 28)
    assert units >= _lib.lib().psxhip_adpcm_chunked_threshold(n) > 300
    entries = B.placed([B.entry(300, 22050, 3, True, "a"), B.entry(long_samples, 44100, B.loop_ms("inside", long_samples, 44100), n == 3, "long")] +
                       [B.entry(100 + 29 * i, 11025, -1, i % 2 == 0, "e%d" % i) for i in range(n - 2)])
    assert len(entries) == n
    pcm = B.synth(entries, seed=5)
    s = B.settings(B.VAG, 64, False, 2048)
    want, p = B.ref_bank(s, entries, pcm)
    bank = make_bank(s, entries)
    got = encode_guarded(bank, pcm, torch.cuda.Stream(device=0))
    assert_bank(got, want, p, "the chunked bank against the reference's files")
    assert np.array_equal(host_files(s, entries, pcm), want)
    bank.close()


def test_the_beam_changes_the_data_blocks_and_nothing_else():
    from psxavenc_amd import adpcm
    entries = B.placed([B.entry(samples, (11025, 22050, 44100)[i % 3], B.loop_ms(("none", "zero", "inside")[i % 3], samples, (11025, 22050, 44100)[i % 3]),
                                i % 2 == 1, "b%d" % i) for i, samples in enumerate((0, 1, 28, 29, 300, 1125, 2000, 57, 640, 999))])
    pcm = B.synth(entries, seed=9)
    s = B.settings(B.VAG, 64, False, 16)
    plain, p = B.ref_bank(s, entries, pcm)
    stream = torch.cuda.Stream(device=0)
    differs = 0
    for beam in (0, 1, 2, 4):
        bank = make_bank(s, entries, beam=beam)
        got = encode_guarded(bank, pcm, stream)
        bank.close()
        if beam < 2:
            assert_bank(got, plain, p, "beam %d is the plain bank" % beam)
            continue
        want = plain.copy()
        for e, base, row in zip(entries, p["unit_base"], p["rows"]):
            if row[3]:
                blocks = adpcm.spu_encode_streams(pcm[e["pcm_offset"]:e["pcm_offset"] + e["samples"]].reshape(1, -1), beam=beam)[0].reshape(-1, 16)
                flags = want[16 * base + 1:16 * (base + row[3]):16].copy()
                want[16 * base:16 * (base + row[3])] = blocks.reshape(-1)
                want[16 * base + 1:16 * (base + row[3]):16] = flags
        assert_bank(got, want, p, "beam %d: psxhip_spu_encode_streams_host_beam's blocks under the same framing" % beam)
        differs += int(not np.array_equal(want, plain))
    assert differs == 2, "the beam's blocks are not the plain encoder's on this material"


def test_encode_host_is_encode_device(mixed):
    entries, pcm, banks = mixed
    for s, want, p in banks[1:3]:
        bank = make_bank(s, entries)
        assert np.array_equal(bank.encode_host(pcm), want)
        assert np.array_equal(bank.encode_host(pcm), want)
        bank.close()


def test_check_device_names_each_corruption(mixed):
    from psxavenc_amd import spubank
    entries, pcm, banks = mixed
    stream = torch.cuda.Stream(device=0)
    kinds = set()
    for s, want, p in banks:
        bank = make_bank(s, entries)
        d_pcm = torch.from_numpy(pcm).to("cuda:0")
        d_bank = bank.encode_device(d_pcm)
        assert bank.check_device(d_bank).cpu().tolist() == [0] * len(entries), "a bank this library wrote is clean"
        for what, i, at, mask, bit in B.corruptions(s, entries, p):
            bad = want.copy()
            bad[at] ^= mask
            with torch.cuda.stream(stream):
                d_bad = torch.from_numpy(bad).to("cuda:0")
            d_status = bank.check_device(d_bad, stream=stream)
            stream.synchronize()                        # (the call is asynchronous on ITS stream)
            status = d_status.cpu().numpy()
            expect = np.zeros(len(entries), np.int32)
            expect[i] = bit
            assert np.array_equal(status, expect), (what, i, status[np.flatnonzero(status != expect)].tolist())
            kinds.add(what)
        bank.close()
    assert len(kinds) == 8
    assert (B.HEADER, B.DUMMY, B.FLAGS, B.TRAP, B.PADDING) == (spubank.STATUS_HEADER, spubank.STATUS_DUMMY, spubank.STATUS_FLAGS, spubank.STATUS_TRAP,
                                                               spubank.STATUS_PADDING)


def test_decode_device_gives_the_statement_s_pcm_and_exact_sums(mixed):
    from psxavenc_amd import SpuBank
    entries, pcm, banks = mixed
    canary = np.int16(0x6B6B)
    for s, want, p in (banks[0], banks[3]):
        bank = make_bank(s, entries)
        d_bank = torch.from_numpy(want).to("cuda:0")
        d_ref = torch.from_numpy(pcm).to("cuda:0")
        d_out = torch.full((pcm.size,), int(canary), dtype=torch.int16, device="cuda:0")
        got, d_sums = bank.decode_device(d_bank, d_out, d_ref)
        assert got is d_out
        torch.cuda.synchronize()
        got, sums = got.cpu().numpy(), d_sums.cpu().numpy().view(np.uint64)
        expect, expect_sums = np.full(pcm.size, canary, np.int16), np.zeros((len(entries), 2), np.uint64)
        for i, (e, base, row) in enumerate(zip(entries, p["unit_base"], p["rows"])):
            if not row[3]:
                continue
            dec, _, _ = R.decode_chain(want[16 * base:16 * (base + row[3])].reshape(-1, 16), 4, 5)
            expect[e["pcm_offset"]:e["pcm_offset"] + e["samples"]] = dec[:e["samples"]]
            ref = np.zeros(28 * row[3], np.int64)
            ref[:e["samples"]] = pcm[e["pcm_offset"]:e["pcm_offset"] + e["samples"]]
            expect_sums[i] = (int(((dec.astype(np.int64) - ref) ** 2).sum()), int((ref ** 2).sum()))
        assert np.array_equal(got, expect), "PCM in the entries' own layout, nothing stored past `samples`"
        assert np.array_equal(sums, expect_sums)
        # without a reference: the PCM alone, into a tensor of the wrapper's
        alone, none = bank.decode_device(d_bank)
        n = bank.pcm_elements
        assert none is None and alone.numel() == n
        assert np.array_equal(alone.cpu().numpy(), np.where(expect[:n] != canary, expect[:n], 0)), "the wrapper's own tensor: zeros where nothing is stored"
        db = SpuBank.snr_db(d_sums)
        some = (expect_sums[:, 0] > 0) & (expect_sums[:, 1] > 0)
        assert db.shape == (len(entries),) and some.sum() > 20
        assert np.allclose(db[some], 10 * np.log10(expect_sums[some, 1].astype(np.float64) / expect_sums[some, 0].astype(np.float64)))
        bank.close()
