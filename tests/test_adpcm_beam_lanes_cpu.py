"""The beam encoder's kernel file (psxavenc_amd/csrc/adpcm_beam_kernels.hip) and its host layer (psxhip_adpcm_encode.cpp: the beam
entry points' argument rules, the session with its chunk tables and verify passes), their own text, on the CPU under the host
sanitizers: tests/cpu/adpcm_beam_lanes.cpp -- a program of its own, built with -fsanitize=address,undefined -- behind the
stand-in's wavefront model (tests/cpu/hip_lanes/hip_lanes_waves.h), against "psxhip ADPCM beam v1" (tests/adpcm_beam_ref.py) byte
for byte.

What the GPU tests cannot see: a sample read outside its buffer (the sample block ends with the last sample a chain may read, the
records' and the errors' blocks with the last record index, and each starts behind the promised alignment and no more), a barrier
or a shuffle not every lane reaches, LDS or global traffic that relies on lockstep (three orders of workgroups, wavefronts and
lanes must give equal bytes), shifts of negative numbers and other undefined behaviour in the step."""
import numpy as np
import pytest

import adpcm_beam_corpus as BC
import adpcm_encode_corpus as K
import lanes_cpu as L

FILL = K.CANARY
SERIAL = [(4, "odd", 5), (4, "pairs", 5), (4, "quads", 9), (4, "scattered", 5), (1, "odd", 4), (2, "pairs", 3), (3, "scattered", 1)]
CHUNKED = [(2, "odd", 5, 4, 2), (4, "pairs", 3, 7, 0), (4, "odd", 1, 4, 0)]


def record(kind, filter_count, bits, beam, name, n_chains, has_err=False, chunk=0, warm=0):
    k = BC.case(filter_count, bits, beam, name, n_chains)
    last = [int(k.chains["sample_offset"][c]) + int(k.chains["pitch"][c]) * (K.valid_samples(k.chains[c]) - 1) + 1
            for c in range(n_chains) if K.valid_samples(k.chains[c])]
    total = max(last) if last else 0
    head = np.array([kind, bits, filter_count, n_chains, k.n_records, total, beam, int(has_err), chunk, warm, 0, FILL, 0, 0, 0, 0], np.int32)
    src = head.tobytes() + k.chains.tobytes() + k.unit_base.tobytes() + k.start.tobytes() + k.samples[:total].tobytes()
    want = k.image[:k.n_records].tobytes() + k.final.tobytes() + (k.err[:k.n_records].tobytes() if has_err else b"")
    return src, want


def _check(folder, exe, records):
    src, dst = str(folder / "in.bin"), str(folder / "out.bin")
    with open(src, "wb") as f:
        for s, _ in records:
            f.write(s)
    raw, at = L.run_orders(exe, src, dst, fibers=True), 0
    for i, (_, want) in enumerate(records):
        got = raw[at:at + len(want)]
        if got != want:
            first = next(j for j, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else -1
            raise AssertionError("record %d differs from the statement first at byte %d of its output" % (i, first))
        at += len(want)
    assert at == len(raw), (at, len(raw))


@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    assert K.CHAIN_DTYPE.itemsize == 24
    d = tmp_path_factory.mktemp("adpcm_beam_lanes")
    return d, L.build(d, "adpcm_beam_lanes", L.SANITIZE)


@pytest.mark.parametrize("filter_count,bits", BC.CODINGS)
def test_serial_kernel_byte_for_byte(lanes, filter_count, bits):
    _check(*lanes, [record(0, filter_count, bits, beam, name, n, has_err=i % 2 == 0) for i, (beam, name, n) in enumerate(SERIAL)])


@pytest.mark.parametrize("filter_count,bits", BC.CODINGS)
def test_chunked_call_and_session_reach_the_serial_result(lanes, filter_count, bits):
    """speculate and verify instantiations; the session started from wrong states, refused a change of width, run again from the
    right ones"""
    recs = [record(1, filter_count, bits, beam, name, n, chunk=chunk, warm=warm) for beam, name, n, chunk, warm in CHUNKED]
    recs.append(record(2, filter_count, bits, 3, "odd", 5, chunk=5, warm=1))
    _check(*lanes, recs)
