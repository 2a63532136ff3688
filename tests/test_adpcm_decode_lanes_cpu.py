"""The ADPCM decoder's kernel file (psxavenc_amd/csrc/adpcm_decode_kernels.hip) and its host layer (psxhip_adpcm_decode.cpp: the
argument rules, the chunk tables, the workspace and the verify passes of the chunked decode), their own text, on the CPU under the
host sanitizers: tests/cpu/adpcm_decode_lanes.cpp behind the stand-in's wavefront model (tests/cpu/hip_lanes/hip_lanes_waves.h),
against "psxhip ADPCM decode v1" (tests/adpcm_decode_ref.py) and plain numpy sums, byte for byte.

The decode kernel stages every lane's records in LDS through the whole wavefront, decodes behind a barrier and writes every work
item's samples with the whole wavefront behind another; the write-out walks a ballot with readlane.  What the GPU tests cannot see:
a record or sample read outside its buffer (the blocks here end with the last element the call may touch and start behind the
promised alignment and no more), a barrier or cross-lane read not every lane reaches, LDS traffic that relies on lockstep (three
orders of workgroups, wavefronts and lanes must give equal bytes), shifts by the records' nibbles and other undefined behaviour.
Records hold every header byte, so every shift and filter nibble.  The last test reads gcov: every line of the kernel file and
all four instantiations of the decode kernel ran."""
import numpy as np
import pytest

import adpcm_decode_ref as R
import lanes_cpu as L

FILL = 0x6B
CANARY = np.frombuffer(bytes([FILL, FILL]), np.int16)[0]
KERNEL_FILE = "adpcm_decode_kernels.hip"
NOT_REACHED = {}
CODINGS = [(4, 4), (5, 4), (4, 8)]
MAX_CHAINS, MAX_UNITS = 67, 23
_pool = {}


def pool(filter_count, bits):
    """chains of records of random bytes (every header value), their start states, and the statement's decode"""
    key = (filter_count, bits)
    if key not in _pool:
        rec = R.random_records(100 + bits + filter_count, bits, MAX_CHAINS * MAX_UNITS).reshape(MAX_CHAINS, MAX_UNITS, -1)
        states = np.random.default_rng(5).integers(-32768, 32768, (MAX_CHAINS, 2)).astype(np.int32)
        states[0] = 0
        pcm = np.zeros((MAX_CHAINS, 28 * MAX_UNITS), np.int16)
        flags = np.zeros((MAX_CHAINS, MAX_UNITS), np.uint8)
        for c in range(MAX_CHAINS):
            pcm[c], _, flags[c] = R.decode_chain(rec[c], bits, filter_count, states[c])
        _pool[key] = (rec, states, pcm, flags)
    return _pool[key]


def layout(n_chains, n_units, pitch, shift=0, cut=True):
    """chains in groups of `pitch` whose samples and records interleave; groups 6 samples apart, the first `shift` samples in (an odd
    shift puts the pairs' samples on dword boundaries of the program's buffer, which starts 2 bytes behind one).  The last unit of
    every third chain is cut by sample_limit at 28 u + 5."""
    c = np.arange(n_chains)
    span, groups = 28 * n_units, -(-n_chains // pitch)
    off = (c // pitch) * (pitch * span + 6) + c % pitch + shift
    limit = np.full(n_chains, span, np.int64)
    if n_units and cut:
        limit[c % 3 == 1] = 28 * (n_units - 1) + 5
    chains = [dict(sample_offset=int(off[k]), pitch=pitch, sample_limit=int(limit[k]), n_units=n_units, unit_stride=pitch) for k in range(n_chains)]
    base = ((c // pitch) * pitch * n_units + c % pitch).astype(np.int32)
    return chains, base, groups * (pitch * span + 6) + 8 + shift, groups * pitch * n_units


def _chain_bytes(chains):
    return b"".join(np.array([k["sample_offset"]], np.int64).tobytes() +
                    np.array([k["pitch"], k["sample_limit"], k["n_units"], k["unit_stride"]], np.int32).tobytes() for k in chains)


def _head(kind, bits, fc, chains, n_records, total, a=0, tail=0, chunk=0, warm=0, passes=0, sums=0):
    return np.array([kind, bits, fc, len(chains), n_records, total, a, tail, chunk, warm, passes, FILL, sums, 0, 0, 0], np.int32).tobytes()


def decode_record(kind, fc, bits, chains, base, total, n_records, flags=True, tail=True, chunk=0, warm=0, passes=0, rec=None, states=None, pcm=None, uflags=None):
    """one decode call and the statement's bytes for it"""
    if rec is None:
        rec, states, pcm, uflags = pool(fc, bits)
    nc = len(chains)
    units = np.zeros((max(n_records, 0), rec.shape[2]), np.uint8)
    want = np.full(total, CANARY, np.int16)
    want_flags = np.full(n_records, FILL, np.uint8)
    want_tail = np.full((nc, 28), CANARY, np.int16)
    want_states = np.zeros((nc, 2), np.int32)
    for c, k in enumerate(chains):
        n, at = k["n_units"], base[c] + k["unit_stride"] * np.arange(k["n_units"])
        units[at] = rec[c, :n]
        lim = min(k["sample_limit"], 28 * n)
        want[k["sample_offset"] + k["pitch"] * np.arange(lim)] = pcm[c, :lim]
        want_flags[at] = uflags[c, :n]
        if k["sample_limit"] % 28 and k["sample_limit"] // 28 < n:
            u = k["sample_limit"] // 28
            want_tail[c] = pcm[c, 28 * u:28 * u + 28]
        want_states[c] = states[c] if n == 0 else (pcm[c, 28 * n - 1], pcm[c, 28 * n - 2])
    src = _head(kind, bits, fc, chains, n_records, total, int(flags), int(tail), chunk, warm, passes) + _chain_bytes(chains) + base.tobytes() + \
        np.ascontiguousarray(states[:nc]).tobytes() + units.tobytes()
    parts = [("samples", want.tobytes()), ("states", want_states.tobytes())]
    if flags:
        parts.append(("flags", want_flags.tobytes()))
    if tail:
        parts.append(("tail", want_tail.tobytes()))
    if kind == 1:
        parts.append(("passes", None))
    return src, parts


def sse_record(pitch, n_chains, n_units, shift, with_tail, with_unit=True, with_sums=True, seed=9):
    chains, base, total, n_records = layout(n_chains, n_units, pitch, shift)
    rng = np.random.default_rng(seed)
    a = rng.integers(-32768, 32768, total).astype(np.int16)
    b = rng.integers(-32768, 32768, total).astype(np.int16)
    for c, (x, y) in ((0, (32767, -32768)), (2, (-32768, 32767))):           # the extremes: a unit's sum passes 2^32
        if c < n_chains:
            idx = chains[c]["sample_offset"] + pitch * np.arange(chains[c]["sample_limit"])
            a[idx], b[idx] = x, y
    tail = rng.integers(-32768, 32768, (n_chains, 28)).astype(np.int16)
    unit, sums = np.frombuffer(bytes([FILL]) * 8 * n_records, np.uint64).copy(), np.zeros((n_chains, 2), np.uint64)
    for c, k in enumerate(chains):
        lim = k["sample_limit"]
        idx = k["sample_offset"] + pitch * np.arange(lim)
        aa, bb = np.zeros(28 * n_units, np.int64), np.zeros(28 * n_units, np.int64)
        aa[:lim], bb[:lim] = a[idx], b[idx]
        if with_tail and lim % 28:
            u = lim // 28
            aa[lim:28 * u + 28] = tail[c, lim - 28 * u:]
        w = ((aa - bb) ** 2).reshape(-1, 28).sum(axis=1).astype(np.uint64)
        unit[base[c] + pitch * np.arange(n_units)] = w
        sums[c] = (int(w.sum()), int((bb ** 2).sum()))
    src = _head(2, 4, 4, chains, n_records, total, int(with_unit), int(with_tail), sums=int(with_sums)) + _chain_bytes(chains) + base.tobytes() + \
        a.tobytes() + b.tobytes() + (tail.tobytes() if with_tail else b"")
    parts = ([("unit_sse", unit.tobytes())] if with_unit else []) + ([("chain_sums", sums.tobytes())] if with_sums else [])
    return src, parts


# ---- the corpus
def serial_records():
    """4- and 8-bit records, four and five filters; pitch 1, 2 and 3; 1, 3 and 65 chains (65 crosses the workgroup of 64 work items);
    1, 4, 5 and 9 units (round the kernel's round of four); even and odd sample offsets -- so that the dword write-out runs and falls
    back, an interleaved pair qualifies for the paired store (odd shift, equal counts) and just fails to (even shift; one of the
    pair cut by sample_limit) --; sample_limit cutting a unit with and without the tail buffer"""
    out = []
    for fc, bits in CODINGS:
        for pitch in (1, 2, 3):
            for nc in (1, 3, 65):
                for n_units in (1, 4, 5, 9):
                    if nc == 65 and n_units in (4, 5) and bits == 8:
                        continue
                    for shift in (0, 1):
                        chains, base, total, n_records = layout(nc, n_units, pitch, shift, cut=not (nc == 3 and n_units == 4))
                        out.append(decode_record(0, fc, bits, chains, base, total, n_records, flags=shift == 0, tail=(shift + n_units) % 2 == 0))
        # the pool's first 256 records hold every header byte: twelve whole chains of it
        chains, base, total, n_records = layout(12, MAX_UNITS, 1, 1)
        out.append(decode_record(0, fc, bits, chains, base, total, n_records))
    return out


def chunked_records():
    """the chunked decode: chunks of 1, 4 and 64 units (the last: one chunk per chain, whose verify pass changes nothing), warm-ups of
    0 and 2, a stereo pair with one channel cut, a lone pitch-2 chain; the fixed-point stream, whose guesses from silence are all wrong"""
    out = []
    for fc, bits in CODINGS:
        for chunk, warm in ((1, 0), (4, 2), (64, 2)):
            chains, base, total, n_records = layout(3, MAX_UNITS, 1, 1)
            out.append(decode_record(1, fc, bits, chains, base, total, n_records, chunk=chunk, warm=warm))
            chains, base, total, n_records = layout(5, MAX_UNITS, 2, 1)
            out.append(decode_record(1, fc, bits, chains, base, total, n_records, flags=False, tail=False, chunk=chunk, warm=warm))
    for start in (1000, -1000):
        n_units = 64
        rec = R.fixed_point_stream(n_units)[None]
        states = np.array([[start, start]], np.int32)
        pcm, st, fl = R.decode_chain(rec[0], 4, 5, (start, start))
        chains = [dict(sample_offset=1, pitch=1, sample_limit=28 * n_units, n_units=n_units, unit_stride=1)]
        out.append(decode_record(1, 5, 4, chains, np.zeros(1, np.int32), 28 * n_units + 2, n_units, chunk=4, warm=8, rec=rec, states=states,
                                 pcm=pcm[None], uflags=fl[None]))
    return out


def sse_records():
    """the SSE kernel staged through LDS (pitch 1 and 2, even and odd starts) and straight from memory (pitch 3); 65 units cross the
    wavefront's 64; with and without the tail, the per-unit sums and the per-chain sums.  (One or two chains to a call: the host
    layer launches 16384 / n_chains workgroups per chain, up to 1024, whatever the chains' lengths.)"""
    out = []
    for pitch in (1, 2, 3):
        out.append(sse_record(pitch, 2, 9, pitch & 1, with_tail=True))
        out.append(sse_record(pitch, 1, 65, 1 - (pitch & 1), with_tail=False, with_unit=pitch != 2, with_sums=pitch != 3))
    return out


def _check(folder, exe, records):
    src, dst = str(folder / "in.bin"), str(folder / "out.bin")
    with open(src, "wb") as f:
        for s, _ in records:
            f.write(s)
    raw, at, passes = L.run_orders(exe, src, dst, fibers=True), 0, []
    for k, (_, parts) in enumerate(records):
        for name, part in parts:
            if part is None:
                passes.append(int(np.frombuffer(raw[at:at + 4], np.int32)[0]))
                at += 4
                continue
            got = raw[at:at + len(part)]
            if got != part:
                first = next(i for i, (a, b) in enumerate(zip(got, part)) if a != b) if len(got) == len(part) else -1
                raise AssertionError("record %d: %s differs from the statement first at byte %d" % (k, name, first))
            at += len(part)
    assert at == len(raw), (at, len(raw))
    return passes


@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    d = tmp_path_factory.mktemp("adpcm_decode_lanes")
    return d, L.build(d, "adpcm_decode_lanes", L.SANITIZE)


def test_records_decode_byte_for_byte(lanes):
    _check(*lanes, serial_records())
    decoded = {bits: set() for _, bits in CODINGS}
    for src, _ in serial_records():
        head = np.frombuffer(src[:64], np.int32)
        bits, nc, n_records = int(head[1]), int(head[3]), int(head[4])
        units = np.frombuffer(src, np.uint8, n_records * R.record_bytes(bits), 64 + nc * (24 + 4 + 8)).reshape(n_records, -1)
        decoded[bits].update(units[:, 0].tolist())
    for fc, bits in CODINGS:
        assert set(pool(fc, bits)[3].reshape(-1).tolist()) == ({0, 2} if fc == 4 else {0, 1, 2, 3}), "every kind of header was decoded"
        # the records the program was given, not the pool they were drawn from: every shift nibble with every filter nibble
        assert {(b & 15, b >> 4) for b in decoded[bits]} == {(s, f) for s in range(16) for f in range(16)}, bits


def test_chunked_decode_and_its_verify_passes(lanes):
    passes = _check(*lanes, chunked_records())
    per = np.array(passes[:-2]).reshape(len(CODINGS), 3, 2)
    assert (per[:, 2] == 1).all(), "one chunk per chain: the first verify pass changes nothing"
    assert (per[:, 0] >= 2).all(), "chunks of one unit guessed from silence: a verify pass changed something"
    assert min(passes[-2:]) >= 2, "the fixed-point stream needs the verify passes"


def test_sse_kernel_is_exact(lanes):
    _check(*lanes, sse_records())


def test_the_records_reach_every_line_and_instantiation(tmp_path):
    exe = L.build(tmp_path, "adpcm_decode_lanes", L.COVERAGE)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        for s, _ in serial_records()[::3] + chunked_records() + sse_records():
            f.write(s)
    L.run(exe, src, dst, sanitized=False)
    cov = L.Coverage(tmp_path, "adpcm_decode_lanes", KERNEL_FILE)
    seen = cov.instantiations("adpcm_decode_kernel")
    print("instantiations of adpcm_decode_kernel:", seen)
    assert len(seen) == 4 and all(c > 0 for c in seen.values()), seen
    unvisited = cov.unvisited()
    print("lines that hold code and did not run:", unvisited)
    assert not [x for x in unvisited if x[1] not in NOT_REACHED], [x for x in unvisited if x[1] not in NOT_REACHED]
    assert len(cov.lines) > 150
