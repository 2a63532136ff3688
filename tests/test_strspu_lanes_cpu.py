"""The STRSPU audio sector kernel file's own text (psxavenc_amd/csrc/strspu_kernels.hip) on the CPU, lane by lane, under the host
sanitizers (tests/cpu/strspu_lanes.cpp behind the stand-in tests/cpu/hip_lanes/hip/hip_runtime.h), against the format's restatement
(tests/strspu_ref.py) byte for byte.  The kernel loads a 16-byte record in every lane and selects afterwards: the two header lanes
and the leading dummy block drop what they loaded, so which record they load shows in no output byte.  Here the units are a heap
block that ends with the last record include/psxav_hip.h promises the call reads, and a load outside is a report.  Mono and stereo,
with and without the leading dummy, loop and no loop, 1, 2 and 3 sectors, dense and scattered destinations, one stream and two with
padded strides; every lane order -- ascending, descending, shuffled -- must give the same bytes."""
import numpy as np
import pytest

import lanes_cpu as L
import strspu_ref as R

FILL = 0xC3
OPTION_SETS = [0, R.LOOP, R.NO_LEADING_DUMMY, R.LOOP | R.NO_LEADING_DUMMY]


def _case(rng, ch, K, options, S, scattered):
    """one call: random records, every stream's units and output further apart than a stream when there are two"""
    opt = options | (0x0001 if not options else 0x1200 + K)
    records = rng.integers(0, 256, (S, K * 126, 16), dtype=np.uint8)
    ustride = K * 126 * 16 + (48 if S > 1 else 0)
    units = rng.integers(0, 256, (S, ustride), dtype=np.uint8)
    units[:, :K * 126 * 16] = records.reshape(S, -1)
    n_slots = 2 * K + 1 if scattered else K
    slots = (rng.permutation(n_slots)[:K] if scattered else np.arange(K)).astype(np.int32)
    ostride = n_slots * 2048 + (2048 + 12 if S > 1 else 0)
    return dict(ch=ch, K=K, freq=44100 + 7 * K, opt=opt, S=S, records=records, units=units, ustride=ustride, scattered=scattered, slots=slots,
                n_slots=n_slots, ostride=ostride)


def _write(path, cases):
    with open(path, "wb") as f:
        for c in cases:
            f.write(np.array([c["K"], c["ch"], c["freq"], c["opt"], c["S"], c["ustride"], int(c["scattered"]), c["n_slots"], c["ostride"], 4, FILL],
                             np.int32).tobytes())
            if c["scattered"]:
                f.write(c["slots"].tobytes())
            f.write(c["units"].tobytes())


def _destination_bytes(c):
    return (c["S"] - 1) * c["ostride"] + c["n_slots"] * 2048


def _want(c):
    want = np.full(_destination_bytes(c), FILL, np.uint8)
    for i in range(c["S"]):
        sectors = R.audio_sectors(R.records_to_lanes(c["records"][i], c["K"], c["ch"]), c["K"], c["ch"], c["freq"], c["opt"])
        for k in range(c["K"]):
            at = i * c["ostride"] + int(c["slots"][k]) * 2048
            want[at:at + 2048] = sectors[k]
    return want


@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    d = tmp_path_factory.mktemp("strspu_lanes")
    exe = L.build(d, "strspu_lanes", L.SANITIZE)

    def check(cases):
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        _write(src, cases)
        raw, at = np.frombuffer(L.run_orders(exe, src, dst), np.uint8), 0
        for c in cases:
            size = _destination_bytes(c)
            bad = np.nonzero(raw[at:at + size] != _want(c))[0]
            assert not bad.size, ((c["ch"], c["K"], hex(c["opt"]), c["S"], c["scattered"]), "bytes differ at %s" % bad[:8].tolist())
            at += size
        assert at == raw.size
    return check


@pytest.mark.parametrize("ch,K", [(ch, K) for ch in (1, 2) for K in (1, 2, 3)])
def test_audio_sector_kernel_on_random_records(lanes, ch, K):
    rng = np.random.default_rng(1000 * ch + K)
    lanes([_case(rng, ch, K, options, S, scattered) for options in OPTION_SETS for S in (1, 2) for scattered in (False, True)])


def test_the_units_block_ends_with_the_last_unit_the_header_promises():
    """what the program allocates, restated: with the leading dummy a channel has one unit less than its blocks, so the stream's last
    `channels` records are behind the units and not part of the block"""
    for ch in (1, 2):
        for K in (1, 3):
            assert R.units_per_channel(K, ch, 0) * ch == K * 126 - ch and R.units_per_channel(K, ch, R.NO_LEADING_DUMMY) * ch == K * 126
