"""The STRSPU reader's kernel file (psxavenc_amd/csrc/strspu_demux_kernels.hip) and the host layer that builds its jobs and lays its
workspace out (psxhip_strspu_demux_device in psxhip_str_demux.cpp), their own text, on the CPU under the host sanitizers:
tests/cpu/strspu_demux_lanes.cpp behind the stand-in's wavefront model (tests/cpu/hip_lanes/hip_lanes_waves.h), against "psxhip STRSPU
demux v1" (tests/strspu_demux_ref.py) byte for byte, on the cases of tests/strspu_demux_cases.py.

The chunk number comes from the stream's bytes and addresses the owner and count words, the chunk records and the unit records;
the de-interleave kernel reads 16 bytes at once or four dwords by what the host layer says of the source's alignment.  A read or
write outside any of them is a sanitizer report here: the sectors and every output are heap blocks that end where
include/psxav_hip.h lets the call reach, the sectors 0, 4, 8 or 12 bytes behind a 16-byte boundary.  Three orders of workgroups,
wavefronts and lanes must give equal bytes.  The last test reads gcov: every line of the kernel file ran, both instantiations of
the de-interleave kernel included."""
import numpy as np
import pytest

import lanes_cpu as L
import str_readers_lanes as S
import strspu_demux_cases as X
import strspu_demux_ref as R

KERNEL_FILE = "strspu_demux_kernels.hip"
NOT_REACHED = {}
DAMAGE = ("removed", "duplicated", "reordered", "number-0", "number-max") + tuple(X.MISMATCH_EDITS)


def _settings(ns, **over):
    fields = dict(vars(ns))
    fields.pop("format")
    fields.update(over)
    return S.settings(8, **fields)


def crossing_records():
    """every channel count x rate x CD speed, all option sets and both audio positions, and the ends of the format: room for one chunk
    more than the stream has"""
    out = []
    for case in X.CROSSING + X.EDGES:
        ns, frames, pcm, sectors, rows, K, budgets = X.stream(case)
        out.append(S.record(_settings(ns), [sectors], 1, frames.shape[0], int(budgets.max()), K + 1))
    return out


def shape_records():
    """no sectors; both load paths of the de-interleave (the source 0, 4, 8, 12 bytes behind a 16-byte boundary, stream strides that
    are and are not multiples of 16, one to three streams); room below the chunks and no room; no table"""
    out = [S.record(_settings(X.settings(2, 44100, 2)), [np.zeros((0, 2048), np.uint8)], -1, 2, 2016, 2)]
    streams = [X.stream(X.CROSSING[i])[3] for i in (7, 11, 7)]
    ns = X.stream(X.CROSSING[7])[0]
    for in_offset, in_pad, n in ((0, 2048, 1), (4, 2048, 1), (8, 2048, 1), (12, 2048, 1), (0, 2048, 2), (0, 2048 + 4, 2), (0, 2048 + 8, 2),
                                 (4, 2048 + 12, 2), (0, 4096, 3)):
        out.append(S.record(_settings(ns), streams[:n], 1, 5, 10 * 2016, 10, in_offset=in_offset, in_pad=in_pad, bs_pad=4 * (n - 1), out_pad=16 * (n - 1)))
    ns, frames, pcm, sectors, rows, K, budgets = X.stream(X.CROSSING[6])
    for cap, table in ((K - 2, True), (0, True), (K, False)):
        out.append(S.record(_settings(ns), [sectors], 1, frames.shape[0], int(budgets.max()), cap, table=table))
    return out


def damage_records():
    """every damage of tests/strspu_demux_cases.py; random sectors with the ids at random, 64 and -- across the scan block of 256 --
    300 of them, chunk numbers that meet the capacity from both sides"""
    ns, frames, pcm, sectors, rows, K, budgets = X.stream(X.CROSSING[6])
    out = [S.record(_settings(ns), [X.damaged(name, sectors, rows, np.random.default_rng(5))], 1, frames.shape[0], int(budgets.max()), K)
           for name in DAMAGE]
    for seed in (1, 2):
        s = _settings(X.settings(1 + seed % 2, 44100, 2, options=X.OPTION_SETS[seed], audio_id=0x0002, video_id=0x8001, width=0, height=0))
        sectors = X.random_sectors(seed, 64, 0x0002, 0x8001)
        out.append(S.record(s, [sectors], 2, 6, 3 * 2016 + 8, 8))
        out.append(S.record(s, [sectors, sectors[::-1]], -1, 12, 2016, 13, in_pad=2048 + 4))
        out.append(S.record(s, [X.random_sectors(seed + 10, 300, 0x0002, 0x8001)], -1, 12, 2 * 2016, 5 + 4 * seed))
    return out


@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    d = tmp_path_factory.mktemp("strspu_demux_lanes")
    return d, L.build(d, "strspu_demux_lanes", L.SANITIZE)


def test_the_crossing_and_the_ends_of_the_format(lanes):
    results = S.check(L, *lanes, crossing_records())
    for case, r in zip(X.CROSSING + X.EDGES, results):
        K = X.stream(case)[5]
        assert r[0]["audio_summary"].tolist() == [K, K, K - 1 if K else -1, 0] and not r[0]["info"][:, 7].any(), case


def test_load_paths_strides_and_capacities(lanes):
    results = S.check(L, *lanes, shape_records())
    assert results[1][0]["audio_summary"].tolist() == [9, 9, 8, 0]
    assert results[5][1]["chunk_info"][:, 1].tolist() == [R.MISMATCH] * 3 + [R.MISSING] * 7


def test_damage_and_random_sectors(lanes):
    results = S.check(L, *lanes, damage_records())
    reached = 0
    for r in results:
        reached |= int(np.bitwise_or.reduce(r[0]["chunk_info"][:, 1]))
    assert reached & R.MISMATCH and reached & R.DUPLICATE and reached & R.MISSING
    assert any(r[0]["summary"][7] > 0 for r in results), "chunk numbers at and past the capacity were dropped"


def test_the_records_reach_every_line(tmp_path):
    exe = L.build(tmp_path, "strspu_demux_lanes", L.COVERAGE)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    S.write(src, crossing_records() + shape_records() + damage_records())
    L.run(exe, src, dst, sanitized=False)
    cov = L.Coverage(tmp_path, "strspu_demux_lanes", KERNEL_FILE)
    seen = cov.instantiations("spu_deinterleave_kernel")
    print("instantiations of spu_deinterleave_kernel:", seen)
    assert len(seen) == 2 and all(c > 0 for c in seen.values()), seen
    unvisited = cov.unvisited()
    print("lines that hold code and did not run:", unvisited)
    assert not [x for x in unvisited if x[1] not in NOT_REACHED], [x for x in unvisited if x[1] not in NOT_REACHED]
    assert len(cov.lines) > 80
