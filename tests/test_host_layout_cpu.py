"""The host layer's layouts (psxavenc_amd/csrc/host_layout.h) on the CPU, under the host sanitizers: what an XA sector holds, where an
STR sector keeps its headers, the chain tables of planar streams and of interleaved channels, and the workspace offsets.  The driver
(tests/cpu/host_layout_check.cpp) prints what the header derives; every expectation here comes from somewhere else -- the XA format's
own numbers, the geometry tables of psxavenc_amd/strdemux.py and tests/str_demux_ref.py, psxavenc_amd.adpcm.make_chains."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import str_demux_ref
from psxavenc_amd import strdemux
from psxavenc_amd.adpcm import make_chains

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpu/host_layout_check.cpp")
    exe = str(tmp_path_factory.mktemp("host_layout") / "host_layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe,
                    os.path.join(ROOT, "tests/cpu/host_layout_check.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), "the sanitizer build reported:\n" + r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        out.setdefault(kind, []).append(rest)
    return out


def ints(text):
    return [int(v) for v in text.split()]


def test_xa_layout_is_the_formats(lines):
    """A sector is 18 sound groups of 128 bytes: 16 bytes of headers and 112 of codes, 28 codes to a unit; 2336 bytes with the
    subheader in front (XA), 2352 with sync and header too (XACD).  A unit record is an SPU block (2 + 14 bytes) for 4-bit codes and
    4 + 28 bytes for 8-bit ones (include/psxav_hip.h).  The sector interleave is what the playback rate makes of that (filefmt.c:399-403)."""
    seen = set()
    for line in lines["xa"]:
        (fmt, stereo, bits), got = (ints(part) for part in line.split(":"))
        codes_per_group = 112 * 8 // bits
        want = [2 if stereo else 1, codes_per_group // 28, 18 * codes_per_group // 28, {0: 2336, 1: 2352}[fmt], 18 * codes_per_group,
                {4: 2 + 14, 8: 4 + 28}[bits]]
        assert got == want, line
        assert want[4] == {4: 4032, 8: 2016}[bits]
        seen.add((fmt, stereo, bits))
    assert seen == {(f, s, b) for f in (0, 1) for s in (0, 1) for b in (4, 8)}
    # the sector interleave: at 1x the drive reads 75 sectors a second, a channel plays 18900 or 37800 samples a second out of each of
    # its sectors -- one sector in every 75 x (samples per channel per sector) / rate is that channel's
    for line in lines["xa_interleave"]:
        (fmt, stereo, bits), got = (ints(part) for part in line.split(":"))
        per_channel = 18 * (112 * 8 // bits) // (2 if stereo else 1)
        assert got == [75 * per_channel // 18900, 75 * per_channel // 37800] and 75 * per_channel % 37800 == 0, line
        seen.discard((fmt, stereo, bits))
    assert not seen


def test_str_sector_geometry_matches_the_python_tables(lines):
    seen = set()
    for line in lines["geo"]:
        (fmt,), got = (ints(part) for part in line.split(":"))
        if fmt in str_demux_ref.GEOMETRY_OF:
            size, sub, hdr = str_demux_ref.GEOMETRY_OF[fmt]
            assert got == [1, size, -1 if sub is None else sub, hdr], line
            assert size == strdemux.SECTOR_SIZE[fmt]
        else:
            assert fmt not in strdemux.SECTOR_SIZE and got == [0, -7, -7, -7], line
        seen.add(fmt)
    assert seen == {6, 7, 9, 8}


def parse_chains(line):
    head, *rows = line.split("|")
    rows = [ints(r) for r in rows]
    return ints(head), rows


def check_chains(rows, want, want_base, line):
    assert len(rows) == len(want), line
    for r, w, b in zip(rows, want, want_base):
        assert r == [int(w["sample_offset"]), int(w["pitch"]), int(w["sample_limit"]), int(w["n_units"]), int(w["unit_stride"]), b], line


def test_planar_chains(lines):
    """stream i: one chain from sample i * stride on, its n_units records behind stream i - 1's"""
    seen = set()
    for line in lines["planar"]:
        (n, stride, pitch, limit, n_units), rows = parse_chains(line)
        assert stride > limit * pitch
        want = make_chains([i * stride for i in range(n)], pitch, limit, n_units)
        check_chains(rows, want, [i * n_units for i in range(n)], line)
        seen.add((n, pitch))
    assert seen == {(n, p) for n in (1, 3) for p in (1, 2)}


def test_interleaved_chains(lines):
    """stream i, channel c: every ch-th sample from i * stride + c on, every ch-th record from i * units_per_stream + c on"""
    seen = set()
    for line in lines["interleaved"]:
        (n, ch, stride, limit, ups), rows = parse_chains(line)
        assert stride > limit * ch and ups % ch == 0
        want = make_chains([i * stride + c for i in range(n) for c in range(ch)], ch, limit, ups // ch, unit_stride=ch)
        check_chains(rows, want, [i * ups + c for i in range(n) for c in range(ch)], line)
        # the records of a stream's chains tile its units_per_stream records exactly once
        for i in range(n):
            hit = np.zeros(n * ups, np.int32)
            for c in range(ch):
                base = rows[i * ch + c][5]
                hit[base + np.arange(ups // ch) * ch] += 1
            assert (hit[i * ups:(i + 1) * ups] == 1).all() and hit.sum() == ups, line
        seen.add((n, ch))
    assert seen == {(n, c) for n in (1, 3) for c in (1, 2)}


def test_fillers_leave_the_rest_of_a_fixed_table_alone(lines):
    assert lines["fixed4"] == [": 0 1 -1 -1 | 0 0"]


def test_bump_offsets_are_256_aligned(lines):
    sizes = [0, 1, 256, 257]
    want, at = [], 0
    for s in sizes:
        want.append(at)
        at += -(-s // 256) * 256
    assert want == [0, 0, 256, 512] and at == 1024
    assert lines["bump"] == [": " + " ".join(str(v) for v in want + [at])]
