"""Compile-time facts about the disc reader's kernels (no GPU needed: hipcc cross-compiles), by the method of
tests/test_disc_resources.py, and the reader's entry points without a device: loud failures, every refusal of the specification
(DESIGN.md section 17), the exports."""
import ctypes as C
import shutil

import numpy as np
import pytest

from test_kernel_resources import HIPCC, _resource_usage

KERNELS = ("disc_read_classify_kernel", "disc_read_count_kernel", "disc_read_prefix_kernel", "disc_read_place_kernel",
           "disc_read_gather_kernel")


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_disc_read_kernels_build_without_scratch():
    """every __global__ of disc_read_kernels.hip: no scratch, no spilled registers, at most 128 VGPRs (four wavefronts per SIMD) and
    16 KiB of LDS per workgroup (four sectors of 588 dwords with 88 of column sums each, the CRC table, the log table).  Built:
    classify 44 VGPRs / 12 180 bytes of LDS, gather 32 / 11 092, count 10, prefix 7, place 14 and no LDS."""
    use = _resource_usage("disc_read_kernels.hip")
    for kernel in KERNELS:
        assert sum(kernel in k for k in use) == 1, (kernel, sorted(use))
    assert len(use) == len(KERNELS), sorted(use)
    for name, u in use.items():
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
        assert int(u["VGPRs"]) <= 128, (name, u)
        assert int(u["LDS Size"]) <= 16384, (name, u)


def _code(rc):
    from psxavenc_amd import _lib
    with pytest.raises(_lib.PsxHipError) as e:
        _lib.check(int(rc))
    return e.value.code


P = 0x100000           # the argument checks look at values only: aligned dummy addresses, never dereferenced
IMAGE = P + (1 << 26)
COUNTS, SUMMARY, TABLE = P + (1 << 27), P + (1 << 27) + 0x1000, P + (1 << 27) + 0x2000


def _track(sectors=P, stride=2336, capacity=4, size=2336, file=-1, channel=-1, mask=0, value=0):
    from psxavenc_amd import discread
    t = discread.DiscTrack()
    t.sectors, t.stride, t.capacity, t.sector_size, t.file_number, t.channel_number = sectors, stride, capacity, size, file, channel
    t.submode_mask, t.submode_value = mask, value
    return t


def _table(*tracks):
    from psxavenc_amd import discread
    arr = (discread.DiscTrack * max(1, len(tracks)))()
    for i, t in enumerate(tracks):
        arr[i] = t
    return arr


@pytest.fixture
def handle():
    """a reader where there is a device, NULL where there is none: the argument checks come before either is looked at"""
    import torch
    from psxavenc_amd import discread
    if not torch.cuda.is_available():
        yield None
        return
    r = discread.DiscReader(0)
    yield r._h
    r.close()


def _read(handle, image=IMAGE, n=8, tracks=None, n_tracks=None, table=None, counts=COUNTS, summary=SUMMARY):
    from psxavenc_amd import discread
    tracks = [_track()] if tracks is None else tracks
    return discread._bind().psxhip_disc_read_device(handle, image, n, _table(*tracks), len(tracks) if n_tracks is None else n_tracks, table,
                                                    counts, summary, None)


def test_every_refusal_of_the_specification(handle):
    """PSXHIP_EINVAL before any device call, with or without a device"""
    from psxavenc_amd import _lib, discread
    assert discread.kernel_rev() == "disc-rd-k1.0"
    bad_calls = [
        dict(image=IMAGE + 2), dict(table=TABLE + 1), dict(counts=COUNTS + 2), dict(summary=SUMMARY + 3),      # a misaligned pointer
        dict(summary=SUMMARY + 4),                                                                              # (the summary: 8-byte aligned)
        dict(tracks=[_track(sectors=P + 2)]), dict(tracks=[_track(stride=2338)]),                               # ... or stride
        dict(tracks=[_track(stride=2332)]), dict(tracks=[_track(size=2352, stride=2048)]),                      # stride < sector_size
        dict(tracks=[_track(size=2340, stride=2340)]), dict(tracks=[_track(size=0)]), dict(tracks=[_track(size=2324, stride=2336)]),
        dict(tracks=[_track(file=256)]), dict(tracks=[_track(file=-2)]), dict(tracks=[_track(channel=32)]), dict(tracks=[_track(channel=-2)]),
        dict(tracks=[_track(capacity=-1)]),
        dict(tracks=[_track(capacity=0, sectors=None)] * 65),                                                   # more than 64 tracks
        dict(n_tracks=-1), dict(n=-1), dict(n=1 << 31),
        dict(tracks=[_track(sectors=IMAGE + 2352 * 2)]),                                                        # a track inside the image
        dict(tracks=[_track(sectors=IMAGE - 2336 * 4 + 4)]),                                                    # a track's end inside the image
        dict(tracks=[_track(), _track(sectors=P + 2336 * 3)]),                                                  # two tracks overlap
        dict(tracks=[_track(stride=4096), _track(sectors=P + 2336, stride=4096)]),                              # ... by their extents
        dict(image=None), dict(summary=None), dict(counts=None), dict(tracks=[_track(sectors=None)]),           # NULL where one is needed
    ]
    for bad in bad_calls:
        assert _code(_read(handle, **bad)) == _lib.PSXHIP_EINVAL, bad
    L = discread._bind()
    assert _code(L.psxhip_disc_read_device(handle, IMAGE, 8, None, 1, None, COUNTS, SUMMARY, None)) == _lib.PSXHIP_EINVAL

    host = np.zeros((4, 2336), np.uint8)
    img = np.zeros((8, 2352), np.uint8)
    counts, summary = np.zeros(4, np.int32), np.zeros(16, np.int32)

    def read_host(image=img.ctypes.data, n=8, track=None, counts=counts.ctypes.data, summary=summary.ctypes.data):
        track = _track(sectors=host.ctypes.data) if track is None else track
        return L.psxhip_disc_read_host(handle, image, n, _table(track), 1, None, counts, summary)

    for bad in (dict(image=None), dict(n=-1), dict(n=1 << 31), dict(counts=None), dict(summary=None), dict(track=_track(sectors=None)),
                dict(track=_track(sectors=host.ctypes.data, stride=2330)), dict(track=_track(sectors=host.ctypes.data, size=2000)),
                dict(track=_track(sectors=host.ctypes.data, capacity=-1)), dict(track=_track(sectors=host.ctypes.data, file=300)),
                dict(track=_track(sectors=host.ctypes.data, channel=40))):
        assert _code(read_host(**bad)) == _lib.PSXHIP_EINVAL, bad
    assert not counts.any() and not summary.any() and not host.any()


def test_no_device_means_loud_failure():
    """PSXHIP_EDEVICE without a GPU, never a CPU fall-back (the same arguments succeed with one: see the GPU tests)"""
    import torch
    if torch.cuda.is_available():
        return
    from psxavenc_amd import _lib, discread
    L = discread._bind()
    h = C.c_void_p()
    assert _code(L.psxhip_disc_reader_create(C.byref(h), 0)) == _lib.PSXHIP_EDEVICE and not h
    assert _code(_read(None)) == _lib.PSXHIP_EDEVICE
    assert _code(_read(None, n=0, image=None)) == _lib.PSXHIP_EDEVICE
    with pytest.raises(_lib.PsxHipError) as e:
        discread.disc_read_host(np.zeros((2, 2352), np.uint8), [discread.track(np.zeros((2, 2336), np.uint8))])
    assert e.value.code == _lib.PSXHIP_EDEVICE
    host = np.zeros((4, 2336), np.uint8)
    img = np.zeros((8, 2352), np.uint8)
    counts, summary = np.zeros(4, np.int32), np.zeros(16, np.int32)
    assert _code(L.psxhip_disc_read_host(None, img.ctypes.data, 8, _table(_track(sectors=host.ctypes.data)), 1, None, counts.ctypes.data,
                                         summary.ctypes.data)) == _lib.PSXHIP_EDEVICE


def test_package_exports_and_struct_sizes(tmp_path):
    import os
    import subprocess
    import psxavenc_amd
    from psxavenc_amd import disc, discread
    assert callable(psxavenc_amd.disc_read) and callable(psxavenc_amd.disc_read_host) and callable(psxavenc_amd.DiscReader)
    assert callable(psxavenc_amd.discread.kernel_rev) and callable(psxavenc_amd.discread.track)
    assert disc.kernel_rev() == "disc-k1.0"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "psxav_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %d\\n",'
                   'sizeof(psxhip_disc_track_t), sizeof(psxhip_disc_read_sector_t), sizeof(psxhip_disc_read_summary_t),'
                   'offsetof(psxhip_disc_track_t, submode_mask), offsetof(psxhip_disc_read_summary_t, n_dropped),'
                   'offsetof(psxhip_disc_read_summary_t, n_corrections),'
                   'PSXHIP_DISC_READ_REPAIRED | PSXHIP_DISC_READ_UNREPAIRABLE | PSXHIP_DISC_READ_EDC | PSXHIP_DISC_READ_EDC_ABSENT |'
                   'PSXHIP_DISC_READ_SYNC | PSXHIP_DISC_READ_SUBHEADER | PSXHIP_DISC_READ_EMPTY | PSXHIP_DISC_READ_UNCLAIMED |'
                   'PSXHIP_DISC_READ_DROPPED | PSXHIP_DISC_READ_FORM);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert got == ["40", "16", "64", "32", "48", "56", "1023"]
    assert [C.sizeof(discread.DiscTrack), C.sizeof(discread.DiscReadSummary)] == [40, 64]
    assert discread.DiscTrack.submode_mask.offset == 32 and discread.DiscReadSummary.n_corrections.offset == 56
    assert discread.SUMMARY_FIELDS.index("n_dropped") == 12 and len(discread.SECTOR_FIELDS) == 4
    assert (discread.REPAIRED, discread.FORM) == (1, 512)
