"""Compile-time facts about the disc finisher's kernels (no GPU needed: hipcc cross-compiles), by the method of
tests/test_adpcm_decode_resources.py, and the finisher's entry points without a device: loud failures, every refusal of the
specification, the exports."""
import ctypes as C
import shutil

import numpy as np
import pytest

from test_kernel_resources import HIPCC, _resource_usage

KERNELS = ("disc_finish_kernel", "disc_check_kernel")


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_disc_kernels_build_without_scratch():
    """both __global__ of disc_kernels.hip: no scratch, no spilled registers.  Four sectors (588 dwords each, and 88 of column sums) and
    the CRC table in LDS: 11.6 KiB per workgroup of four wavefronts, so registers and LDS leave room for eight wavefronts per SIMD."""
    use = _resource_usage("disc_kernels.hip")
    for kernel in KERNELS:
        assert sum(kernel in k for k in use) == 1, (kernel, sorted(use))
    assert len(use) == len(KERNELS), sorted(use)
    for name, u in use.items():
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
        assert int(u["VGPRs"]) <= 64, (name, u)
        assert int(u["LDS Size"]) <= 12288, (name, u)


def _code(rc):
    from psxavenc_amd import _lib
    with pytest.raises(_lib.PsxHipError) as e:
        _lib.check(int(rc))
    return e.value.code


P = 0x100000           # the argument checks look at values only: aligned dummy addresses, never dereferenced


def _source(sectors=P, stride=2336, n=4, size=2336, file=-1, channel=-1, sub=(0, 0, 8, 0)):
    from psxavenc_amd import disc
    s = disc.DiscSource()
    s.sectors, s.stride, s.n_sectors, s.sector_size, s.file_number, s.channel_number = sectors, stride, n, size, file, channel
    for i in range(4):
        s.data_subheader[i] = sub[i]
    return s


def _table(*srcs):
    from psxavenc_amd import disc
    arr = (disc.DiscSource * max(1, len(srcs)))()
    for i, s in enumerate(srcs):
        arr[i] = s
    return arr


def test_every_refusal_of_the_specification():
    """PSXHIP_EINVAL before any device call, with or without a device"""
    from psxavenc_amd import _lib, disc
    L = disc._bind()
    assert disc.kernel_rev() == "disc-k1.0"
    out = P + (1 << 24)

    def finish(slots=(0, -1), start_lba=0, srcs=None, n_sources=None, d_out=out, first=0, n=8, lay=True):
        srcs = [_source()] if srcs is None else srcs
        layout = disc.layout(list(slots), start_lba) if lay else None
        if lay and len(slots) > 64:
            layout.period = len(slots)
        return L.psxhip_disc_finish_device(0, C.byref(layout) if lay else None, _table(*srcs), len(srcs) if n_sources is None else n_sources,
                                           d_out, first, n, None)

    bad_cases = (
        dict(lay=False), dict(n_sources=-1), dict(n_sources=65), dict(slots=()), dict(slots=(0,) * 65), dict(slots=(0, 1)), dict(slots=(0, -2)),
        dict(srcs=[_source(size=2340)]), dict(srcs=[_source(size=0)]), dict(srcs=[_source(n=-1)]), dict(srcs=[_source(stride=2338)]),
        dict(srcs=[_source(stride=2332)]), dict(srcs=[_source(stride=2048, size=2352)]), dict(srcs=[_source(sectors=P + 2)]),
        dict(srcs=[_source(sectors=None)]), dict(srcs=[_source(file=256)]), dict(srcs=[_source(file=-2)]), dict(srcs=[_source(channel=32)]),
        dict(srcs=[_source(channel=-2)]),
        dict(srcs=[_source(size=2048, stride=2048, sub=(0, 0, 0x28, 0))]),          # a 2048-byte source is never form 2
        dict(slots=(-1, -1)),                                                      # a source with sectors owns no slot
        dict(srcs=[_source(), _source(sectors=P + 0x10000)], slots=(0, 0)),        # ... the second one
        dict(start_lba=-1), dict(start_lba=450000 - 150 - 7), dict(first=-1), dict(n=-1), dict(first=450000), dict(d_out=None),
        dict(d_out=out + 1), dict(d_out=P + 2336 * 2),                              # d_out inside the source
        dict(d_out=P - 2352 * 8 + 4),                                              # d_out's end inside the source
    )
    for bad in bad_cases:
        assert _code(finish(**bad)) == _lib.PSXHIP_EINVAL, bad
    # the same table is what psxhip_disc_plan refuses (it reads no pointer and no lba)
    for bad in (dict(slots=()), dict(slots=(0, 1)), dict(srcs=[_source(size=2340)]), dict(srcs=[_source(size=2048, stride=2048, sub=(0, 0, 0x28, 0))]),
                dict(slots=(-1, -1)), dict(srcs=[_source(file=256)])):
        srcs = bad.get("srcs", [_source()])
        lay = disc.layout(list(bad.get("slots", (0, -1))), 0)
        assert L.psxhip_disc_plan(C.byref(lay), _table(*srcs), len(srcs)) == _lib.PSXHIP_EINVAL, bad
    lay = disc.layout([0, -1], -5)
    assert L.psxhip_disc_plan(C.byref(lay), _table(_source(sectors=None)), 1) == 8
    assert L.psxhip_disc_plan(None, _table(_source()), 1) == _lib.PSXHIP_EINVAL

    def check(image=P, n=4, start_lba=0, status=None, summary=P + 0x10000):
        return L.psxhip_disc_check_device(0, image, n, start_lba, status, summary, None)

    for bad in (dict(n=-1), dict(image=None), dict(image=P + 1), dict(status=P + 2), dict(summary=None), dict(summary=P + 2), dict(start_lba=-2),
                dict(start_lba=450000 - 150 - 3), dict(n=1 << 31)):
        assert _code(check(**bad)) == _lib.PSXHIP_EINVAL, bad

    host = np.zeros((4, 2336), np.uint8)
    img = np.zeros((8, 2352), np.uint8)

    def finish_host(slots=(0, -1), start_lba=0, src=None, out=img.ctypes.data, first=0, n=8):
        src = _source(sectors=host.ctypes.data) if src is None else src
        lay = disc.layout(list(slots), start_lba)
        return L.psxhip_disc_finish_host(0, C.byref(lay), _table(src), 1, out, first, n)

    for bad in (dict(slots=(-1,)), dict(start_lba=-1), dict(out=None), dict(n=-1), dict(first=-1), dict(src=_source(sectors=None)),
                dict(src=_source(sectors=host.ctypes.data, stride=2330)), dict(start_lba=449999)):
        assert _code(finish_host(**bad)) == _lib.PSXHIP_EINVAL, bad


def test_no_device_means_loud_failure():
    """PSXHIP_EDEVICE without a GPU, never a CPU fall-back (and PSXHIP_OK for the same calls' arguments: see the GPU tests)"""
    import torch
    if torch.cuda.is_available():
        return
    from psxavenc_amd import _lib, disc
    L = disc._bind()
    lay = disc.layout([0, -1], 0)
    assert _code(L.psxhip_disc_finish_device(0, C.byref(lay), _table(_source()), 1, P + (1 << 24), 0, 8, None)) == _lib.PSXHIP_EDEVICE
    assert _code(L.psxhip_disc_check_device(0, P, 4, 0, None, P + 0x10000, None)) == _lib.PSXHIP_EDEVICE
    host = np.zeros((4, 2336), np.uint8)
    with pytest.raises(_lib.PsxHipError) as e:
        disc.disc_finish_host(lay, [disc.source(host)])
    assert e.value.code == _lib.PSXHIP_EDEVICE
    assert disc.disc_plan(lay, [disc.source(host)]) == 8          # host-only: needs no device


def test_package_exports_and_struct_sizes(tmp_path):
    import os
    import subprocess
    import psxavenc_amd
    from psxavenc_amd import disc
    assert callable(psxavenc_amd.disc_plan) and callable(psxavenc_amd.disc_finish) and callable(psxavenc_amd.disc_check)
    assert callable(psxavenc_amd.disc.kernel_rev)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "psxav_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d\\n",'
                   'sizeof(psxhip_disc_source_t), sizeof(psxhip_disc_layout_t), sizeof(psxhip_disc_summary_t),'
                   'offsetof(psxhip_disc_source_t, data_subheader), offsetof(psxhip_disc_summary_t, n_edc_absent),'
                   'PSXHIP_DISC_SYNC | PSXHIP_DISC_HEADER | PSXHIP_DISC_SUBHEADER | PSXHIP_DISC_EDC | PSXHIP_DISC_ECC_P | PSXHIP_DISC_ECC_Q |'
                   'PSXHIP_DISC_EDC_ABSENT);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert got == ["40", "264", "48", "32", "40", "127"]
    assert [C.sizeof(disc.DiscSource), C.sizeof(disc.DiscLayout)] == [40, 264]
    assert disc.SUMMARY_FIELDS.index("n_edc_absent") == 10
