"""Compile-time facts about the STR reader's kernels (no GPU needed: hipcc cross-compiles), by the method of
tests/test_kernel_resources.py, and the reader's entry points without a device: loud failures, argument checks, the exports."""
import ctypes as C
import shutil

import numpy as np
import pytest

from test_kernel_resources import HIPCC, _resource_usage

KERNELS = ("str_demux_scan_kernel", "str_demux_prefix_kernel", "str_demux_place_kernel", "str_demux_gather_kernel", "str_demux_finish_kernel")


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_str_demux_kernels_build_without_scratch():
    """every __global__ of str_demux_kernels.hip: no scratch, no spilled registers.  The gather kernel stages one sector and the CRC
    table in LDS (3.4 KiB per workgroup of four wavefronts): registers and LDS leave room for eight wavefronts per SIMD."""
    use = _resource_usage("str_demux_kernels.hip")
    for kernel in KERNELS:
        assert sum(kernel in k for k in use) == 1, (kernel, sorted(use))
    assert len(use) == len(KERNELS), sorted(use)
    for name, u in use.items():
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
        assert int(u["VGPRs"]) <= 64, (name, u)
        assert int(u["LDS Size"]) <= 4096, (name, u)


def _code(rc):
    from psxavenc_amd import _lib
    with pytest.raises(_lib.PsxHipError) as e:
        _lib.check(rc)
    return e.value.code


def test_entry_points_fail_loudly():
    """PSXHIP_EINVAL on bad arguments with or without a device; PSXHIP_EDEVICE without one, never a CPU fall-back"""
    import torch
    from psxavenc_amd import _lib, strdemux, strmux
    L = strdemux._bind()
    assert strdemux.kernel_rev() == "str-dmx-k1.0"
    s = strmux.settings(fmt=7, width=48, height=32)
    p = 0x10000            # the argument checks look at values only: aligned dummy addresses, never dereferenced

    def demux(settings=s, reader=None, n_streams=1, d_sectors=p, in_stride=2352 * 4, n=4, first=-1, rows=2, d_bs=p, bs_stride=4032,
              bs_stream=8064, d_sizes=p, d_info=p, d_xa=p, cap=4, xa_stream=2352 * 4, d_table=None, d_summary=p):
        return L.psxhip_str_demux_device(reader, C.byref(settings), n_streams, d_sectors, in_stride, n, first, rows, d_bs, bs_stride, bs_stream,
                                         d_sizes, d_info, d_xa, cap, xa_stream, d_table, d_summary, None)

    for bad in (dict(settings=strmux.settings(fmt=8)), dict(settings=strmux.settings(fmt=0)), dict(bs_stride=2012), dict(bs_stride=4034),
                dict(d_sectors=p + 2), dict(d_bs=p + 1), dict(d_sizes=p + 2), dict(d_info=p + 2), dict(d_xa=p + 3), dict(d_table=p + 1),
                dict(d_summary=p + 2), dict(in_stride=2354 * 4 + 2), dict(bs_stream=8066), dict(xa_stream=2353 * 4 + 1), dict(n=-1), dict(rows=-1),
                dict(cap=-1), dict(first=-2), dict(first=1 << 32), dict(n_streams=0), dict(n_streams=65536), dict(d_summary=None),
                dict(d_sectors=None), dict(d_bs=None), dict(d_xa=None), dict(n_streams=2, in_stride=2352 * 3), dict(n_streams=2, bs_stream=4032),
                dict(n_streams=2, xa_stream=2352)):
        assert _code(demux(**bad)) == _lib.PSXHIP_EINVAL, bad
    info, dec, summ = np.zeros((2, 8), np.int32), np.zeros((2, 4), np.int32), np.zeros(8, np.int32)
    sectors = np.zeros((4, 2352), np.uint8)

    def read(settings=s, n=4, rows=2, pcm_capacity=0, summary=summ.ctypes.data):
        return L.psxhip_str_read_host(None, C.byref(settings), sectors.ctypes.data, n, -1, rows, None, info.ctypes.data, dec.ctypes.data, None,
                                      pcm_capacity, None, summary)

    for bad in (dict(settings=strmux.settings(fmt=5)), dict(n=-1), dict(rows=-1), dict(pcm_capacity=-1), dict(summary=None),
                dict(settings=strmux.settings(fmt=7, fps_num=0)), dict(settings=strmux.settings(fmt=7, cd_speed=3)),
                dict(settings=strmux.settings(fmt=7, bits=5)), dict(settings=strmux.settings(fmt=7, codec=3))):
        assert _code(read(**bad)) == _lib.PSXHIP_EINVAL, bad
    if torch.cuda.is_available():
        return
    assert _code(demux()) == _lib.PSXHIP_EDEVICE
    assert _code(read()) == _lib.PSXHIP_EDEVICE
    h = C.c_void_p()
    assert _code(L.psxhip_str_reader_create(C.byref(h), 0)) == _lib.PSXHIP_EDEVICE and not h
    with pytest.raises(_lib.PsxHipError) as e:
        strdemux.StrReader(0)
    assert e.value.code == _lib.PSXHIP_EDEVICE


def test_package_exports_and_struct_sizes(tmp_path):
    import os
    import subprocess
    import psxavenc_amd
    assert callable(psxavenc_amd.StrReader) and callable(psxavenc_amd.strdemux.kernel_rev)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "psxav_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n",'
                   'sizeof(psxhip_str_frame_info_t), sizeof(psxhip_str_summary_t), sizeof(psxhip_str_sector_t),'
                   'offsetof(psxhip_str_frame_info_t, status), offsetof(psxhip_str_summary_t, n_dropped_audio));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["32", "32", "16", "28", "28"]
