"""Compile-time facts about the STRSPU reader's kernels (no GPU needed: hipcc cross-compiles), by the method of
tests/test_strspu_resources.py, and the reader's entry points without a device: loud failures, argument checks, the exports."""
import ctypes as C
import shutil

import numpy as np
import pytest

from test_kernel_resources import HIPCC, _resource_usage

KERNELS = ("strspu_demux_init_kernel", "strspu_demux_scan_kernel", "strspu_demux_finish_kernel")


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_strspu_demux_kernels_build_without_scratch():
    """every __global__ of strspu_demux_kernels.hip: no scratch, no spilled registers; the de-interleave kernel -- a load, a store and
    index arithmetic, in its 16-byte and its four-dword form -- no LDS, and registers that leave a SIMD its eight wavefronts"""
    use = _resource_usage("strspu_demux_kernels.hip")
    for kernel in KERNELS:
        assert sum(kernel in k for k in use) == 1, (kernel, sorted(use))
    hot = {k: u for k, u in use.items() if "spu_deinterleave_kernel" in k}
    assert len(hot) == 2 and len(use) == len(KERNELS) + 2, sorted(use)
    for name, u in use.items():
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
    for name, u in hot.items():
        assert u["LDS Size"] == "0" and u["Occupancy"] == "8", (name, u)


def _code(rc):
    from psxavenc_amd import _lib
    with pytest.raises(_lib.PsxHipError) as e:
        _lib.check(int(rc))
    return e.value.code


P = 0x100000           # the argument checks look at values only: aligned dummy addresses, never dereferenced


def _settings(**kw):
    from psxavenc_amd import strmux
    base = dict(fmt=8, width=48, height=32, channels=2, frequency=44100, tail=strmux.TAIL_COMPLETE)
    base.update(kw)
    return strmux.settings(**base)


def _demux(L, settings=None, reader=None, n_streams=1, d_sectors=P, in_stride=2048 * 4, n=4, first=-1, rows=2, d_bs=P, bs_stride=4032,
           bs_stream=8064, d_sizes=P, d_info=P, d_units=P, cap=4, units_stream=4 * 126 * 16, d_chunk=P, d_table=None, d_summary=P, d_asum=P):
    s = settings if settings is not None else _settings()
    return L.psxhip_strspu_demux_device(reader, C.byref(s), n_streams, d_sectors, in_stride, n, first, rows, d_bs, bs_stride, bs_stream, d_sizes,
                                        d_info, d_units, cap, units_stream, d_chunk, d_table, d_summary, d_asum, None)


def _deint(L, d_in=P, n=4, chunk_stride=2048, lane_offset=0x20, lane_bytes=1008, channels=2, src=None, streams=1, in_stride=4 * 2048,
           d_units=P + (1 << 24), units_stream=4 * 126 * 16):
    return L.psxhip_spu_deinterleave_device(0, d_in, n, chunk_stride, lane_offset, lane_bytes, channels, src, streams, in_stride, d_units,
                                            units_stream, None)


def _read(L, settings=None, n=4, rows=2, pcm_capacity=0, summary=True):
    s = settings if settings is not None else _settings()
    sectors = np.zeros((4, 2048), np.uint8)
    info, dec, summ = np.zeros((2, 8), np.int32), np.zeros((2, 4), np.int32), np.zeros(8, np.int32)
    return L.psxhip_strspu_read_host(None, C.byref(s), sectors.ctypes.data, n, -1, rows, None, info.ctypes.data, dec.ctypes.data, None,
                                     pcm_capacity, None, summ.ctypes.data if summary else None, None)


def test_entry_points_refuse_bad_arguments():
    """PSXHIP_EINVAL before any device call, with or without a device"""
    from psxavenc_amd import _lib, strdemux, strmux
    L = strdemux._bind()
    bad_settings = (
        _settings(audio_id=0x8001),                       # the audio id equals the video id
        _settings(video_id=-1),                           # any video id, with audio
        _settings(channels=3),
        _settings(fmt=9), _settings(fmt=7),
    )
    undefined_bit = _settings()
    undefined_bit.strspu_options |= 1 << 18
    for s in bad_settings + (undefined_bit,):
        assert _code(_demux(L, settings=s)) == _lib.PSXHIP_EINVAL
        assert _code(_read(L, settings=s)) == _lib.PSXHIP_EINVAL
    for bad in (dict(d_units=P + 4), dict(d_units=P + 8), dict(units_stream=4 * 126 * 16 + 4), dict(cap=strdemux.STRSPU_MAX_CHUNKS + 1), dict(cap=-1),
                dict(d_units=None), dict(d_chunk=None), dict(d_chunk=P + 2), dict(d_asum=None), dict(d_asum=P + 1), dict(n_streams=0),
                dict(n_streams=65536), dict(n_streams=2, units_stream=4 * 126 * 16 - 16), dict(n_streams=2, in_stride=2048 * 3),
                dict(n_streams=2, bs_stream=4032), dict(d_sectors=P + 2), dict(d_bs=P + 1), dict(bs_stride=2012), dict(d_summary=None),
                dict(d_table=P + 1), dict(n=-1), dict(rows=-1), dict(first=-2)):
        assert _code(_demux(L, **bad)) == _lib.PSXHIP_EINVAL, bad
    for bad in (dict(lane_bytes=1000), dict(lane_bytes=0), dict(lane_bytes=24), dict(channels=0), dict(lane_offset=0x40), dict(channels=3),
                dict(chunk_stride=2016), dict(lane_offset=0x22), dict(chunk_stride=2050), dict(d_in=P + 2), dict(d_units=P + (1 << 24) + 4),
                dict(units_stream=4 * 126 * 16 + 8), dict(in_stride=4 * 2048 + 2), dict(src=P + 2), dict(n=-1), dict(streams=0), dict(streams=65536),
                dict(d_in=None), dict(d_units=None), dict(streams=2, units_stream=4 * 126 * 16 - 16), dict(streams=2, in_stride=3 * 2048),
                dict(n=(1 << 31) // 126 + 1)):
        assert _code(_deint(L, **bad)) == _lib.PSXHIP_EINVAL, bad
    for bad in (dict(n=-1), dict(rows=-1), dict(pcm_capacity=-1), dict(summary=False), dict(settings=_settings(fps_num=0)),
                dict(settings=_settings(cd_speed=3)), dict(settings=_settings(codec=3))):
        assert _code(_read(L, **bad)) == _lib.PSXHIP_EINVAL, bad


def test_no_device_means_loud_failure():
    """PSXHIP_EDEVICE without a GPU, never a CPU fall-back"""
    import torch
    if torch.cuda.is_available():
        return
    from psxavenc_amd import _lib, strdemux
    L = strdemux._bind()
    assert _code(_demux(L)) == _lib.PSXHIP_EDEVICE
    assert _code(_demux(L, settings=_settings(channels=0), cap=0, d_units=None, d_chunk=None)) == _lib.PSXHIP_EDEVICE
    assert _code(_deint(L)) == _lib.PSXHIP_EDEVICE
    assert _code(_deint(L, lane_offset=0, lane_bytes=16, channels=3, chunk_stride=48, units_stream=4 * 3 * 16)) == _lib.PSXHIP_EDEVICE
    assert _code(_read(L)) == _lib.PSXHIP_EDEVICE


def test_the_old_entry_points_still_refuse_format_8():
    from psxavenc_amd import _lib, strdemux
    L = strdemux._bind()
    s = _settings()
    rc = L.psxhip_str_demux_device(None, C.byref(s), 1, P, 2048 * 4, 4, -1, 2, P, 4032, 8064, P, P, P, 4, 2048 * 4, None, P, None)
    assert _code(rc) == _lib.PSXHIP_EINVAL
    assert b"psxhip_strspu_demux_device" in L.psxhip_last_error()          # the refusal names the call that takes format 8
    info, dec, summ = np.zeros((2, 8), np.int32), np.zeros((2, 4), np.int32), np.zeros(8, np.int32)
    sectors = np.zeros((4, 2048), np.uint8)
    rc = L.psxhip_str_read_host(None, C.byref(s), sectors.ctypes.data, 4, -1, 2, None, info.ctypes.data, dec.ctypes.data, None, 0, None,
                                summ.ctypes.data)
    assert _code(rc) == _lib.PSXHIP_EINVAL and b"psxhip_strspu_read_host" in L.psxhip_last_error()
    assert strdemux.kernel_rev() == "str-dmx-k1.0"


def test_package_exports_and_struct_sizes(tmp_path):
    import os
    import subprocess
    import psxavenc_amd
    from psxavenc_amd import strdemux
    assert strdemux.strspu_demux_kernel_rev() == "strspu-dmx-k1.0"
    assert callable(strdemux.StrReader.demux_strspu_device) and callable(strdemux.StrReader.read_strspu)
    assert callable(strdemux.spu_deinterleave_device) and callable(psxavenc_amd.spu_deinterleave_device)
    assert len(strdemux.CHUNK_FIELDS) == 8 and len(strdemux.AUDIO_SUMMARY_FIELDS) == 4
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "psxav_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %d %d %d\\n",'
                   'sizeof(psxhip_strspu_chunk_info_t), sizeof(psxhip_strspu_audio_summary_t), sizeof(psxhip_str_summary_t),'
                   'sizeof(psxhip_str_settings_t), offsetof(psxhip_strspu_chunk_info_t, flags), offsetof(psxhip_strspu_audio_summary_t, last_chunk),'
                   'PSXHIP_STRSPU_CHUNK_MISSING, PSXHIP_STRSPU_CHUNK_DUPLICATE, PSXHIP_STRSPU_CHUNK_MISMATCH);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert got == ["32", "16", "32", "64", "24", "8", "1", "2", "4"]
