"""Compile-time facts about format 8's audio sector kernel (no GPU needed: hipcc cross-compiles), by the method of
tests/test_disc_resources.py, and the entry points without a device: loud failures, argument checks, the exports.

The kernel lives in strspu_kernels.hip, beside sector_kernels.hip (whose own kernels keep building as they did: that is
tests/test_kernel_resources.py)."""
import ctypes as C
import shutil

import pytest

from test_kernel_resources import HIPCC, _resource_usage


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_strspu_kernel_builds_without_scratch_and_without_lds():
    """one lane per 16 bytes, a load, selects and stores: no LDS, no scratch, no spill, and registers that leave a SIMD its eight
    wavefronts"""
    use = _resource_usage("strspu_kernels.hip")
    assert len(use) == 1 and sum("strspu_audio_sector_kernel" in k for k in use) == 1, sorted(use)
    for name, u in use.items():
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
        assert u["LDS Size"] == "0", (name, u)
        assert int(u["VGPRs"]) <= 32 and u["Occupancy"] == "8", (name, u)
    # ... and sector_kernels.hip still compiles for gfx950, with the video sector kernel format 8 shares with the other flavours
    sector = _resource_usage("sector_kernels.hip")
    assert sum("str_video_sector_kernel" in k for k in sector) == 1, sorted(sector)


def _code(rc):
    from psxavenc_amd import _lib
    with pytest.raises(_lib.PsxHipError) as e:
        _lib.check(int(rc))
    return e.value.code


P = 0x100000           # the argument checks look at values only: aligned dummy addresses, never dereferenced


def _sectors(L, units=P, n=4, channels=2, frequency=44100, options=1, streams=1, ustride=4 * 126 * 16, out=P + (1 << 24), dst=None, ostride=4 * 2048):
    return L.psxhip_strspu_audio_sectors_device(0, units, n, channels, frequency, options, streams, ustride, out, dst, ostride, None)


def test_audio_sector_builder_refuses_bad_arguments():
    """PSXHIP_EINVAL before any device call, with or without a device"""
    from psxavenc_amd import _lib, strmux
    L = strmux._bind()
    bad_cases = (
        dict(units=None), dict(out=None), dict(units=P + 4), dict(units=P + 8), dict(out=P + (1 << 24) + 2), dict(ustride=4 * 126 * 16 + 4),
        dict(ostride=4 * 2048 + 2), dict(dst=P + 0x8002), dict(n=-1), dict(n=(1 << 31) // 126 + 1), dict(channels=0), dict(channels=3),
        dict(frequency=0), dict(frequency=-1), dict(options=1 | (1 << 18)), dict(options=1 | (1 << 31)), dict(streams=0), dict(streams=65536),
        dict(streams=2, ustride=4 * 126 * 16 - 16), dict(streams=2, ostride=4 * 2048 - 4),
    )
    for bad in bad_cases:
        assert _code(_sectors(L, **bad)) == _lib.PSXHIP_EINVAL, bad


def test_no_device_means_loud_failure():
    """PSXHIP_EDEVICE without a GPU, never a CPU fall-back -- the builder, and both muxer paths with format 8"""
    import numpy as np
    import torch
    if torch.cuda.is_available():
        return
    from psxavenc_amd import _lib, strmux
    L = strmux._bind()
    assert _code(_sectors(L)) == _lib.PSXHIP_EDEVICE
    assert _code(_sectors(L, out=P + (1 << 24) + 4, dst=P + 0x8000, options=0xFFFF | strmux.STRSPU_LOOP | strmux.STRSPU_NO_LEADING_DUMMY)) == _lib.PSXHIP_EDEVICE
    with pytest.raises(_lib.PsxHipError) as e:
        strmux.StrMuxer((0,))
    assert e.value.code == _lib.PSXHIP_EDEVICE
    # the handle-less checks of the muxer still speak: a NULL handle with format 8 settings
    s = strmux.settings(fmt=strmux.FORMAT_STRSPU, width=48, height=32, frequency=44100, tail=strmux.TAIL_COMPLETE)
    frames = np.zeros((2, 48 * 32 * 3 // 2), np.uint8)
    out = np.zeros((64, 2048), np.uint8)
    rc = L.psxhip_str_encode_host(None, C.byref(s), frames.ctypes.data, 2, None, 0, out.ctypes.data, out.size, None)
    assert _code(rc) == _lib.PSXHIP_EINVAL
    rc = L.psxhip_str_encode_device(None, C.byref(s), 1, P, 0, 2, None, 0, 0, P + (1 << 24), 64 * 2048, None, None)
    assert _code(rc) == _lib.PSXHIP_EINVAL


def test_package_exports_and_struct_size(tmp_path):
    import os
    import subprocess
    from psxavenc_amd import strmux
    assert strmux.FORMAT_STRSPU == 8 and callable(strmux.strspu_audio_sectors_device)
    assert strmux.strspu_kernel_rev() == "strspu-k1.0"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "psxav_mdec.h"\n#include "psxav_hip.h"\nint main(void){printf("%zu %zu %d %d %d %d\\n",'
                   'sizeof(psxhip_str_settings_t), offsetof(psxhip_str_settings_t, strspu_options), PSXHIP_STRSPU_ID_MASK, PSXHIP_STRSPU_LOOP,'
                   'PSXHIP_STRSPU_NO_LEADING_DUMMY, (int)FORMAT_STRSPU);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert got == ["64", "60", "65535", "65536", "131072", "8"]          # no struct size change: the field was `reserved`
    assert C.sizeof(strmux.StrSettings) == 64 and strmux.StrSettings.strspu_options.offset == 60
