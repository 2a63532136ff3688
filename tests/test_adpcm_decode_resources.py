"""Compile-time facts about the ADPCM decoder's kernels (no GPU needed: hipcc cross-compiles), by the method of
tests/test_kernel_resources.py, and the decoder's entry points without a device: loud failures, argument checks, the helpers."""
import shutil

import numpy as np
import pytest

from test_kernel_resources import HIPCC, _resource_usage


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_adpcm_decode_kernels_build_without_scratch():
    """every __global__ of adpcm_decode_kernels.hip: no scratch, no spilled registers.  The decode kernel's occupancy is set by its
    LDS rows (19.5 KiB per wavefront with 4-bit records, 23.5 KiB with 8-bit: two wavefronts per SIMD); 128 vector registers would
    still let four wavefronts share a SIMD, so registers are never what limits it."""
    use = _resource_usage("adpcm_decode_kernels.hip")
    assert sum("adpcm_decode_kernel" in k for k in use) == 4, sorted(use)             # speculate / verify x 4-bit / 8-bit
    for kernel in ("adpcm_sse_kernel", "adpcm_decode_final_kernel"):        # (xa_disassemble_kernel: sector_kernels.hip,
        assert sum(kernel in k for k in use) == 1, (kernel, sorted(use))    #  tests/test_kernel_resources.py)
    for name, u in use.items():
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
        if "adpcm_decode_kernel" in name:
            assert int(u["VGPRs"]) <= 128, (name, u)
            assert int(u["LDS Size"]) <= 160 * 1024 // 6, (name, u)                    # six wavefronts per CU at the least


def _err(fn, *args):
    from psxavenc_amd import _lib
    with pytest.raises(_lib.PsxHipError) as e:
        rc = fn(*args)
        if rc < 0:
            _lib.check(rc)
    return e.value.code


def test_entry_points_fail_loudly():
    """PSXHIP_EINVAL on bad arguments with or without a device; PSXHIP_EDEVICE without one, never a CPU fall-back"""
    import torch
    from psxavenc_amd import _lib, adpcm_decode
    from psxavenc_amd.adpcm import CHAIN_DTYPE, make_chains
    L = adpcm_decode._bind()
    assert adpcm_decode.kernel_rev().startswith("adpcm-dec-k")
    # the argument checks look at values only: aligned dummy addresses, never dereferenced
    p = 0x10000
    for fc, bits in ((5, 8), (3, 4), (6, 4), (4, 5), (4, 16)):
        assert _err(L.psxhip_adpcm_decode_chains_device, 0, p, p, p, 1, fc, bits, p, p, None, None, None) == _lib.PSXHIP_EINVAL
        ch = make_chains([0], 1, 28, 1)
        base = np.zeros(1, np.int32)
        assert _err(L.psxhip_adpcm_decode_chains_chunked, 0, p, ch.ctypes.data, base.ctypes.data, 1, fc, bits, p, p, None, None, 4, 8, 0,
                    None) == _lib.PSXHIP_EINVAL
    assert _err(L.psxhip_adpcm_decode_chains_device, 0, p, p, p, -1, 5, 4, p, p, None, None, None) == _lib.PSXHIP_EINVAL
    ch = make_chains([0], 0, 28, 1)                  # pitch < 1
    assert ch.dtype == CHAIN_DTYPE
    base = np.zeros(1, np.int32)
    assert _err(L.psxhip_adpcm_decode_chains_chunked, 0, p, ch.ctypes.data, base.ctypes.data, 1, 5, 4, p, p, None, None, 4, 8, 0,
                None) == _lib.PSXHIP_EINVAL
    assert _err(L.psxhip_adpcm_sse_device, 0, p, None, p, p, -1, None, None, None, None) == _lib.PSXHIP_EINVAL
    assert _err(L.psxhip_xa_disassemble_device, 0, p, 1, 0, 1, 37800, 5, p, None, None) == _lib.PSXHIP_EINVAL
    assert _err(L.psxhip_xa_disassemble_device, 0, p, -1, 0, 1, 37800, 4, p, None, None) == _lib.PSXHIP_EINVAL
    assert _err(L.psxhip_xa_disassemble_device, 0, p, 1, 2, 1, 37800, 4, p, None, None) == _lib.PSXHIP_EINVAL
    blocks = np.zeros((1, 32), np.uint8)
    st = np.zeros((1, 2), np.int32)
    out = np.zeros((1, 56), np.int16)
    assert _err(L.psxhip_spu_decode_streams_host, 0, blocks.ctypes.data, 1, 32, -1, st.ctypes.data, out.ctypes.data, 56) == _lib.PSXHIP_EINVAL
    assert _err(L.psxhip_xa_decode_streams_host, 0, 0, 1, 37800, 7, blocks.ctypes.data, 1, 2336, 1, st.ctypes.data, out.ctypes.data, 56,
                None) == _lib.PSXHIP_EINVAL
    if torch.cuda.is_available():
        return
    ch = make_chains([0], 1, 28, 1)
    assert _err(L.psxhip_adpcm_decode_chains_device, 0, p, p, p, 1, 5, 4, p, p, None, None, None) == _lib.PSXHIP_EDEVICE
    assert _err(L.psxhip_adpcm_decode_chains_chunked, 0, p, ch.ctypes.data, base.ctypes.data, 1, 5, 4, p, p, None, None, 4, 8, 0,
                None) == _lib.PSXHIP_EDEVICE
    assert _err(L.psxhip_adpcm_sse_device, 0, p, None, p, p, 1, None, None, p, None) == _lib.PSXHIP_EDEVICE
    assert _err(L.psxhip_xa_disassemble_device, 0, p, 1, 0, 1, 37800, 4, p, None, None) == _lib.PSXHIP_EDEVICE
    with pytest.raises(_lib.PsxHipError) as e:
        adpcm_decode.spu_decode_streams(blocks)
    assert e.value.code == _lib.PSXHIP_EDEVICE
    with pytest.raises(_lib.PsxHipError) as e:
        from psxavenc_amd.adpcm import XaSettings
        adpcm_decode.xa_decode_streams(XaSettings(), np.zeros((1, 2336), np.uint8))
    assert e.value.code == _lib.PSXHIP_EDEVICE


def test_package_exports():
    import psxavenc_amd
    for name in ("decode_chains_device", "decode_chains_chunked", "adpcm_sse", "xa_disassemble", "spu_decode_streams", "xa_decode_streams",
                 "snr_db"):
        assert callable(getattr(psxavenc_amd, name)), name
    assert callable(psxavenc_amd.adpcm_decode.kernel_rev)


def test_snr_helper():
    from psxavenc_amd import snr_db
    got = snr_db(np.array([[100, 100000], [0, 5], [7, 0], [0, 0]], np.int64))
    assert np.isclose(got[0], 30.0) and np.isposinf(got[1]) and np.isneginf(got[2]) and np.isnan(got[3])
    # the library's sums are uint64 held in int64 tensors: a sum above 2^63 reads back right
    big = np.array([[1, -(2 ** 63)]], np.int64)
    assert np.isclose(snr_db(big)[0], 10 * np.log10(2.0 ** 63))
