"""Compile-time facts about the sound bank's kernels (no GPU needed: hipcc cross-compiles), by the method of
tests/test_display_resources.py, and the entry points' argument rules, which hold with or without a device.  Both kernels stream 16
bytes per lane: one that went through scratch would double the traffic."""
import ctypes as C
import shutil

import numpy as np
import pytest

from test_kernel_resources import HIPCC, _resource_usage

EINVAL, EDEVICE = -1, -2


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_spu_bank_kernels_build_without_scratch():
    use = _resource_usage("spu_bank_kernels.hip")
    assert len(use) == 2 and any("spu_bank_frame_kernel" in k for k in use) and any("spu_bank_check_kernel" in k for k in use), sorted(use)
    for name, u in use.items():
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
        assert int(u["VGPRs"]) <= 64, (name, u)                   # eight wavefronts per SIMD
        assert u["LDS Size"] == "0", (name, u)


def _lib_and_mirror():
    from psxavenc_amd import _lib, spubank
    return _lib, spubank, spubank._bind()


def _create(s, entries, handle=True, device=0):
    _lib, spubank, L = _lib_and_mirror()
    arr, n = spubank._entry_array(entries)
    h = C.c_void_p()
    rc = L.psxhip_spu_bank_create(C.byref(h) if handle else None, device, C.byref(s), arr, n)
    return rc, h


def test_revision_and_exports():
    import psxavenc_amd
    _lib, spubank, L = _lib_and_mirror()
    assert spubank.kernel_rev() == "spubank-k1.0"
    assert psxavenc_amd.SpuBank is spubank.SpuBank
    for name in ("layout", "encode_device", "encode_host", "check_device", "decode_device", "snr_db"):
        assert callable(getattr(spubank.SpuBank, name)), name
    assert (spubank.STATUS_HEADER, spubank.STATUS_DUMMY, spubank.STATUS_FLAGS, spubank.STATUS_TRAP, spubank.STATUS_PADDING) == (1, 2, 4, 8, 16)
    assert C.sizeof(spubank.SpuBankSettings) == 20 and C.sizeof(spubank.SpuBankEntry) == 48


def test_bad_arguments_are_einval_with_or_without_a_gpu():
    _lib, spubank, L = _lib_and_mirror()
    ok, one = spubank.settings(3), [spubank.entry(0, 100, 22050)]
    bad = dict(
        no_entries=(ok, []),
        format_spui=(spubank.settings(4), one),
        alignment_not_16=(spubank.settings(3, alignment=40), one),
        bank_alignment_too_large=(spubank.settings(3, bank_alignment=1 << 17), one),
        bank_alignment_not_16=(spubank.settings(3, bank_alignment=24), one),
        beam_5=(spubank.settings(3, beam=5), one),
        samples_negative=(ok, [spubank.entry(0, -1, 22050)]),
        samples_too_many=(ok, [spubank.entry(0, 0x7FFFFFFF - 27, 22050)]),
        frequency_zero=(ok, [spubank.entry(0, 100, 0)]),
        negative_offset=(ok, [spubank.entry(-1, 100, 22050)]),
        too_large=(ok, [spubank.entry(0, 0x7FFFFFFF - 28, 22050)] * 28),
    )
    texts = set()
    for name, (s, entries) in bad.items():
        rc, h = _create(s, entries)
        assert rc == EINVAL and not h.value, name
        text = L.psxhip_last_error().decode()
        assert text.startswith("psxhip_spu_bank: "), (name, text)
        texts.add(text)
        with pytest.raises(_lib.PsxHipError) as e:
            spubank.plan(s, entries)
        assert e.value.code == EINVAL and text in str(e.value), name
    assert len(texts) == len(bad)
    assert _create(ok, one, handle=False)[0] == EINVAL
    # the calls that take a context refuse none
    assert L.psxhip_spu_bank_total_bytes(None) == EINVAL and L.psxhip_spu_bank_layout(None, None, None) == EINVAL
    assert L.psxhip_spu_bank_encode_device(None, None, None, None) == EINVAL
    assert L.psxhip_spu_bank_encode_host(None, None, 0, None, 0) == EINVAL
    assert L.psxhip_spu_bank_check_device(None, None, None, None) == EINVAL
    assert L.psxhip_spu_bank_decode_device(None, None, None, None, None, None) == EINVAL
    L.psxhip_spu_bank_destroy(None)


def test_without_a_gpu_create_fails_loudly_and_with_one_the_pointers_are_checked():
    """sound arguments: PSXHIP_EDEVICE without a device, like every other entry point.  With one, a context exists and the calls
    refuse what they cannot use before anything is launched (host memory stands in for the pointers)"""
    import torch
    _lib, spubank, L = _lib_and_mirror()
    entries = [spubank.entry(0, 100, 22050, 0, True, "a"), spubank.entry(100, 0, 11025)]
    rc, h = _create(spubank.settings(3), entries)
    if not torch.cuda.is_available():
        assert rc == EDEVICE and not h.value and "no HIP device" in L.psxhip_last_error().decode()
        with pytest.raises(_lib.PsxHipError) as e:
            spubank.SpuBank(spubank.settings(3), entries)
        assert e.value.code == EDEVICE
        return
    assert rc == 0 and h.value
    total = L.psxhip_spu_bank_total_bytes(h)
    offsets, sizes = np.zeros(2, np.int64), np.zeros(2, np.int64)
    assert L.psxhip_spu_bank_layout(h, offsets.ctypes.data, sizes.ctypes.data) == 0
    assert offsets.tolist() == [0, 48 + 128] and sizes.tolist() == [48 + 128, 48 + 64] and total == 48 + 128 + 48 + 64
    buf = np.zeros(1024, np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    for rc in (L.psxhip_spu_bank_encode_device(h, p, None, None), L.psxhip_spu_bank_encode_device(h, None, p, None),
               L.psxhip_spu_bank_encode_device(h, p, p + 8, None), L.psxhip_spu_bank_encode_device(h, p + 1, p, None),
               L.psxhip_spu_bank_encode_host(h, p, 99, p, 1024), L.psxhip_spu_bank_encode_host(h, p, 100, p, total - 1),
               L.psxhip_spu_bank_encode_host(h, None, 100, p, 1024), L.psxhip_spu_bank_encode_host(h, p, 100, None, 1024),
               L.psxhip_spu_bank_check_device(h, p, None, None), L.psxhip_spu_bank_check_device(h, None, p, None),
               L.psxhip_spu_bank_check_device(h, p + 4, p, None), L.psxhip_spu_bank_check_device(h, p, p + 2, None),
               L.psxhip_spu_bank_decode_device(h, None, p, None, None, None), L.psxhip_spu_bank_decode_device(h, p, None, None, None, None),
               L.psxhip_spu_bank_decode_device(h, p + 8, p, None, None, None), L.psxhip_spu_bank_decode_device(h, p, p + 1, None, None, None),
               L.psxhip_spu_bank_decode_device(h, p, p, p, None, None), L.psxhip_spu_bank_decode_device(h, p, p, None, p, None),
               L.psxhip_spu_bank_decode_device(h, p, p, p, p + 4, None)):
        assert rc == EINVAL
        assert L.psxhip_last_error().decode().startswith("psxhip_spu_bank_")
    L.psxhip_spu_bank_destroy(h)
