"""Compile-time facts about the seam kernels ("psxhip SPU loop seam v1"; no GPU needed: hipcc cross-compiles), by
the method of tests/test_spu_bank_resources.py, and the seam entry points' argument rules, which hold with or without a device.  The
report kernel keeps two decoders and a block in registers through two fully unrolled units: what must not happen to it is scratch."""
import ctypes as C
import shutil

import numpy as np
import pytest

from test_kernel_resources import HIPCC, _resource_usage

EINVAL, EDEVICE = -1, -2


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_spu_seam_kernels_build_without_scratch():
    use = _resource_usage("spu_seam_kernels.hip")
    assert len(use) == 2 and any("spu_seam_step_kernel" in k for k in use) and any("spu_seam_report_kernel" in k for k in use), sorted(use)
    for name, u in use.items():
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
        assert u["LDS Size"] == "0" and u["Dynamic Stack"] == "False", (name, u)
        assert int(u["VGPRs"]) <= 256, (name, u)


def _lib_and_mirror():
    from psxavenc_amd import _lib, spubank
    return _lib, spubank, spubank._bind()


def test_revision_and_exports():
    import psxavenc_amd
    _lib, spubank, L = _lib_and_mirror()
    assert spubank.seam_kernel_rev() == "spuseam-k1.0"
    assert spubank.kernel_rev() == "spubank-k1.0", "the framing kernels did not change"
    for name in ("set_seam", "seam_passes", "seam_report", "seam_records"):
        assert callable(getattr(psxavenc_amd.SpuBank, name)), name
    assert (spubank.SEAM_OFF, spubank.SEAM_STEADY, spubank.SEAM_PASSES) == (0, 1, 8)
    assert C.sizeof(spubank.SpuSeam) == 40 == spubank.SEAM_DTYPE.itemsize
    assert [f[0] for f in spubank.SpuSeam._fields_] == list(spubank.SEAM_DTYPE.names)
    assert [getattr(spubank.SpuSeam, n).offset for n in spubank.SEAM_DTYPE.names] == [spubank.SEAM_DTYPE.fields[n][1] for n in spubank.SEAM_DTYPE.names]
    assert C.sizeof(spubank.SpuBankSettings) == 20, "the settings struct did not change"
    with open(_lib.__file__.replace("psxavenc_amd/_lib.py", "include/psxav_hip.h")) as f:
        header = f.read()
    for name in ("psxhip_spu_bank_set_seam", "psxhip_spu_bank_seam_passes_device", "psxhip_spu_bank_seam_device", "psxhip_spu_seam_kernel_rev",
                 "PSXHIP_SPU_SEAM_OFF 0", "PSXHIP_SPU_SEAM_STEADY 1", "PSXHIP_SPU_SEAM_PASSES 8"):
        assert name in header, name


def test_a_null_bank_is_einval_with_or_without_a_gpu():
    _lib, spubank, L = _lib_and_mirror()
    texts = set()
    for call in (lambda: L.psxhip_spu_bank_set_seam(None, 1), lambda: L.psxhip_spu_bank_seam_passes_device(None, None, None),
                 lambda: L.psxhip_spu_bank_seam_device(None, None, None, None, None)):
        assert call() == EINVAL
        text = L.psxhip_last_error().decode()
        assert text.startswith("psxhip_spu_bank_s"), text
        texts.add(text)
    assert len(texts) == 3


def test_with_a_gpu_the_mode_and_the_pointers_are_checked():
    """the calls refuse what they cannot use before anything is launched (host memory stands in for the pointers); without a device
    no context exists to call them with (tests/test_spu_bank_resources.py holds create to PSXHIP_EDEVICE there)"""
    import torch
    _lib, spubank, L = _lib_and_mirror()
    entries = [spubank.entry(0, 100, 22050, 0, True, "a"), spubank.entry(100, 0, 11025)]
    arr, n = spubank._entry_array(entries)
    h = C.c_void_p()
    s = spubank.settings(3)
    rc = L.psxhip_spu_bank_create(C.byref(h), 0, C.byref(s), arr, n)
    if not torch.cuda.is_available():
        assert rc == EDEVICE and not h.value
        return
    assert rc == 0 and h.value
    buf = np.zeros(1024, np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    texts = set()

    def refused(rc):
        assert rc == EINVAL
        text = L.psxhip_last_error().decode()
        assert text.startswith("psxhip_spu_bank_s"), text
        texts.add(text)
    for mode in (-1, 2, 8):
        refused(L.psxhip_spu_bank_set_seam(h, mode))
    refused(L.psxhip_spu_bank_seam_passes_device(h, p, None))           # the mode is off
    assert L.psxhip_spu_bank_set_seam(h, 1) == 0 and L.psxhip_spu_bank_set_seam(h, 0) == 0
    refused(L.psxhip_spu_bank_seam_passes_device(h, p, None))           # and off again
    assert L.psxhip_spu_bank_set_seam(h, 1) == 0
    for args in ((h, None, None), (h, p + 2, None)):
        refused(L.psxhip_spu_bank_seam_passes_device(*args))
    for args in ((h, None, None, p, None), (h, p, None, None, None), (h, p + 8, None, p, None), (h, p, None, p + 4, None), (h, p, p + 1, p, None)):
        refused(L.psxhip_spu_bank_seam_device(*args))
    assert len(texts) == 6, "three modes, the mode that is off, and a text per call for its pointers"
    L.psxhip_spu_bank_destroy(h)
