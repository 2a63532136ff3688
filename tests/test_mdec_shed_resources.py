"""Compile-time facts about the refinement's kernels (mdec_shed_kernels.hip; no GPU needed: hipcc cross-compiles), by the method of
tests/test_kernel_resources.py, the entry points' argument rules, which hold with or without a device, and the symbols exported."""
import ctypes as C
import shutil

import pytest

from test_kernel_resources import HIPCC, _resource_usage

KERNELS = ("mdec_shed_analyse_kernel", "mdec_shed_decide_kernel", "mdec_shed_emit_kernel")


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_shed_kernels_build_without_scratch_or_spills():
    use = _resource_usage("mdec_shed_kernels.hip")
    assert len(use) == 3, sorted(use)
    for k in KERNELS:
        hits = [u for name, u in use.items() if k in name]
        assert len(hits) == 1, (k, sorted(use))
        u = hits[0]
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (k, u)
        assert int(u["VGPRs"]) <= 128, (k, u)                     # four 4-wavefront groups per SIMD pair at the least


def _lib():
    from psxavenc_amd import _lib
    return _lib


def test_symbols_and_revision():
    L = _lib().lib()
    for name in ("psxhip_mdec_refine_frames_device", "psxhip_mdec_encode_refine_frames_host", "psxhip_mdec_shed_kernel_rev"):
        assert hasattr(L, name), name
    L.psxhip_mdec_shed_kernel_rev.restype = C.c_char_p
    assert L.psxhip_mdec_shed_kernel_rev() == b"mdec-shed-k1.0"
    # the existing kernels' revisions are what they were
    L.psxhip_mdec_decode_kernel_rev.restype = C.c_char_p
    assert L.psxhip_version() == b"psxav_hip 0.4 (gfx950, mdec-k3.11)"
    assert L.psxhip_mdec_decode_kernel_rev().startswith(b"mdec-dec-k")


def test_without_a_context_the_calls_fail_loudly():
    """no context can exist without a device: PSXHIP_EDEVICE there, PSXHIP_EINVAL where there is one"""
    import torch
    lib = _lib()
    L = lib.lib()
    want = lib.PSXHIP_EINVAL if torch.cuda.is_available() else lib.PSXHIP_EDEVICE
    assert L.psxhip_mdec_refine_frames_device(None, None, 0, 0, None, 8, 1, None, 0, None, None, None) == want
    assert L.psxhip_mdec_encode_refine_frames_host(None, None, 0, None, 8, 1, None, 0, None, None) == want
    if not torch.cuda.is_available():
        assert "no HIP device" in L.psxhip_last_error().decode()
