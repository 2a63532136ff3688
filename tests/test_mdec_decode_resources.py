"""Compile-time facts about the decoder's kernels (no GPU needed: hipcc cross-compiles), by the method of
tests/test_kernel_resources.py: parse, reconstruct and SSE build for gfx950 without scratch and without spilled registers.  The parse
kernel keeps its whole reader state in scalar registers; a state that went to scratch would put a memory round trip into every
code of the chain."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_decode_kernels_build_without_scratch():
    use = _resource_usage("mdec_decode_kernels.hip")
    for kernel in ("mdec_parse_kernel", "mdec_reconstruct_kernel", "mdec_sse_kernel"):
        hits = {k: v for k, v in use.items() if kernel in k}
        assert len(hits) == 1, (kernel, sorted(use))
        for name, u in hits.items():
            assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
            assert int(u["VGPRs"]) <= 64, (name, u)           # eight wavefronts per SIMD


def test_decoder_without_a_gpu_fails_loudly():
    """create returns PSXHIP_EDEVICE without a device, like every other entry point; bad sizes are PSXHIP_EINVAL with or without"""
    import torch
    from psxavenc_amd import MdecDecoder, _lib, decode
    assert decode.kernel_rev().startswith("mdec-dec-k")
    with pytest.raises(_lib.PsxHipError) as e:
        MdecDecoder(320, 250)
    assert e.value.code == _lib.PSXHIP_EINVAL
    if torch.cuda.is_available():
        MdecDecoder(320, 240).close()
        return
    with pytest.raises(_lib.PsxHipError) as e:
        MdecDecoder(320, 240)
    assert e.value.code == _lib.PSXHIP_EDEVICE


def test_psnr_helper():
    import numpy as np
    from psxavenc_amd import psnr
    w, h = 320, 240
    got = psnr(np.array([[w * h, w * h // 4, 0]]), w, h)       # mean squared error 1, 1, 0
    assert np.allclose(got[0, :2], 20 * np.log10(255.0)) and np.isinf(got[0, 2])
