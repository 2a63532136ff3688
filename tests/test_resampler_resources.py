"""Compile-time facts about the audio front-end kernel (no GPU needed: hipcc cross-compiles): every instantiation builds without
scratch and without spilled vector registers, by the method of tests/test_kernel_resources.py."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_audio_frontend_kernels_build_without_scratch():
    use = _resource_usage("audio_frontend_kernels.hip")
    shapes = {k: v for k, v in use.items() if "afe_kernel" in k}
    assert len(shapes) == 16, sorted(use)                     # 1 .. 8 output channels x (taps in LDS | in L2)
    for name, u in shapes.items():
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0", (name, u)
        assert int(u["VGPRs"]) <= 128, (name, u)              # two 256-lane groups per CU at the least
