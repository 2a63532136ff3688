"""Compile-time facts about the beam encoder's kernels (adpcm_beam_kernels.hip; no GPU needed: hipcc cross-compiles), by the method
of tests/test_kernel_resources.py: no scratch, no spills, the register counts DESIGN.md section 22 states; and the symbols exported."""
import ctypes as C
import os
import re
import shutil

import pytest

from test_kernel_resources import HIPCC, ROOT, _resource_usage

# vector registers per instantiation as DESIGN.md section 22 gives them: a change in either place is a change in both
VGPRS = {"adpcm_beam_chains_kernel": 95, "adpcm_beam_chunks_kernelILb0E": 100, "adpcm_beam_chunks_kernelILb1E": 102}


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_beam_kernels_build_without_scratch_or_spills():
    use = _resource_usage("adpcm_beam_kernels.hip")
    assert len(use) == 3, sorted(use)
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    for k, vgprs in VGPRS.items():
        hits = [u for name, u in use.items() if k in name]
        assert len(hits) == 1, (k, sorted(use))
        u = hits[0]
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (k, u)
        assert int(u["VGPRs"]) == vgprs, (k, u)
        assert int(u["VGPRs"]) <= 128                                 # four wavefronts per SIMD at the least
    stated = re.search(r"VGPRs: serial (\d+), speculate (\d+), verify (\d+)", design)
    assert stated and [int(v) for v in stated.groups()] == [VGPRS["adpcm_beam_chains_kernel"], VGPRS["adpcm_beam_chunks_kernelILb0E"],
                                                            VGPRS["adpcm_beam_chunks_kernelILb1E"]]


def test_symbols_and_revisions():
    from psxavenc_amd import _lib
    L = _lib.lib()
    for name in ("psxhip_adpcm_beam_encode_chains_device", "psxhip_adpcm_beam_encode_chains_chunked", "psxhip_adpcm_session_set_beam",
                 "psxhip_spu_encode_streams_host_beam", "psxhip_xa_encode_streams_host_beam", "psxhip_adpcm_beam_kernel_rev",
                 # ... and none removed
                 "psxhip_adpcm_encode_chains_device", "psxhip_adpcm_encode_chains_chunked", "psxhip_adpcm_session_create",
                 "psxhip_adpcm_session_run", "psxhip_adpcm_session_reset", "psxhip_adpcm_session_destroy", "psxhip_adpcm_session_set_timing",
                 "psxhip_adpcm_session_last_timing", "psxhip_spu_encode_streams_host", "psxhip_xa_encode_streams_host",
                 "psxhip_xa_encode_streams_host_flags", "psxhip_spu_pack_device", "psxhip_xa_assemble_device", "psxhip_adpcm_release_blocks",
                 "psxhip_adpcm_chunked_threshold", "psxhip_adpcm_pick_chunking", "psxhip_adpcm_kernel_rev"):
        assert hasattr(L, name), name
    L.psxhip_adpcm_beam_kernel_rev.restype = C.c_char_p
    L.psxhip_adpcm_kernel_rev.restype = C.c_char_p
    assert L.psxhip_adpcm_beam_kernel_rev() == b"adpcm-beam-k1.0"
    assert L.psxhip_adpcm_kernel_rev().startswith(b"adpcm-k")


def test_the_beam_width_is_refused_before_any_device_is_asked_for():
    """beam outside 1 .. 4 is PSXHIP_EINVAL with or without a device"""
    from psxavenc_amd import _lib, adpcm
    L = adpcm._bind()
    assert L.psxhip_adpcm_beam_encode_chains_chunked(0, None, None, None, 0, 5, 4, None, None, 9, 4, 2, 0, None) == _lib.PSXHIP_EINVAL
    assert L.psxhip_spu_encode_streams_host_beam(0, None, 0, 0, 1, 0, None, None, 0, 0) == _lib.PSXHIP_EINVAL
    assert "beam 1 .. 4" in L.psxhip_last_error().decode()
