"""Compile-time facts about the picture ingest's kernels (no GPU needed: hipcc cross-compiles), by the method of
tests/test_display_resources.py.  The conversion streams: a kernel whose samples went through scratch would double the traffic it
exists to keep low, and one above 64 registers would halve the wavefronts that hide its loads."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, ROOT, _resource_usage

# layout class x depth x output mode (RGB24 replicated, RGB24 bilinear, YUV420P), not one kernel per format:
#   planar 4:2:0, planar 4:2:2, semi-planar 4:2:0     2 depths x 3 modes each    18
#   planar 4:4:4 (nothing to mix)                     2 depths x 2 modes          4
#   packed 4:2:2 (8 bits)                             3 modes                     3
#   grey (8 bits, no chroma)                          2 modes                     2
#   packed RGB (3 or 4 bytes a pixel)                 1 mode each                 2
INSTANTIATIONS = 18 + 4 + 3 + 2 + 2


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_ingest_kernels_build_without_scratch():
    use = _resource_usage("ingest_kernels.hip")
    hits = {k: v for k, v in use.items() if "ingest_convert_kernel" in k}
    assert INSTANTIATIONS == 29 and len(hits) == INSTANTIATIONS and len(hits) == len(use), sorted(use)
    for name, u in hits.items():
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
        assert int(u["VGPRs"]) <= 64, (name, u)                   # eight wavefronts per SIMD


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_ingest_kernels_pack_bytes_without_the_packed_shift():
    """as tests/test_display_resources.py says of display_kernels.hip: v_ashr_pk_u8_i32 leaves the upper half of its destination
    dirty on an MI355X; the kernel packs bytes with byte permutes (ingest_kernels.hip: pack4)"""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-S", "ingest_kernels.hip", "-o", "-"], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("s_endpgm") >= INSTANTIATIONS and "v_ashr_pk_u8_i32" not in r.stdout
    assert "v_perm_b32" in r.stdout
