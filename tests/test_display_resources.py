"""Compile-time facts about the display back-end's kernels (no GPU needed: hipcc cross-compiles), by the method of
tests/test_kernel_resources.py, and the entry points' argument rules, which hold with or without a device.  The conversion streams: a
kernel whose pixels went through scratch would double the traffic it exists to keep low."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_kernel_resources import CSRC, HIPCC, ROOT, _resource_usage


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_display_kernels_build_without_scratch():
    use = _resource_usage("display_kernels.hip")
    hits = {k: v for k, v in use.items() if "display_convert_kernel" in k}
    # RGB24 and RGBX32 x 2 chroma modes; RGB555 x 2 chroma modes x dither x mask bit
    assert len(hits) == 12 and len(hits) == len(use), sorted(use)
    for name, u in hits.items():
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
        assert int(u["VGPRs"]) <= 64, (name, u)                   # eight wavefronts per SIMD


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_display_kernels_pack_bytes_without_the_packed_shift():
    """The compiler folds `clamp(a >> 16, 0, 255) | clamp(b >> 16, 0, 255) << 8` into v_ashr_pk_u8_i32 and reads the upper half of
    its result as zero; an MI355X leaves that half of the register as it was, and the bytes ORed in above it came out wrong
    (RGB24 and RGBX32, first GPU run of this kernel).  The kernel packs with byte permutes instead (display_kernels.hip: pack4);
    this keeps the instruction from coming back with a later edit."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-S", "display_kernels.hip", "-o", "-"], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("s_endpgm") >= 12 and "v_ashr_pk_u8_i32" not in r.stdout
    assert "v_perm_b32" in r.stdout


def _bound():
    from psxavenc_amd import display
    return display._bind()


def _convert(width=32, height=16, n=0, fmt=0, options=0, frames=None, dst=None, frame_stride=None, pitch=None, stride=None):
    """psxhip_display_convert_device with sound arguments except those given; n = 0: no memory is touched"""
    from psxavenc_amd import display
    row = display.row_bytes(fmt, width) or 4 * width
    pitch = row if pitch is None else pitch
    return _bound().psxhip_display_convert_device(0, frames, width * height * 3 // 2 if frame_stride is None else frame_stride, width, height, n,
                                                  None, fmt, options, dst, pitch, height * pitch if stride is None else stride, None)


def test_row_bytes_and_revision():
    from psxavenc_amd import display
    assert display.kernel_rev().startswith("disp-k")
    assert [display.row_bytes(f, 320) for f in (display.OUT_RGB24, display.OUT_RGBX32, display.OUT_RGB555)] == [960, 1280, 640]
    assert display.row_bytes(3, 320) == 0 and display.row_bytes(-1, 320) == 0
    assert (display.DISPLAY_CHROMA_BILINEAR, display.DISPLAY_DITHER, display.DISPLAY_MASK_BIT) == (1, 2, 4)


def test_bad_arguments_are_einval_with_or_without_a_gpu():
    from psxavenc_amd import _lib, display
    bad = dict(
        width_not_a_multiple_of_16=dict(width=40),
        width_too_large=dict(width=1040),
        height_too_small=dict(height=0),
        unknown_format=dict(fmt=3),
        misaligned_pitch=dict(pitch=3 * 32 + 2),
        pitch_below_the_row_bytes=dict(pitch=3 * 32 - 4),
        stride_below_the_picture=dict(stride=16 * 96 - 4),
        misaligned_stride=dict(stride=16 * 96 + 2),
        misaligned_frame_stride=dict(frame_stride=32 * 16 * 3 // 2 + 2),
        frame_stride_below_the_frame=dict(frame_stride=32 * 16 * 3 // 2 - 4),
        dither_with_rgb24=dict(fmt=display.OUT_RGB24, options=display.DISPLAY_DITHER),
        mask_bit_with_rgbx32=dict(fmt=display.OUT_RGBX32, options=display.DISPLAY_MASK_BIT),
        unknown_option_bit=dict(fmt=display.OUT_RGB555, options=8),
        negative_frame_count=dict(n=-1),
        frames_without_pointers=dict(n=1),
    )
    for name, kw in bad.items():
        assert _convert(**kw) == _lib.PSXHIP_EINVAL, name
        assert _lib.lib().psxhip_last_error().decode().startswith("psxhip_display_convert_device:"), name
    # host memory stands in for the pointers: the rules below are decided before anything would be read
    frames, dst = np.zeros(32 * 16 * 3 // 2 + 16, np.uint8), np.zeros(16 * 96 + 16, np.uint8)
    f, d = frames.ctypes.data + (-frames.ctypes.data) % 16, dst.ctypes.data + (-dst.ctypes.data) % 16
    assert _convert(n=1, frames=f, dst=d + 2) == _lib.PSXHIP_EINVAL                # misaligned destination
    assert _convert(n=1, frames=f + 1, dst=d) == _lib.PSXHIP_EINVAL                # misaligned source
    assert _convert(n=1, frames=f, dst=f + 32) == _lib.PSXHIP_EINVAL               # the pictures overlap the frames
    # the host entry and the decode-and-display entry check the same rules
    L = _bound()
    assert L.psxhip_display_convert_host(0, None, 40, 16, 0, 0, 0, None) == _lib.PSXHIP_EINVAL
    assert L.psxhip_display_convert_host(0, None, 32, 16, 0, display.OUT_RGB24, display.DISPLAY_DITHER, None) == _lib.PSXHIP_EINVAL
    assert L.psxhip_display_convert_host(0, None, 32, 16, 1, 0, 0, None) == _lib.PSXHIP_EINVAL
    assert L.psxhip_mdec_decode_display_device(None, None, 0, None, 0, 0, None, 0, 0, None, 96, 16 * 96, None) == _lib.PSXHIP_EINVAL


def test_without_a_gpu_the_entry_points_fail_loudly():
    """sound arguments: PSXHIP_EDEVICE without a device, like every other entry point; success with one (no frames: nothing runs)"""
    import torch
    from psxavenc_amd import _lib
    want = _lib.PSXHIP_OK if torch.cuda.is_available() else _lib.PSXHIP_EDEVICE
    assert _convert() == want
    assert _convert(fmt=2, options=7, pitch=2 * 32 + 68) == want
    assert _bound().psxhip_display_convert_host(0, None, 32, 16, 0, 0, 0, None) == want
    if not torch.cuda.is_available():
        assert "no HIP device" in _lib.lib().psxhip_last_error().decode()
