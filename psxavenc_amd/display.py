"""Display back-end -- Python mirror of the display section of include/psxav_hip.h.

``convert_device`` turns NV21 frames (as ``MdecDecoder.decode_frames_device`` writes them) into RGB24, RGBX32 or the PlayStation
frame buffer's 15-bit pixels on the device; ``MdecDecoder.decode_display_device`` (decode.py) goes from bitstreams to pictures in one
call.  The arithmetic is "psxhip display v1" (DESIGN.md section 18).
"""
import ctypes as C

import numpy as np

from . import _lib

try:  # torch is plumbing (device memory, streams); the host-buffer path works without it
    import torch
except Exception:  # pragma: no cover
    torch = None

OUT_RGB24, OUT_RGBX32, OUT_RGB555 = 0, 1, 2                        # out_format
DISPLAY_CHROMA_BILINEAR, DISPLAY_DITHER, DISPLAY_MASK_BIT = 1, 2, 4   # options


def _bind():
    L = _lib.lib()
    if getattr(L, "_psxhip_display_bound", False):
        return L
    vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    L.psxhip_display_row_bytes.argtypes = [i32, i32]
    L.psxhip_display_row_bytes.restype = sz
    L.psxhip_display_convert_device.argtypes = [i32, vp, sz, i32, i32, i32, vp, i32, u32, vp, sz, sz, vp]
    L.psxhip_display_convert_host.argtypes = [i32, vp, i32, i32, i32, i32, u32, vp]
    L.psxhip_mdec_decode_display_device.argtypes = [vp, vp, sz, vp, i32, i32, vp, i32, u32, vp, sz, sz, vp]
    L.psxhip_display_kernel_rev.restype = C.c_char_p
    L._psxhip_display_bound = True
    return L


def kernel_rev():
    return _bind().psxhip_display_kernel_rev().decode()


def row_bytes(out_format, width):
    """bytes of one row of pixels; 0 on a bad format"""
    return int(_bind().psxhip_display_row_bytes(out_format, width))


def picture_tensor(stream, device, n, height, out_format, width, d_dst, dst_pitch):
    """the (n, height, dst_pitch) uint8 destination of a device call: the caller's d_dst (its strides are the placement), or a new
    one of the launch stream, zeroed -- pictures of skipped frames and bytes past the row bytes read as 0"""
    if d_dst is None:
        pitch = row_bytes(out_format, width) if dst_pitch is None else dst_pitch
        return _lib.new_tensor(stream, device, (n, height, pitch), torch.uint8, 0)
    assert d_dst.is_cuda and d_dst.dtype == torch.uint8 and d_dst.dim() == 3 and d_dst.shape[:2] == (n, height) and d_dst.stride(2) == 1
    assert dst_pitch is None or dst_pitch == d_dst.stride(1)
    return d_dst


def convert_device(d_frames, width, height, out_format=OUT_RGB24, options=0, d_decoded=None, d_dst=None, dst_pitch=None, stream=None):
    """psxhip_display_convert_device: d_frames uint8 CUDA tensor (n, frame_stride) of NV21 frames -> uint8 tensor (n, height,
    dst_pitch), of which the first row_bytes(out_format, width) bytes of a row are the pixels.  d_decoded: optional (n, 4) int32
    records of the decoder; a frame whose status is not 0 is skipped.  d_dst: optional preallocated (n, height, pitch) tensor or
    view (its strides are dst_stride and dst_pitch: a window of a larger surface); else dst_pitch (default: the row bytes) sizes a
    new, zeroed one.  Asynchronous on the stream."""
    assert torch is not None and d_frames.is_cuda and d_frames.dtype == torch.uint8 and d_frames.dim() == 2 and d_frames.stride(1) == 1
    n = d_frames.shape[0]
    assert d_decoded is None or (d_decoded.is_cuda and d_decoded.dtype == torch.int32 and d_decoded.is_contiguous() and d_decoded.numel() == n * 4)
    d_dst = picture_tensor(stream, d_frames.device, n, height, out_format, width, d_dst, dst_pitch)
    st = _lib.launch_stream(stream, d_frames.device)
    _lib.check(_bind().psxhip_display_convert_device(
        d_frames.device.index or 0, d_frames.data_ptr(), d_frames.stride(0), width, height, n,
        d_decoded.data_ptr() if d_decoded is not None else None, out_format, options, d_dst.data_ptr(), d_dst.stride(1), d_dst.stride(0),
        st.cuda_stream))
    return d_dst


def convert_host(frames, width, height, out_format=OUT_RGB24, options=0, device=0):
    """psxhip_display_convert_host: frames (n, width * height * 3 / 2) uint8 host array -> (n, height, row bytes) uint8"""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    assert frames.ndim == 2 and frames.shape[1] == width * height * 3 // 2
    n = frames.shape[0]
    out = np.zeros((n, height, row_bytes(out_format, width)), np.uint8)
    _lib.check(_bind().psxhip_display_convert_host(device, frames.ctypes.data, width, height, n, out_format, options, out.ctypes.data))
    return out
