"""MDEC BS frame decoder -- Python mirror of the decoder section of include/psxav_hip.h.

``MdecDecoder`` turns bitstreams (rows as ``MdecEncoder.encode_frames_device`` writes them) back into quantised levels and NV21
frames on the device; ``sse_device`` sums the squared errors of two sets of frames per plane; ``psnr`` is the caller's arithmetic on
those sums.  The reference has no decoder: the syntax is its encoder's, the reconstruction is "psxhip MDEC reconstruct v1"
(DESIGN.md section 11).
"""
import ctypes as C

import numpy as np

from . import _lib

try:  # torch is plumbing (device memory, streams); the host-buffer path works without it
    import torch
except Exception:  # pragma: no cover
    torch = None

# psxhip_mdec_decoded_t.status
DEC_OK, DEC_EHEADER, DEC_EVERSION, DEC_EPREMATURE, DEC_EDC, DEC_EAC, DEC_EOVERRUN, DEC_EENDCODE, DEC_ETRUNCATED = 0, -1, -2, -3, -4, -5, -6, -7, -8


def _bind():
    L = _lib.lib()
    if getattr(L, "_psxhip_decode_bound", False):
        return L
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    L.psxhip_mdec_decoder_create.argtypes = [C.POINTER(vp), i32, i32, i32, i32]
    L.psxhip_mdec_decoder_destroy.argtypes = [vp]
    L.psxhip_mdec_decoder_destroy.restype = None
    L.psxhip_mdec_decode_frames_device.argtypes = [vp, vp, sz, vp, i32, i32, vp, vp, sz, vp, vp]
    L.psxhip_mdec_decode_frames_host.argtypes = [vp, vp, sz, vp, i32, i32, vp, vp, vp]
    L.psxhip_mdec_sse_device.argtypes = [i32, vp, vp, sz, i32, i32, i32, vp, vp]
    L.psxhip_mdec_decode_kernel_rev.restype = C.c_char_p
    L._psxhip_decode_bound = True
    return L


def kernel_rev():
    return _bind().psxhip_mdec_decode_kernel_rev().decode()


class MdecDecoder:
    """One decoder context: a frame size, and whether v3 DC values wrap to 10 bits (streams of codec v3dc)."""

    def __init__(self, video_width, video_height, dc_wrap=False, device=0):
        self._h = C.c_void_p()
        self.video_width, self.video_height, self.dc_wrap, self.device = video_width, video_height, bool(dc_wrap), device
        _lib.check(_bind().psxhip_mdec_decoder_create(C.byref(self._h), device, video_width, video_height, int(self.dc_wrap)))

    @property
    def frame_bytes(self):
        return self.video_width * self.video_height * 3 // 2

    @property
    def blocks(self):
        return (self.video_width // 16) * (self.video_height // 16) * 6

    def close(self):
        if self._h:
            _bind().psxhip_mdec_decoder_destroy(self._h)
            self._h = C.c_void_p()

    destroy = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode_frames_device(self, d_bs, sizes, levels=True, frames=True, d_levels=None, d_frames=None, d_decoded=None, stream=None):
        """d_bs: uint8 CUDA tensor (n, bs_stride).  sizes: int (every frame) or int32 CUDA tensor (n,).  levels / frames: whether
        levels (n, blocks, 64) int16 and NV21 frames (n, frame_stride) uint8 are wanted; d_levels / d_frames / d_decoded: optional
        preallocated tensors.  Returns (d_levels | None, d_frames | None, d_decoded (n, 4) int32 [status, quant scale, version, bits
        consumed]); asynchronous on the stream."""
        assert torch is not None and d_bs.is_cuda and d_bs.dtype == torch.uint8 and d_bs.dim() == 2
        n = d_bs.shape[0]
        if isinstance(sizes, int):
            sizes_p, uniform = None, sizes
        else:
            assert sizes.is_cuda and sizes.dtype == torch.int32 and sizes.numel() == n and sizes.is_contiguous()
            sizes_p, uniform = sizes.data_ptr(), 0
        if d_levels is None and levels:
            d_levels = _lib.new_tensor(stream, d_bs.device, (n, self.blocks, 64), torch.int16)
        if d_frames is None and frames:
            d_frames = _lib.new_tensor(stream, d_bs.device, (n, self.frame_bytes), torch.uint8, 0)
        if d_decoded is None:
            d_decoded = _lib.new_tensor(stream, d_bs.device, (n, 4), torch.int32, 0)
        assert d_levels is None or (d_levels.dtype == torch.int16 and d_levels.is_contiguous() and d_levels.numel() == n * self.blocks * 64)
        assert d_frames is None or (d_frames.dtype == torch.uint8 and d_frames.dim() == 2 and d_frames.shape[0] == n)
        assert d_decoded.dtype == torch.int32 and d_decoded.is_contiguous() and d_decoded.numel() == n * 4
        st = _lib.launch_stream(stream, d_bs.device)
        _lib.check(_bind().psxhip_mdec_decode_frames_device(
            self._h, d_bs.data_ptr(), d_bs.stride(0), sizes_p, uniform, n, d_levels.data_ptr() if d_levels is not None else None,
            d_frames.data_ptr() if d_frames is not None else None, d_frames.stride(0) if d_frames is not None else 0,
            d_decoded.data_ptr(), st.cuda_stream))
        return d_levels, d_frames, d_decoded

    def decode_display_device(self, d_bs, sizes, out_format=0, options=0, d_decoded=None, d_dst=None, dst_pitch=None, stream=None):
        """psxhip_mdec_decode_display_device: decode_frames_device followed by display.convert_device, gated by the records; the
        NV21 frames stay in the context's workspace.  d_bs, sizes, d_decoded as decode_frames_device takes them; out_format,
        options, d_dst, dst_pitch as display.convert_device does.  Returns (d_dst (n, height, dst_pitch) uint8, d_decoded (n, 4));
        the picture of a frame that does not parse keeps its contents (zeros in a tensor made here).  Asynchronous on the stream."""
        from . import display
        assert torch is not None and d_bs.is_cuda and d_bs.dtype == torch.uint8 and d_bs.dim() == 2
        n = d_bs.shape[0]
        if isinstance(sizes, int):
            sizes_p, uniform = None, sizes
        else:
            assert sizes.is_cuda and sizes.dtype == torch.int32 and sizes.numel() == n and sizes.is_contiguous()
            sizes_p, uniform = sizes.data_ptr(), 0
        if d_decoded is None:
            d_decoded = _lib.new_tensor(stream, d_bs.device, (n, 4), torch.int32, 0)
        assert d_decoded.dtype == torch.int32 and d_decoded.is_contiguous() and d_decoded.numel() == n * 4
        d_dst = display.picture_tensor(stream, d_bs.device, n, self.video_height, out_format, self.video_width, d_dst, dst_pitch)
        st = _lib.launch_stream(stream, d_bs.device)
        _lib.check(display._bind().psxhip_mdec_decode_display_device(
            self._h, d_bs.data_ptr(), d_bs.stride(0), sizes_p, uniform, n, d_decoded.data_ptr(), out_format, options, d_dst.data_ptr(),
            d_dst.stride(1), d_dst.stride(0), st.cuda_stream))
        return d_dst, d_decoded

    def decode_frames_host(self, bs, sizes, levels=True, frames=True):
        """bs: (n, stride) uint8 host array; sizes: int or int32 sequence.  Returns (levels | None, frames | None, decoded (n, 4))."""
        bs = np.ascontiguousarray(bs, dtype=np.uint8)
        n, stride = bs.shape
        if np.isscalar(sizes):
            sizes_p, uniform = None, int(sizes)
        else:
            sizes = np.ascontiguousarray(sizes, dtype=np.int32)
            assert sizes.size == n
            sizes_p, uniform = sizes.ctypes.data, 0
        lv = np.zeros((n, self.blocks, 64), np.int16) if levels else None
        fr = np.zeros((n, self.frame_bytes), np.uint8) if frames else None
        dec = np.zeros((n, 4), np.int32)
        _lib.check(_bind().psxhip_mdec_decode_frames_host(self._h, bs.ctypes.data, stride, sizes_p, uniform, n,
                                                          lv.ctypes.data if levels else None, fr.ctypes.data if frames else None,
                                                          dec.ctypes.data))
        return lv, fr, dec


def sse_device(d_a, d_b, width, height, d_sse=None, stream=None):
    """psxhip_mdec_sse_device: d_a, d_b uint8 CUDA tensors (n, frame_stride) with equal strides -> (n, 3) sums of squared
    differences over Y, Cb, Cr (int64 tensor holding the library's uint64: a frame's sum is below 2^37); asynchronous."""
    assert torch is not None and d_a.is_cuda and d_b.is_cuda and d_a.dtype == torch.uint8 and d_b.dtype == torch.uint8
    assert d_a.dim() == 2 and d_a.shape[0] == d_b.shape[0] and d_a.stride(0) == d_b.stride(0)
    n = d_a.shape[0]
    if d_sse is None:
        d_sse = _lib.new_tensor(stream, d_a.device, (n, 3), torch.int64, 0)
    assert d_sse.dtype == torch.int64 and d_sse.is_contiguous() and d_sse.numel() == n * 3
    st = _lib.launch_stream(stream, d_a.device)
    _lib.check(_bind().psxhip_mdec_sse_device(d_a.device.index or 0, d_a.data_ptr(), d_b.data_ptr(), d_a.stride(0), width, height, n,
                                              d_sse.data_ptr(), st.cuda_stream))
    return d_sse


def psnr(sse, width, height):
    """dB per plane from sums of squared errors (..., 3) [Y, Cb, Cr] of width x height NV21 frames: 10 log10(255^2 samples / sse);
    inf where the planes are equal."""
    sse = np.asarray(sse, dtype=np.float64)
    samples = np.array([width * height, width * height // 4, width * height // 4], np.float64)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(255.0 ** 2 * samples / sse)
