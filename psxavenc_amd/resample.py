"""Audio front-end: resample + remix -- Python mirror of psxhip_resampler_* (include/psxav_hip.h).

Reference surface: the libswresample context psxavenc configures and drives (psxavenc/decoding.c:215-254,370-406): decoded PCM
-> interleaved int16 at the target rate and channel count.  Parity with libswresample itself is unpinned (FFmpeg is absent); the
arithmetic is specified in DESIGN.md section 10 and restated in numpy in tests/resample_ref.py."""
import ctypes as C

import numpy as np

from . import _lib

PCM_S16, PCM_S16P, PCM_S32, PCM_S32P, PCM_F32, PCM_F32P = range(6)
_DTYPE = {PCM_S16: np.int16, PCM_S16P: np.int16, PCM_S32: np.int32, PCM_S32P: np.int32, PCM_F32: np.float32, PCM_F32P: np.float32}


def _bind():
    L = _lib.lib()
    if getattr(L, "_resampler_bound", False):
        return L
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.psxhip_resampler_design.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i32), vp, i32]
    L.psxhip_resampler_output_count.argtypes = [i32, i32, i64, i64, i32]
    L.psxhip_resampler_output_count.restype = i64
    L.psxhip_resampler_create.argtypes = [C.POINTER(vp), i32, i32, i32, i32, i32, i32, vp]
    L.psxhip_resampler_destroy.argtypes = [vp]
    L.psxhip_resampler_destroy.restype = None
    L.psxhip_resampler_reset.argtypes = [vp]
    L.psxhip_resampler_reset.restype = None
    L.psxhip_resampler_convert_device.argtypes = [vp, vp, i64, vp, C.POINTER(i64), i32, vp]
    L.psxhip_resampler_convert_host.argtypes = [vp, vp, i64, vp, i64, C.POINTER(i64), i32]
    L.psxhip_resampler_kernel_rev.restype = C.c_char_p
    L._resampler_bound = True
    return L


def design(src_rate, dst_rate):
    """(P, T, coef (P, T) int16); raises on rates out of range.  Equal rates: (1, 0, empty)"""
    L = _bind()
    p, t = C.c_int(), C.c_int()
    _lib.check(min(0, L.psxhip_resampler_design(src_rate, dst_rate, C.byref(p), C.byref(t), None, 0)))
    coef = np.zeros((p.value, t.value), np.int16)
    if t.value:
        _lib.check(min(0, L.psxhip_resampler_design(src_rate, dst_rate, C.byref(p), C.byref(t), coef.ctypes.data, coef.size)))
    return p.value, t.value, coef


def output_count(src_rate, dst_rate, consumed, n_in, flush=False):
    n = _bind().psxhip_resampler_output_count(src_rate, dst_rate, consumed, n_in, int(bool(flush)))
    _lib.check(min(0, n))
    return n


def kernel_rev():
    return _bind().psxhip_resampler_kernel_rev().decode()


def default_matrix(src_channels, dst_channels):
    """the matrix create uses for mix=None (Q14, (dst, src)), or None where there is no default"""
    m = np.zeros((dst_channels, src_channels), np.int16)
    if src_channels == dst_channels:
        np.fill_diagonal(m, 16384)
    elif (src_channels, dst_channels) == (2, 1):
        m[0] = 8192
    elif (src_channels, dst_channels) == (1, 2):
        m[:, 0] = 16384
    elif (src_channels, dst_channels) == (6, 2):
        m[0, [0, 2, 4]] = (6786, 4799, 4799)
        m[1, [1, 2, 5]] = (6786, 4799, 4799)
    else:
        return None
    return m


class Resampler:
    """psxhip_resampler_t"""

    def __init__(self, src_format, src_channels, src_rate, dst_channels, dst_rate, mix=None, device=0):
        self._h = C.c_void_p()
        self.src_format, self.src_channels, self.src_rate = src_format, src_channels, src_rate
        self.dst_channels, self.dst_rate, self.device = dst_channels, dst_rate, device
        self.planar = bool(src_format & 1)
        self.dtype = _DTYPE.get(src_format, np.int16)
        m = None if mix is None else np.ascontiguousarray(mix, dtype=np.int16)
        if m is not None:
            assert m.shape == (dst_channels, src_channels), m.shape
        _lib.check(_bind().psxhip_resampler_create(C.byref(self._h), device, src_format, src_channels, src_rate, dst_channels, dst_rate,
                                                   None if m is None else m.ctypes.data))
        self.consumed = 0

    def close(self):
        if self._h:
            _bind().psxhip_resampler_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _bind().psxhip_resampler_reset(self._h)
        self.consumed = 0

    def output_count(self, n_in, flush=False):
        return output_count(self.src_rate, self.dst_rate, self.consumed, n_in, flush)

    def _pointers(self, planes):
        arr = (C.c_void_p * 8)()
        for k, p in enumerate(planes):
            arr[k] = p
        return arr

    def convert_host(self, pcm, flush=False):
        """pcm: numpy, (n, src_channels) interleaved or (src_channels, n) planar, of the format's dtype -> (n_out, dst_channels) int16"""
        pcm = np.ascontiguousarray(pcm, dtype=self.dtype)
        if self.planar:
            assert pcm.ndim == 2 and pcm.shape[0] == self.src_channels
            n = pcm.shape[1]
            ptrs = self._pointers([pcm[k].ctypes.data for k in range(self.src_channels)])
        else:
            pcm = pcm.reshape(-1, self.src_channels)
            n = pcm.shape[0]
            ptrs = self._pointers([pcm.ctypes.data])
        want = self.output_count(n, flush)
        out = np.zeros((max(want, 1), self.dst_channels), np.int16)
        got = C.c_int64()
        _lib.check(_bind().psxhip_resampler_convert_host(self._h, ptrs, n, out.ctypes.data, want, C.byref(got), int(bool(flush))))
        assert got.value == want
        self.consumed += n
        return out[:want]

    def convert_device(self, d_pcm, d_out=None, flush=False, stream=None):
        """d_pcm: CUDA tensor, (n, src_channels) interleaved or (src_channels, n) planar (rows may be apart: one pointer per plane)
        -> (n_out, dst_channels) int16 on the same device, asynchronous on `stream`"""
        import torch
        assert d_pcm.is_cuda
        if self.planar:
            assert d_pcm.dim() == 2 and d_pcm.shape[0] == self.src_channels and (d_pcm.shape[1] <= 1 or d_pcm.stride(1) == 1)
            n = d_pcm.shape[1]
            ptrs = self._pointers([d_pcm[k].data_ptr() for k in range(self.src_channels)])
        else:
            assert d_pcm.is_contiguous()
            n = d_pcm.numel() // self.src_channels
            ptrs = self._pointers([d_pcm.data_ptr()])
        want = self.output_count(n, flush)
        if d_out is None:
            d_out = _lib.new_tensor(stream, d_pcm.device, (want, self.dst_channels), torch.int16)
        assert d_out.is_contiguous() and d_out.numel() >= want * self.dst_channels
        st = _lib.launch_stream(stream, d_pcm.device)
        got = C.c_int64()
        _lib.check(_bind().psxhip_resampler_convert_device(self._h, ptrs, n, d_out.data_ptr() if want else None, C.byref(got),
                                                           int(bool(flush)), st.cuda_stream))
        assert got.value == want
        self.consumed += n
        return d_out[:want] if d_out.dim() == 2 else d_out
