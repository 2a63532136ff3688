"""Picture ingest -- Python mirror of the ingest section of include/psxav_hip.h.

``Ingest.convert_device`` turns the pictures a video decoder produces (planar, semi-planar or packed; 8 or 10 bits; padded rows; any
of five matrices, limited or full range) into one of the scaler's two inputs on the device, picking the source picture of every output
picture from an index; ``ingest_scale_device`` runs it and the scaler on one stream.  ``fit``, ``pace`` and ``recommend`` are the
planners, which need no device.  The arithmetic is "psxhip ingest v1" (DESIGN.md section 19).
"""
import ctypes as C

import numpy as np

from . import _lib

try:  # torch is plumbing (device memory, streams); the host-buffer path and the planners work without it
    import torch
except Exception:  # pragma: no cover
    torch = None

(SRC_YUV420P, SRC_YUV422P, SRC_YUV444P, SRC_NV12, SRC_NV21, SRC_YUYV422, SRC_UYVY422, SRC_YUV420P10, SRC_YUV422P10, SRC_YUV444P10,
 SRC_P010, SRC_GRAY8, SRC_RGB24, SRC_BGR24, SRC_RGBA32, SRC_BGRA32) = range(16)                            # src_format
MATRIX_BT601, MATRIX_BT709, MATRIX_SMPTE240M, MATRIX_FCC, MATRIX_BT2020_NCL = range(5)                     # matrix
PIX_RGB24, PIX_YUV420P = 0, 1                                                                              # out_format (the scaler's)
INGEST_CHROMA_BILINEAR = 1                                                                                 # options


class Plane(C.Structure):
    """psxhip_ingest_plane_t"""
    _fields_ = [("offset", C.c_size_t), ("pitch", C.c_size_t)]


def _bind():
    L = _lib.lib()
    if getattr(L, "_psxhip_ingest_bound", False):
        return L
    vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    L.psxhip_ingest_create.argtypes = [C.POINTER(vp), i32, i32, i32, i32, vp, i32, i32, i32, i32, u32]
    L.psxhip_ingest_destroy.argtypes = [vp]
    L.psxhip_ingest_destroy.restype = None
    L.psxhip_ingest_output_bytes.argtypes = [vp]
    L.psxhip_ingest_output_bytes.restype = sz
    L.psxhip_ingest_source_bytes.argtypes = [vp]
    L.psxhip_ingest_source_bytes.restype = sz
    L.psxhip_ingest_matrix.argtypes = [vp, vp]
    L.psxhip_ingest_convert_device.argtypes = [vp, vp, sz, i32, vp, i32, vp, sz, vp]
    L.psxhip_ingest_convert_host.argtypes = [vp, vp, sz, i32, vp, i32, vp, sz]
    L.psxhip_ingest_kernel_rev.restype = C.c_char_p
    L.psxhip_ingest_recommend.argtypes = [i32, i32, i32, i32]
    L.psxhip_ingest_fit.argtypes = [i32, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.psxhip_ingest_pace.argtypes = [vp, i32, i32, i32, i32, i32, vp, i32]
    L._psxhip_ingest_bound = True
    return L


def kernel_rev():
    return _bind().psxhip_ingest_kernel_rev().decode()


def recommend(src_format, matrix, width, height):
    """psxhip_ingest_recommend: PIX_YUV420P where the cheap path is allowed, else PIX_RGB24"""
    rc = _bind().psxhip_ingest_recommend(src_format, matrix, width, height)
    _lib.check(rc if rc < 0 else 0)
    return rc


def fit(src_w, src_h, max_w, max_h, ignore_aspect=False):
    """psxhip_ingest_fit: the target size reduced to the source's aspect ratio -> (width, height)"""
    w, h = C.c_int(), C.c_int()
    _lib.check(_bind().psxhip_ingest_fit(src_w, src_h, max_w, max_h, int(bool(ignore_aspect)), C.byref(w), C.byref(h)))
    return w.value, h.value


def pace(pts, tb_num, tb_den, fps_num, fps_den):
    """psxhip_ingest_pace: time stamps of the decoded pictures -> int32 array, the source picture of every output frame"""
    pts = np.ascontiguousarray(pts, dtype=np.int64)
    L = _bind()
    n = L.psxhip_ingest_pace(pts.ctypes.data, pts.size, tb_num, tb_den, fps_num, fps_den, None, 0)
    _lib.check(n if n < 0 else 0)
    out = np.zeros(n, np.int32)
    assert L.psxhip_ingest_pace(pts.ctypes.data, pts.size, tb_num, tb_den, fps_num, fps_den, out.ctypes.data, n) == n
    return out


class Ingest:
    """psxhip_ingest_t"""

    def __init__(self, src_format, width, height, planes, matrix=MATRIX_BT601, full_range=False, out_format=PIX_RGB24, options=0, device=0):
        """planes: (offset, pitch) in bytes of every plane of the format"""
        self._h = C.c_void_p()
        arr = (Plane * max(1, len(planes)))(*[Plane(int(o), int(p)) for o, p in planes])
        _lib.check(_bind().psxhip_ingest_create(C.byref(self._h), device, src_format, width, height, C.cast(arr, C.c_void_p), len(planes),
                                                matrix, int(bool(full_range)), out_format, options))
        self.width, self.height, self.out_format, self.device = width, height, out_format, device
        self.output_bytes = int(_bind().psxhip_ingest_output_bytes(self._h))
        self.source_bytes = int(_bind().psxhip_ingest_source_bytes(self._h))

    create = classmethod(lambda cls, *a, **kw: cls(*a, **kw))

    def close(self):
        if self._h:
            _bind().psxhip_ingest_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def matrix(self):
        """psxhip_ingest_matrix: (cy, rv, gu, gv, bu, yoff, coff)"""
        out = np.zeros(7, np.int32)
        _lib.check(_bind().psxhip_ingest_matrix(self._h, out.ctypes.data))
        return tuple(int(v) for v in out)

    def convert_device(self, d_src, d_src_index=None, n_out=None, d_out=None, stream=None):
        """psxhip_ingest_convert_device: d_src uint8 CUDA tensor (n_src, src_stride) -> uint8 tensor (n_out, out_stride), of which the
        first output_bytes of a row are the picture.  d_src_index: optional int32 CUDA tensor (n_out,), the source picture of every
        output picture (negative: left as it is); else n_out = n_src, picture for picture.  d_out: optional preallocated tensor or
        view (its row stride is out_stride); else a new, zeroed one of the launch stream.  Asynchronous on the stream."""
        assert torch is not None and d_src.is_cuda and d_src.dtype == torch.uint8 and d_src.dim() == 2 and d_src.stride(1) == 1
        n_src = d_src.shape[0]
        if d_src_index is not None:
            assert d_src_index.is_cuda and d_src_index.dtype == torch.int32 and d_src_index.dim() == 1 and d_src_index.is_contiguous()
            assert n_out is None or n_out == d_src_index.numel()
            n_out = d_src_index.numel()
        elif n_out is None:
            n_out = n_src
        if d_out is None:
            d_out = _lib.new_tensor(stream, d_src.device, (n_out, self.output_bytes), torch.uint8, 0)
        assert d_out.is_cuda and d_out.dtype == torch.uint8 and d_out.dim() == 2 and d_out.shape[0] == n_out and d_out.stride(1) == 1
        st = _lib.launch_stream(stream, d_src.device)
        _lib.check(_bind().psxhip_ingest_convert_device(
            self._h, d_src.data_ptr(), d_src.stride(0), n_src, d_src_index.data_ptr() if d_src_index is not None else None, n_out,
            d_out.data_ptr(), d_out.stride(0), st.cuda_stream))
        return d_out

    def convert_host(self, src, src_index=None, out=None):
        """psxhip_ingest_convert_host: src (n_src, src_stride) uint8 host array -> (n_out, out_stride) uint8; out: the destination as
        it is before the call (default: zeros, tightly packed)"""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        assert src.ndim == 2
        index = None if src_index is None else np.ascontiguousarray(src_index, dtype=np.int32)
        n_out = src.shape[0] if index is None else index.size
        out = np.zeros((n_out, self.output_bytes), np.uint8) if out is None else np.ascontiguousarray(out, dtype=np.uint8)
        assert out.ndim == 2 and out.shape[0] == n_out
        _lib.check(_bind().psxhip_ingest_convert_host(self._h, src.ctypes.data, src.shape[1], src.shape[0],
                                                      None if index is None else index.ctypes.data, n_out, out.ctypes.data, out.shape[1]))
        return out


def ingest_scale_device(ingest, scaler, d_src, d_src_index=None, d_frames=None, stream=None):
    """Both stages on one stream: decoder pictures -> (ingest) the scaler's input -> (scaler) NV21 frames of the encoder's size.  The
    scaler is one created for ingest.out_format at the ingest's size; the intermediate pictures are a tensor of the launch stream.
    Returns the frames (n_out, scaler.frame_bytes); asynchronous."""
    assert scaler.source_bytes == ingest.output_bytes
    d_mid = ingest.convert_device(d_src, d_src_index, stream=stream)
    return scaler.convert_device(d_mid, d_frames, stream=stream)
