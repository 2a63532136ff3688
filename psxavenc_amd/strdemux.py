"""STR / STRCD / STRV reader -- Python mirror of the reader section of include/psxav_hip.h.

``StrReader.demux_device`` takes muxed sectors apart on the device: one row per frame (what ``MdecDecoder.decode_frames_device`` reads),
the XA sectors compacted in stream order (what ``xa_disassemble`` reads), a record per frame, a table entry per sector, a summary per
stream.  ``StrReader.read`` is the whole reader for one stream in host memory: sectors in, pictures and PCM out.  The rules are
"psxhip STR demux v1" (DESIGN.md section 13).
"""
import ctypes as C

import numpy as np

from . import _lib
from .strmux import StrSettings

try:  # torch is plumbing (device memory, streams); read() works on numpy arrays
    import torch
except Exception:  # pragma: no cover
    torch = None

SECTOR_SIZE = {6: 2336, 7: 2352, 9: 2048}
CHUNK = 2016
# psxhip_str_frame_info_t.status
FRAME_MISSING, FRAME_DUPLICATE, FRAME_MISMATCH, FRAME_RANGE, FRAME_EDC, FRAME_GEOMETRY = 1, 2, 4, 8, 16, 32
# the int32 columns of psxhip_str_frame_info_t and psxhip_str_summary_t (frame_index, bytes_used and first_frame are unsigned in C)
INFO_FIELDS = ("frame_index", "chunk_count", "chunks_placed", "bytes_used", "width", "height", "first_sector", "status")
SUMMARY_FIELDS = ("n_video", "n_audio", "n_other", "first_frame", "n_rows", "n_complete", "n_dropped_video", "n_dropped_audio")


def _bind():
    L = _lib.lib()
    if getattr(L, "_psxhip_str_demux_bound", False):
        return L
    vp, sz, i32, i64 = C.c_void_p, C.c_size_t, C.c_int, C.c_int64
    L.psxhip_str_reader_create.argtypes = [C.POINTER(vp), i32]
    L.psxhip_str_reader_destroy.argtypes = [vp]
    L.psxhip_str_reader_destroy.restype = None
    L.psxhip_str_demux_device.argtypes = [vp, C.POINTER(StrSettings), i32, vp, sz, i32, i64, i32, vp, sz, sz, vp, vp, vp, i32, sz, vp, vp, vp]
    L.psxhip_str_read_host.argtypes = [vp, C.POINTER(StrSettings), vp, i32, i64, i32, vp, vp, vp, vp, i64, vp, vp]
    L.psxhip_str_demux_kernel_rev.restype = C.c_char_p
    L._psxhip_str_demux_bound = True
    return L


def kernel_rev():
    return _bind().psxhip_str_demux_kernel_rev().decode()


def _ptr(t):
    return t.data_ptr() if t is not None else None


class StrReader:
    """psxhip_str_reader_t: owns the workspace, and for read() the device buffers and the decoder context."""

    def __init__(self, device=0):
        self.device = int(device)
        self._h = C.c_void_p()
        _lib.check(_bind().psxhip_str_reader_create(C.byref(self._h), self.device))

    def close(self):
        if self._h:
            _bind().psxhip_str_reader_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def demux_device(self, s, d_sectors, max_frames, bs_stride, first_frame=-1, xa_capacity=None, d_bs=None, d_sizes=None, d_info=None,
                     d_xa=None, d_table=None, d_summary=None, table=True, stream=None):
        """psxhip_str_demux_device.  d_sectors: uint8 CUDA tensor (S, n_sectors, sector size), or (n_sectors, sector size) for one stream;
        its stride over streams may be padded.  Outputs (allocated, zeroed, when not given; given d_bs / d_xa may have padded strides over
        streams): d_bs (S, max_frames, bs_stride) uint8, d_sizes (S, max_frames) int32, d_info (S, max_frames, 8) int32
        [INFO_FIELDS], d_xa (S, xa_capacity, sector size) uint8 (xa_capacity None: n_sectors), d_table (S, n_sectors, 4) int32 [kind,
        frame, index, flags] (table=False: none), d_summary (S, 8) int32 [SUMMARY_FIELDS].  Returns a dict of those tensors under the
        names bs, sizes, info, xa, table, summary; asynchronous on the stream."""
        assert torch is not None and d_sectors.is_cuda and d_sectors.dtype == torch.uint8
        if d_sectors.dim() == 2:
            d_sectors = d_sectors.unsqueeze(0)
        ssz = SECTOR_SIZE[s.format]
        S, n = d_sectors.shape[0], d_sectors.shape[1]
        assert d_sectors.shape[2] == ssz and d_sectors.stride(2) == 1 and (n == 0 or d_sectors.stride(1) == ssz)
        dev = d_sectors.device
        if xa_capacity is None:
            xa_capacity = n
        if d_bs is None:
            d_bs = torch.zeros((S, max_frames, bs_stride), dtype=torch.uint8, device=dev)
        if d_sizes is None:
            d_sizes = torch.zeros((S, max_frames), dtype=torch.int32, device=dev)
        if d_info is None:
            d_info = torch.zeros((S, max_frames, 8), dtype=torch.int32, device=dev)
        if d_xa is None:
            d_xa = torch.zeros((S, xa_capacity, ssz), dtype=torch.uint8, device=dev)
        if d_table is None and table:
            d_table = torch.zeros((S, n, 4), dtype=torch.int32, device=dev)
        if d_summary is None:
            d_summary = torch.zeros((S, 8), dtype=torch.int32, device=dev)
        assert d_bs.dtype == torch.uint8 and tuple(d_bs.shape) == (S, max_frames, bs_stride) and d_bs.stride(2) == 1
        assert d_xa.dtype == torch.uint8 and tuple(d_xa.shape) == (S, xa_capacity, ssz) and (xa_capacity == 0 or d_xa.stride(1) == ssz)
        for t, shape in ((d_sizes, (S, max_frames)), (d_info, (S, max_frames, 8)), (d_summary, (S, 8))) + (((d_table, (S, n, 4)),) if d_table is not None else ()):
            assert t.dtype == torch.int32 and tuple(t.shape) == shape and t.is_contiguous()
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        assert max_frames == 0 or d_bs.stride(1) == bs_stride, "a row's pitch is bs_stride: room behind the last whole chunk is the row's margin"
        _lib.check(_bind().psxhip_str_demux_device(
            self._h, C.byref(s), S, d_sectors.data_ptr(), d_sectors.stride(0) if S > 1 else 0, n, int(first_frame), max_frames,
            d_bs.data_ptr(), bs_stride, d_bs.stride(0) if S > 1 else 0, d_sizes.data_ptr(), d_info.data_ptr(), d_xa.data_ptr(), xa_capacity,
            d_xa.stride(0) if S > 1 else 0, _ptr(d_table), d_summary.data_ptr(), st.cuda_stream))
        return dict(bs=d_bs, sizes=d_sizes, info=d_info, xa=d_xa, table=d_table, summary=d_summary)

    def read(self, s, sectors, max_frames, first_frame=-1, frames=None, pcm_sectors=None, want_frames=True):
        """psxhip_str_read_host: one stream in host memory.  sectors: (n_sectors, sector size) uint8.  frames: optional (max_frames, w*h*3/2)
        uint8 array the pictures are written into (a frame that does not decode leaves its picture as it was; zeros when not given;
        want_frames=False: no pictures).  pcm_sectors: XA sectors to decode at the most (None: all of the stream's; 0: no audio).
        Returns dict(frames, info (max_frames, 8) int32 [INFO_FIELDS], decoded (max_frames, 4) int32 [status, quant scale, version, bits
        consumed], pcm int16 (interleaved L,R when stereo), xa_status int32 per decoded XA sector, summary (8,) int32 [SUMMARY_FIELDS])."""
        ssz = SECTOR_SIZE[s.format]
        sectors = np.ascontiguousarray(sectors, dtype=np.uint8).reshape(-1, ssz)
        n = sectors.shape[0]
        if want_frames and frames is None:
            frames = np.zeros((max_frames, s.video_width * s.video_height * 3 // 2), np.uint8)
        if frames is not None:
            assert frames.dtype == np.uint8 and frames.flags.c_contiguous and frames.shape == (max_frames, s.video_width * s.video_height * 3 // 2)
        info = np.zeros((max_frames, 8), np.int32)
        decoded = np.zeros((max_frames, 4), np.int32)
        summary = np.zeros(8, np.int32)
        per_sector = 4032 if s.audio_bit_depth == 4 else 2016
        cap = n if pcm_sectors is None else int(pcm_sectors)
        pcm = np.zeros(max(cap, 1) * per_sector, np.int16)
        xa_status = np.zeros(max(cap, 1), np.int32)
        rc = _bind().psxhip_str_read_host(self._h, C.byref(s), sectors.ctypes.data if n else None, n, int(first_frame), max_frames,
                                          frames.ctypes.data if frames is not None else None, info.ctypes.data, decoded.ctypes.data,
                                          pcm.ctypes.data if cap else None, cap * per_sector, xa_status.ctypes.data, summary.ctypes.data)
        if rc < 0:
            _lib.check(rc)
        ch = max(1, s.audio_channels)
        return dict(frames=frames, info=info, decoded=decoded, pcm=pcm[:rc * ch], xa_status=xa_status[:rc * ch // per_sector],
                    summary=summary)
