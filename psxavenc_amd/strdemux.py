"""STR / STRCD / STRV reader -- Python mirror of the reader section of include/psxav_hip.h.

``StrReader.demux_device`` takes muxed sectors apart on the device: one row per frame (what ``MdecDecoder.decode_frames_device`` reads),
the XA sectors compacted in stream order (what ``xa_disassemble`` reads), a record per frame, a table entry per sector, a summary per
stream.  ``StrReader.read`` is the whole reader for one stream in host memory: sectors in, pictures and PCM out.  The rules are
"psxhip STR demux v1" (DESIGN.md section 13).

``StrReader.demux_strspu_device`` and ``StrReader.read_strspu`` are the same for format 8 (STRSPU): the video rows as above, the audio
chunks de-interleaved into SPU unit records in the order ``decode_chains_*`` reads, a record per chunk, a second summary per stream
("psxhip STRSPU demux v1").  ``spu_deinterleave_device`` is the de-interleave on its own, for SPUI / VAGI bodies.
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
# psxhip_strspu_chunk_info_t.status, and the int32 columns of psxhip_strspu_chunk_info_t and psxhip_strspu_audio_summary_t
CHUNK_MISSING, CHUNK_DUPLICATE, CHUNK_MISMATCH = 1, 2, 4
CHUNK_FIELDS = ("first_sector", "status", "channels", "lane_bytes", "frequency", "first_sample", "flags", "reserved")
AUDIO_SUMMARY_FIELDS = ("n_chunks", "n_complete", "last_chunk", "reserved")
STRSPU_SECTOR = 2048
STRSPU_MAX_CHUNKS = (2 ** 31 - 1) // 126


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
    L.psxhip_strspu_demux_device.argtypes = [vp, C.POINTER(StrSettings), i32, vp, sz, i32, i64, i32, vp, sz, sz, vp, vp, vp, i32, sz, vp, vp, vp,
                                             vp, vp]
    L.psxhip_spu_deinterleave_device.argtypes = [i32, vp, i32, sz, sz, sz, i32, vp, i32, sz, vp, sz, vp]
    L.psxhip_strspu_read_host.argtypes = [vp, C.POINTER(StrSettings), vp, i32, i64, i32, vp, vp, vp, vp, i64, vp, vp, vp]
    L.psxhip_strspu_demux_kernel_rev.restype = C.c_char_p
    L._psxhip_str_demux_bound = True
    return L


def kernel_rev():
    return _bind().psxhip_str_demux_kernel_rev().decode()


def strspu_demux_kernel_rev():
    return _bind().psxhip_strspu_demux_kernel_rev().decode()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _out(t, stream, dev, shape, dtype, padded=False):
    """An output tensor of a device call: a new zeroed one on the stream when t is None, else t held to shape and dtype -- contiguous,
    or, for the tensors whose stride over streams may be padded, with rows that lie back to back within a stream."""
    if t is None:
        return _lib.new_tensor(stream, dev, shape, dtype, 0)
    assert t.dtype == dtype and tuple(t.shape) == tuple(shape), (t.dtype, tuple(t.shape), shape)
    if padded:
        assert t.stride(2) == 1 and (shape[1] == 0 or t.stride(1) == shape[2]), "rows lie back to back: a row's pitch is its length"
    else:
        assert t.is_contiguous()
    return t


def _sectors_3d(d_sectors, ssz):
    """the sectors of a device call as (S, n_sectors, sector size): one stream may come without its first dimension"""
    assert torch is not None and d_sectors.is_cuda and d_sectors.dtype == torch.uint8
    if d_sectors.dim() == 2:
        d_sectors = d_sectors.unsqueeze(0)
    n = d_sectors.shape[1]
    assert d_sectors.shape[2] == ssz and d_sectors.stride(2) == 1 and (n == 0 or d_sectors.stride(1) == ssz)
    return d_sectors, d_sectors.shape[0], n


def _host_arrays(s, sectors, ssz, max_frames, frames, want_frames):
    """what both host readers take and fill: the sectors as (n, sector size), then frames (the caller's, zeros, or None), info,
    decoded, summary"""
    sectors = np.ascontiguousarray(sectors, dtype=np.uint8).reshape(-1, ssz)
    frame_bytes = s.video_width * s.video_height * 3 // 2
    if want_frames and frames is None:
        frames = np.zeros((max_frames, frame_bytes), np.uint8)
    if frames is not None:
        assert frames.dtype == np.uint8 and frames.flags.c_contiguous and frames.shape == (max_frames, frame_bytes)
    return sectors, frames, np.zeros((max_frames, 8), np.int32), np.zeros((max_frames, 4), np.int32), np.zeros(8, np.int32)


def spu_deinterleave_device(d_in, lane_bytes, channels, lane_offset=0, d_src_chunk=None, n_chunks=None, d_units=None, stream=None):
    """psxhip_spu_deinterleave_device.  d_in: uint8 CUDA tensor (S, chunks, chunk_stride), or (chunks, chunk_stride) for one stream; its
    strides over streams and chunks may be padded.  Chunk k is row d_src_chunk[k] of d_in (int32 CUDA tensor (n_chunks,), a negative
    entry skips the chunk; None: row k, n_chunks of them -- all when None).  Returns d_units (S, n_chunks * channels * lane_bytes / 16,
    16) uint8 (zeroed when not given): block b of lane c of chunk k at record (k B + b) * channels + c; asynchronous on the stream."""
    assert torch is not None and d_in.is_cuda and d_in.dtype == torch.uint8
    if d_in.dim() == 2:
        d_in = d_in.unsqueeze(0)
    S = d_in.shape[0]
    assert d_in.stride(2) == 1
    if n_chunks is None:
        n_chunks = d_in.shape[1] if d_src_chunk is None else d_src_chunk.shape[0]
    if d_src_chunk is not None:
        assert d_src_chunk.dtype == torch.int32 and d_src_chunk.is_contiguous() and d_src_chunk.shape[0] >= n_chunks
    records = n_chunks * channels * (lane_bytes // 16)
    if d_units is None:
        d_units = _lib.new_tensor(stream, d_in.device, (S, records, 16), torch.uint8, 0)
    assert d_units.dtype == torch.uint8 and tuple(d_units.shape) == (S, records, 16) and d_units.stride(2) == 1
    assert records == 0 or d_units.stride(1) == 16
    st = _lib.launch_stream(stream, d_in.device)
    _lib.check(_bind().psxhip_spu_deinterleave_device(
        d_in.device.index or 0, d_in.data_ptr(), n_chunks, d_in.stride(1), lane_offset, lane_bytes, channels, _ptr(d_src_chunk), S,
        d_in.stride(0) if S > 1 else 0, d_units.data_ptr(), d_units.stride(0) if S > 1 else 0, st.cuda_stream))
    return d_units


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
        ssz = SECTOR_SIZE[s.format]
        d_sectors, S, n = _sectors_3d(d_sectors, ssz)
        dev = d_sectors.device
        if xa_capacity is None:
            xa_capacity = n
        # a row's pitch is bs_stride: room behind the last whole chunk is the row's margin
        d_bs = _out(d_bs, stream, dev, (S, max_frames, bs_stride), torch.uint8, padded=True)
        d_sizes = _out(d_sizes, stream, dev, (S, max_frames), torch.int32)
        d_info = _out(d_info, stream, dev, (S, max_frames, 8), torch.int32)
        d_xa = _out(d_xa, stream, dev, (S, xa_capacity, ssz), torch.uint8, padded=True)
        if d_table is not None or table:
            d_table = _out(d_table, stream, dev, (S, n, 4), torch.int32)
        d_summary = _out(d_summary, stream, dev, (S, 8), torch.int32)
        st = _lib.launch_stream(stream, dev)
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
        sectors, frames, info, decoded, summary = _host_arrays(s, sectors, SECTOR_SIZE[s.format], max_frames, frames, want_frames)
        n = sectors.shape[0]
        per_sector = 4032 if s.audio_bit_depth == 4 else 2016
        cap = n if pcm_sectors is None else int(pcm_sectors)
        pcm = np.zeros(max(cap, 1) * per_sector, np.int16)
        xa_status = np.zeros(max(cap, 1), np.int32)
        rc = _bind().psxhip_str_read_host(self._h, C.byref(s), sectors.ctypes.data if n else None, n, int(first_frame), max_frames,
                                          frames.ctypes.data if frames is not None else None, info.ctypes.data, decoded.ctypes.data, pcm.ctypes.data if cap else None, cap * per_sector, xa_status.ctypes.data,
                                          summary.ctypes.data)
        if rc < 0:
            _lib.check(rc)
        ch = max(1, s.audio_channels)
        return dict(frames=frames, info=info, decoded=decoded, pcm=pcm[:rc * ch], xa_status=xa_status[:rc * ch // per_sector],
                    summary=summary)

    def demux_strspu_device(self, s, d_sectors, max_frames, bs_stride, first_frame=-1, audio_capacity=None, d_bs=None, d_sizes=None,
                            d_info=None, d_units=None, d_chunk_info=None, d_table=None, d_summary=None, d_audio_summary=None, table=True,
                            stream=None):
        """psxhip_strspu_demux_device.  d_sectors: uint8 CUDA tensor (S, n_sectors, 2048), or (n_sectors, 2048) for one stream; its stride
        over streams may be padded.  Outputs (allocated, zeroed, when not given; given d_bs / d_units may have padded strides over
        streams): d_bs, d_sizes, d_info, d_table, d_summary as demux_device's; d_units (S, audio_capacity * 126, 16) uint8
        (audio_capacity None: n_sectors), d_chunk_info (S, audio_capacity, 8) int32 [CHUNK_FIELDS], d_audio_summary (S, 4) int32
        [AUDIO_SUMMARY_FIELDS].  Returns a dict of those tensors under the names bs, sizes, info, units, chunk_info, table, summary,
        audio_summary; asynchronous on the stream."""
        d_sectors, S, n = _sectors_3d(d_sectors, STRSPU_SECTOR)
        dev = d_sectors.device
        if audio_capacity is None:
            audio_capacity = n
        d_bs = _out(d_bs, stream, dev, (S, max_frames, bs_stride), torch.uint8, padded=True)
        d_sizes = _out(d_sizes, stream, dev, (S, max_frames), torch.int32)
        d_info = _out(d_info, stream, dev, (S, max_frames, 8), torch.int32)
        d_units = _out(d_units, stream, dev, (S, audio_capacity * 126, 16), torch.uint8, padded=True)
        d_chunk_info = _out(d_chunk_info, stream, dev, (S, audio_capacity, 8), torch.int32)
        if d_table is not None or table:
            d_table = _out(d_table, stream, dev, (S, n, 4), torch.int32)
        d_summary = _out(d_summary, stream, dev, (S, 8), torch.int32)
        d_audio_summary = _out(d_audio_summary, stream, dev, (S, 4), torch.int32)
        st = _lib.launch_stream(stream, dev)
        _lib.check(_bind().psxhip_strspu_demux_device(
            self._h, C.byref(s), S, d_sectors.data_ptr(), d_sectors.stride(0) if S > 1 else 0, n, int(first_frame), max_frames,
            d_bs.data_ptr(), bs_stride, d_bs.stride(0) if S > 1 else 0, d_sizes.data_ptr(), d_info.data_ptr(),
            d_units.data_ptr() if audio_capacity else None, audio_capacity, d_units.stride(0) if S > 1 else 0,
            d_chunk_info.data_ptr() if audio_capacity else None, _ptr(d_table), d_summary.data_ptr(), d_audio_summary.data_ptr(),
            st.cuda_stream))
        return dict(bs=d_bs, sizes=d_sizes, info=d_info, units=d_units, chunk_info=d_chunk_info, table=d_table, summary=d_summary,
                    audio_summary=d_audio_summary)

    def read_strspu(self, s, sectors, max_frames, first_frame=-1, frames=None, pcm_capacity=None, want_frames=True):
        """psxhip_strspu_read_host: one STRSPU stream in host memory.  sectors: (n_sectors, 2048) uint8.  frames / want_frames: as read().
        pcm_capacity: int16 elements of room for PCM (None: room for a chunk per sector; 0: no audio, pcm NULL).  Returns dict(frames,
        info, decoded as read()'s, pcm int16 (interleaved L,R when stereo), chunk_info (chunks taken apart, 8) int32 [CHUNK_FIELDS],
        summary (8,) int32 [SUMMARY_FIELDS], audio_summary (4,) int32 [AUDIO_SUMMARY_FIELDS])."""
        sectors, frames, info, decoded, summary = _host_arrays(s, sectors, STRSPU_SECTOR, max_frames, frames, want_frames)
        n = sectors.shape[0]
        audio_summary = np.zeros(4, np.int32)
        ch = s.audio_channels
        cap = n * 126 * 28 if pcm_capacity is None else int(pcm_capacity)
        pcm = np.zeros(max(cap, 1), np.int16)
        # the chunk records the library writes: the chunks the PCM buffer holds (reader_plan.cpp: strspu_read_capacity)
        d = 0 if s.strspu_options & 0x20000 else 1
        held = min(n, (cap // (28 * ch) + d) // (126 // ch), STRSPU_MAX_CHUNKS // 28) if ch and cap else 0
        chunk_info = np.zeros((max(held, 1), 8), np.int32)
        rc = _bind().psxhip_strspu_read_host(self._h, C.byref(s), sectors.ctypes.data if n else None, n, int(first_frame), max_frames,
                                             frames.ctypes.data if frames is not None else None, info.ctypes.data, decoded.ctypes.data, pcm.ctypes.data if cap else None, cap, chunk_info.ctypes.data,
                                             summary.ctypes.data, audio_summary.ctypes.data)
        if rc < 0:
            _lib.check(rc)
        return dict(frames=frames, info=info, decoded=decoded, pcm=pcm[:rc * max(1, ch)], chunk_info=chunk_info[:held], summary=summary,
                    audio_summary=audio_summary)
