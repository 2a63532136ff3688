"""Disc reader -- Python mirror of the disc reader section of include/psxav_hip.h.

``disc_read`` takes a raw image of 2352-byte sectors in HBM apart: damaged form-1 sectors are repaired from their P / Q parity, every
sector is routed to a track by file number, channel number and submode, and every track's sectors are written compacted in image
order, in the sector size ``StrReader.demux_device`` and ``xa_disassemble`` read.  ``disc_read_host`` is the same for an image in
host memory.  The rules are "psxhip disc read v1" (DESIGN.md section 17).
"""
import ctypes as C

import numpy as np

from . import _lib

try:  # torch is plumbing (device memory, streams); disc_read_host works on numpy arrays
    import torch
except Exception:  # pragma: no cover
    torch = None

MAX_TRACKS = 64
REPAIRED, UNREPAIRABLE, EDC, EDC_ABSENT, SYNC, SUBHEADER, EMPTY, UNCLAIMED, DROPPED, FORM = (1 << k for k in range(10))
# the int32 columns of psxhip_disc_read_sector_t
SECTOR_FIELDS = ("track", "ordinal", "status", "corrections")
# psxhip_disc_read_summary_t: fourteen int32, then n_corrections (int64)
SUMMARY_FIELDS = ("n_sectors", "n_form1", "n_form2", "n_clean", "n_repaired", "n_unrepairable", "n_edc", "n_edc_absent", "n_sync",
                  "n_subheader", "n_empty", "n_unclaimed", "n_dropped", "reserved", "n_corrections")


class DiscTrack(C.Structure):
    """psxhip_disc_track_t"""
    _fields_ = [("sectors", C.c_void_p), ("stride", C.c_int64), ("capacity", C.c_int32), ("sector_size", C.c_int32),
                ("file_number", C.c_int32), ("channel_number", C.c_int32), ("submode_mask", C.c_uint8), ("submode_value", C.c_uint8),
                ("reserved", C.c_uint8 * 6)]


class DiscReadSummary(C.Structure):
    """psxhip_disc_read_summary_t"""
    _fields_ = [(name, C.c_int32) for name in SUMMARY_FIELDS[:14]] + [("n_corrections", C.c_int64)]


def _bind():
    L = _lib.lib()
    if getattr(L, "_psxhip_disc_read_bound", False):
        return L
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.psxhip_disc_reader_create.argtypes = [C.POINTER(vp), i32]
    L.psxhip_disc_reader_destroy.argtypes = [vp]
    L.psxhip_disc_reader_destroy.restype = None
    L.psxhip_disc_read_device.argtypes = [vp, vp, i64, C.POINTER(DiscTrack), i32, vp, vp, vp, vp]
    L.psxhip_disc_read_host.argtypes = [vp, vp, i64, C.POINTER(DiscTrack), i32, vp, vp, vp]
    L.psxhip_disc_read_kernel_rev.restype = C.c_char_p
    L._psxhip_disc_read_bound = True
    return L


def kernel_rev():
    return _bind().psxhip_disc_read_kernel_rev().decode()


def track(sectors, size=None, file=-1, channel=-1, mask=0, value=0, capacity=None):
    """One track: `sectors` is a 2-D uint8 array or CUDA tensor the track's sectors are written into, one slot per row, unit stride
    along the row; its row pitch is the stride, `size` (default: the row length) the sector size, `capacity` (default: the rows) the
    slots.  A sector belongs to the track when its file number is `file` (-1: any), its channel number `channel` (-1: any) and
    (submode & mask) == value.  Returns (psxhip_disc_track_t, sectors): keep the second alive as long as the first is used."""
    n, width = int(sectors.shape[0]), int(sectors.shape[1])
    size = width if size is None else int(size)
    capacity = n if capacity is None else int(capacity)
    assert capacity <= n
    if torch is not None and isinstance(sectors, torch.Tensor):
        assert sectors.dtype == torch.uint8 and (n == 0 or sectors.stride(1) == 1)
        ptr, pitch = sectors.data_ptr(), sectors.stride(0) if n > 1 else max(width, size)
    else:
        assert sectors.dtype == np.uint8 and (n == 0 or sectors.strides[1] == 1)
        ptr, pitch = sectors.ctypes.data, sectors.strides[0] if n > 1 else max(width, size)
    t = DiscTrack()
    t.sectors = ptr if n else None
    t.stride = pitch
    t.capacity = capacity
    t.sector_size = size
    t.file_number = int(file)
    t.channel_number = int(channel)
    t.submode_mask = int(mask)
    t.submode_value = int(value)
    return t, sectors


def _table(tracks):
    arr = (DiscTrack * max(1, len(tracks)))()
    for i, (t, _) in enumerate(tracks):
        arr[i] = t
    return arr


def summary_dict(words):
    """psxhip_disc_read_summary_t as 16 int32 (a tensor's or an array's list) -> dict of SUMMARY_FIELDS"""
    words = [int(v) for v in words]
    d = dict(zip(SUMMARY_FIELDS[:14], words[:14]))
    d["n_corrections"] = (words[14] & 0xFFFFFFFF) | (words[15] << 32)
    return d


class DiscReader:
    """psxhip_disc_reader_t: owns the workspace; calls on one handle are stream-ordered."""

    def __init__(self, device=0):
        self.device = int(device)
        self._h = C.c_void_p()
        _lib.check(_bind().psxhip_disc_reader_create(C.byref(self._h), self.device))

    def close(self):
        if self._h:
            _bind().psxhip_disc_reader_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def read_device(self, d_image, tracks, table=True, stream=None):
        """psxhip_disc_read_device.  d_image: (n, 2352) uint8 CUDA tensor; tracks: a list of track(...) results over CUDA tensors.
        Returns dict(table (n, 4) int32 [SECTOR_FIELDS] or None, counts (len(tracks),) int32, summary (16,) int32 [summary_dict]);
        asynchronous on the stream."""
        assert torch is not None and d_image.is_cuda and d_image.dtype == torch.uint8 and d_image.is_contiguous()
        n = d_image.numel() // 2352
        dev = d_image.device
        d_table = _lib.new_tensor(stream, dev, (n, 4), torch.int32, 0) if table else None
        d_counts = _lib.new_tensor(stream, dev, (max(1, len(tracks)),), torch.int32, 0)
        d_summary = _lib.new_tensor(stream, dev, (16,), torch.int32, 0)
        st = _lib.launch_stream(stream, dev)
        _lib.check(_bind().psxhip_disc_read_device(self._h, d_image.data_ptr() if n else None, n, _table(tracks), len(tracks),
                                                   d_table.data_ptr() if table and n else None, d_counts.data_ptr(), d_summary.data_ptr(),
                                                   st.cuda_stream))
        return dict(table=d_table, counts=d_counts[:len(tracks)], summary=d_summary)

    def read_host(self, image, tracks, table=True):
        """psxhip_disc_read_host.  image: (n, 2352) uint8 array; tracks: a list of track(...) results over numpy arrays, which are
        written in place.  Returns dict(table (n, 4) int32 or None, counts (len(tracks),) int32, summary dict)."""
        image = np.ascontiguousarray(image, dtype=np.uint8).reshape(-1, 2352)
        n = image.shape[0]
        tab = np.zeros((n, 4), np.int32) if table else None
        counts = np.zeros(max(1, len(tracks)), np.int32)
        summary = np.zeros(16, np.int32)
        _lib.check(_bind().psxhip_disc_read_host(self._h, image.ctypes.data if n else None, n, _table(tracks), len(tracks),
                                                 tab.ctypes.data if table and n else None, counts.ctypes.data, summary.ctypes.data))
        return dict(table=tab, counts=counts[:len(tracks)], summary=summary_dict(summary.tolist()))


def disc_read(d_image, tracks, reader=None, table=True, stream=None):
    """DiscReader.read_device on `reader`, or on a handle made for this call (then the call waits for the stream: the handle's
    workspace goes with it)."""
    if reader is not None:
        return reader.read_device(d_image, tracks, table, stream)
    r = DiscReader(d_image.device.index or 0)
    try:
        out = r.read_device(d_image, tracks, table, stream)
        _lib.launch_stream(stream, d_image.device).synchronize()
        return out
    finally:
        r.close()


def disc_read_host(image, tracks, device=0, table=True):
    """DiscReader.read_host on a handle made for this call"""
    r = DiscReader(device)
    try:
        return r.read_host(image, tracks, table)
    finally:
        r.close()
