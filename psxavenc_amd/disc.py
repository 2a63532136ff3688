"""Disc finisher -- Python mirror of the disc finisher section of include/psxav_hip.h.

``disc_finish`` turns sectors as the encoders leave them (``xa`` / ``xacd`` / ``str`` / ``strcd`` / ``strv`` buffers in HBM) into an
interleaved image of raw 2352-byte Mode 2 sectors a drive can read: sync, absolute BCD header, both subheader copies, EDC and, for
form 1, P and Q parity.  ``disc_check`` is the inverse statement: status bits per sector and a summary.  ``disc_plan`` sizes the image
and needs no device.  The rules are "psxhip disc finish v1" / "psxhip disc check v1" (DESIGN.md section 14).
"""
import ctypes as C

import numpy as np

from . import _lib

try:  # torch is plumbing (device memory, streams); disc_plan and disc_finish_host work without it
    import torch
except Exception:  # pragma: no cover
    torch = None

MAX_SOURCES = MAX_PERIOD = 64
LBA_LIMIT = 450000
SYNC, HEADER, SUBHEADER, EDC, ECC_P, ECC_Q, EDC_ABSENT = 1, 2, 4, 8, 16, 32, 64
# the int32 fields of psxhip_disc_summary_t
SUMMARY_FIELDS = ("n_sectors", "n_form1", "n_form2", "n_bad", "n_sync", "n_header", "n_subheader", "n_edc", "n_ecc_p", "n_ecc_q",
                  "n_edc_absent", "reserved")


class DiscSource(C.Structure):
    """psxhip_disc_source_t"""
    _fields_ = [("sectors", C.c_void_p), ("stride", C.c_int64), ("n_sectors", C.c_int32), ("sector_size", C.c_int32),
                ("file_number", C.c_int32), ("channel_number", C.c_int32), ("data_subheader", C.c_uint8 * 4), ("reserved", C.c_int32)]


class DiscLayout(C.Structure):
    """psxhip_disc_layout_t"""
    _fields_ = [("period", C.c_int32), ("start_lba", C.c_int32), ("slot_source", C.c_int32 * MAX_PERIOD)]


def _bind():
    L = _lib.lib()
    if getattr(L, "_psxhip_disc_bound", False):
        return L
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.psxhip_disc_plan.argtypes = [C.POINTER(DiscLayout), C.POINTER(DiscSource), i32]
    L.psxhip_disc_plan.restype = i64
    L.psxhip_disc_finish_device.argtypes = [i32, C.POINTER(DiscLayout), C.POINTER(DiscSource), i32, vp, i64, i64, vp]
    L.psxhip_disc_check_device.argtypes = [i32, vp, i64, i64, vp, vp, vp]
    L.psxhip_disc_finish_host.argtypes = [i32, C.POINTER(DiscLayout), C.POINTER(DiscSource), i32, vp, i64, i64]
    L.psxhip_disc_kernel_rev.restype = C.c_char_p
    L._psxhip_disc_bound = True
    return L


def kernel_rev():
    return _bind().psxhip_disc_kernel_rev().decode()


def layout(slot_source, start_lba=0):
    """psxhip_disc_layout_t from the period's slot list (a source index, or -1 for a gap, per slot)"""
    lay = DiscLayout()
    lay.period = len(slot_source)
    lay.start_lba = int(start_lba)
    for q, s in enumerate(list(slot_source)[:MAX_PERIOD]):
        lay.slot_source[q] = int(s)
    return lay


def source(sectors, size=None, file=-1, channel=-1, data_subheader=(0, 0, 0x08, 0)):
    """One source: `sectors` is a 2-D uint8 array or CUDA tensor, one sector per row, unit stride along the row; its row pitch is the
    stride, `size` (default: the row length) the sector size -- a row longer than `size` carries junk the finisher never reads.  Returns
    (psxhip_disc_source_t, sectors): keep the second alive as long as the first is used."""
    n, width = int(sectors.shape[0]), int(sectors.shape[1])
    size = width if size is None else int(size)
    if torch is not None and isinstance(sectors, torch.Tensor):
        assert sectors.dtype == torch.uint8 and (n == 0 or sectors.stride(1) == 1)
        ptr, pitch = sectors.data_ptr(), sectors.stride(0) if n > 1 else max(width, size)
    else:
        assert sectors.dtype == np.uint8 and (n == 0 or sectors.strides[1] == 1)
        ptr, pitch = sectors.ctypes.data, sectors.strides[0] if n > 1 else max(width, size)
    s = DiscSource()
    s.sectors = ptr if n else None
    s.stride = pitch
    s.n_sectors = n
    s.sector_size = size
    s.file_number = int(file)
    s.channel_number = int(channel)
    for i in range(4):
        s.data_subheader[i] = int(data_subheader[i])
    return s, sectors


def _table(sources):
    arr = (DiscSource * max(1, len(sources)))()
    for i, (s, _) in enumerate(sources):
        arr[i] = s
    return arr


def disc_plan(lay, sources):
    """psxhip_disc_plan: sectors of the whole schedule.  sources: a list of source(...) results."""
    n = _bind().psxhip_disc_plan(C.byref(lay), _table(sources), len(sources))
    if n < 0:
        _lib.check(int(n))
    return int(n)


def disc_finish(lay, sources, first_out=0, n_out=None, d_out=None, device=0, stream=None):
    """psxhip_disc_finish_device: sectors first_out .. first_out + n_out - 1 of the schedule (n_out None: to its end) into d_out, a
    (n_out, 2352) uint8 CUDA tensor (allocated when not given).  Asynchronous on the stream; returns d_out."""
    assert torch is not None
    if n_out is None:
        n_out = disc_plan(lay, sources) - first_out
    dev = torch.device("cuda", device)
    if d_out is None:
        d_out = _lib.new_tensor(stream, dev, (max(n_out, 0), 2352), torch.uint8)
    assert d_out.is_cuda and d_out.dtype == torch.uint8 and d_out.is_contiguous() and d_out.numel() >= n_out * 2352
    st = _lib.launch_stream(stream, dev)
    _lib.check(_bind().psxhip_disc_finish_device(device, C.byref(lay), _table(sources), len(sources), d_out.data_ptr(), first_out, n_out,
                                                 st.cuda_stream))
    return d_out


def disc_check(d_image, start_lba=-1, status=True, stream=None):
    """psxhip_disc_check_device over a (n, 2352) uint8 CUDA tensor.  Returns (d_status int32 (n,) or None, d_summary int32 (12,)
    [SUMMARY_FIELDS]); asynchronous on the stream."""
    assert torch is not None and d_image.is_cuda and d_image.dtype == torch.uint8 and d_image.is_contiguous()
    n = d_image.numel() // 2352
    dev = d_image.device
    d_status = _lib.new_tensor(stream, dev, (n,), torch.int32, 0) if status else None
    d_summary = _lib.new_tensor(stream, dev, (12,), torch.int32, 0)
    st = _lib.launch_stream(stream, dev)
    _lib.check(_bind().psxhip_disc_check_device(dev.index or 0, d_image.data_ptr() if n else None, n, int(start_lba),
                                                d_status.data_ptr() if status else None, d_summary.data_ptr(), st.cuda_stream))
    return d_status, d_summary


def disc_finish_host(lay, sources, first_out=0, n_out=None, device=0):
    """psxhip_disc_finish_host: sources are numpy arrays in host memory; returns the image as a (n_out, 2352) uint8 array."""
    if n_out is None:
        n_out = disc_plan(lay, sources) - first_out
    out = np.zeros((max(n_out, 0), 2352), np.uint8)
    _lib.check(_bind().psxhip_disc_finish_host(device, C.byref(lay), _table(sources), len(sources), out.ctypes.data, first_out, n_out))
    return out
