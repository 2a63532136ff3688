"""SPU / VAG sound banks -- Python mirror of psxhip_spu_bank_* (include/psxav_hip.h; "psxhip SPU bank v1").

Many mono samples of different lengths, rates, loop points and names, encoded by one call into one device buffer of SPU or VAG
files (each byte for byte what ``spufile.encode`` gives for that sample), and the way back: a check of the framing per entry and a
decode of every entry's blocks into the entries' own PCM layout, with the sums an SNR per entry is made of.
"""
import ctypes as C

import numpy as np

from . import _lib
from .adpcm_decode import snr_db as _snr_db
from .spufile import FORMAT_SPU, FORMAT_VAG  # noqa: F401

try:  # torch is plumbing (device memory, streams); plan() and encode_host() work without it
    import torch
except Exception:  # pragma: no cover
    torch = None

STATUS_HEADER, STATUS_DUMMY, STATUS_FLAGS, STATUS_TRAP, STATUS_PADDING = 1, 2, 4, 8, 16
# "psxhip SPU loop seam v1" 
SEAM_OFF, SEAM_STEADY, SEAM_PASSES = 0, 1, 8


class SpuBankSettings(C.Structure):
    """psxhip_spu_bank_settings_t"""
    _fields_ = [("format", C.c_int32), ("alignment", C.c_int32), ("no_leading_dummy", C.c_int32), ("bank_alignment", C.c_int32),
                ("beam", C.c_int32)]


class SpuBankEntry(C.Structure):
    """psxhip_spu_bank_entry_t"""
    _fields_ = [("pcm_offset", C.c_int64), ("samples", C.c_int64), ("audio_frequency", C.c_int32), ("audio_loop_point", C.c_int32),
                ("enable_loop", C.c_int32), ("name", C.c_char * 16)]


class SpuSeam(C.Structure):
    """psxhip_spu_seam_t"""
    _fields_ = [("seam_block", C.c_int32), ("first_units", C.c_int32), ("first_peak", C.c_int32), ("settled", C.c_int32),
                ("first_sse", C.c_uint64), ("pass1_err", C.c_uint64), ("pass2_err", C.c_uint64)]


# the same record as a numpy dtype: what SpuBank.seam_report returns
SEAM_DTYPE = np.dtype([("seam_block", "<i4"), ("first_units", "<i4"), ("first_peak", "<i4"), ("settled", "<i4"), ("first_sse", "<u8"),
                       ("pass1_err", "<u8"), ("pass2_err", "<u8")])


def settings(fmt, alignment=64, no_dummy=False, bank_alignment=16, beam=0):
    return SpuBankSettings(fmt, alignment, int(no_dummy), bank_alignment, beam)


def entry(pcm_offset, samples, freq=44100, loop_point=-1, enable_loop=False, name=""):
    return SpuBankEntry(pcm_offset, samples, freq, loop_point, int(enable_loop), name.encode()[:16])


def _bind():
    L = _lib.lib()
    if getattr(L, "_psxhip_spu_bank_bound", False):
        return L
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.psxhip_spu_bank_plan.argtypes = [C.POINTER(SpuBankSettings), C.POINTER(SpuBankEntry), i32, vp, vp, vp]
    L.psxhip_spu_bank_create.argtypes = [C.POINTER(vp), i32, C.POINTER(SpuBankSettings), C.POINTER(SpuBankEntry), i32]
    L.psxhip_spu_bank_destroy.argtypes = [vp]
    L.psxhip_spu_bank_destroy.restype = None
    L.psxhip_spu_bank_total_bytes.argtypes = [vp]
    L.psxhip_spu_bank_total_bytes.restype = i64
    L.psxhip_spu_bank_layout.argtypes = [vp, vp, vp]
    L.psxhip_spu_bank_encode_device.argtypes = [vp, vp, vp, vp]
    L.psxhip_spu_bank_encode_host.argtypes = [vp, vp, i64, vp, C.c_size_t]
    L.psxhip_spu_bank_encode_host.restype = i64
    L.psxhip_spu_bank_check_device.argtypes = [vp, vp, vp, vp]
    L.psxhip_spu_bank_decode_device.argtypes = [vp, vp, vp, vp, vp, vp]
    L.psxhip_spu_bank_kernel_rev.restype = C.c_char_p
    L.psxhip_spu_bank_set_seam.argtypes = [vp, i32]
    L.psxhip_spu_bank_seam_passes_device.argtypes = [vp, vp, vp]
    L.psxhip_spu_bank_seam_device.argtypes = [vp, vp, vp, vp, vp]
    L.psxhip_spu_seam_kernel_rev.restype = C.c_char_p
    L._psxhip_spu_bank_bound = True
    return L


def kernel_rev():
    return _bind().psxhip_spu_bank_kernel_rev().decode()


def seam_kernel_rev():
    return _bind().psxhip_spu_seam_kernel_rev().decode()


def _entry_array(entries):
    entries = list(entries)
    return (SpuBankEntry * max(len(entries), 1))(*entries), len(entries)


def plan(s, entries):
    """psxhip_spu_bank_plan: (offsets, sizes, total) of the bank these settings and entries make.  Needs no device."""
    arr, n = _entry_array(entries)
    offsets, sizes, total = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64), C.c_int64(0)
    _lib.check(_bind().psxhip_spu_bank_plan(C.byref(s), arr, n, offsets.ctypes.data, sizes.ctypes.data, C.addressof(total)))
    return offsets[:n], sizes[:n], int(total.value)


class SpuBank:
    """A bank context: the plan and its device tables.  Its calls share those tables: one call of a context at a time."""

    def __init__(self, s, entries, device=0):
        L = _bind()
        arr, n = _entry_array(entries)
        self.device = torch.device("cuda", device) if torch is not None and isinstance(device, int) else device
        self._h = C.c_void_p()
        _lib.check(L.psxhip_spu_bank_create(C.byref(self._h), device if isinstance(device, int) else (device.index or 0), C.byref(s), arr, n))
        self.n = n
        self.total = int(L.psxhip_spu_bank_total_bytes(self._h))
        self.pcm_elements = max([e.pcm_offset + e.samples for e in list(arr)[:n]] + [0])

    def close(self):
        if self._h:
            _bind().psxhip_spu_bank_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def layout(self):
        """(offsets, sizes) of the files, int64 arrays in entry order, and the bank's bytes"""
        offsets, sizes = np.zeros(self.n, np.int64), np.zeros(self.n, np.int64)
        _lib.check(_bind().psxhip_spu_bank_layout(self._h, offsets.ctypes.data, sizes.ctypes.data))
        return offsets, sizes, self.total

    def encode_device(self, d_pcm, d_out=None, stream=None):
        """d_pcm: int16 CUDA tensor holding every entry's samples at its pcm_offset.  Returns d_out, a uint8 CUDA tensor whose first
        `total` bytes are the bank (a new tensor of that size when None).  Asynchronous on the stream unless an entry is long enough
        for the chunked encoder (include/psxav_hip.h)."""
        if d_out is None:
            d_out = _lib.new_tensor(stream, d_pcm.device, (max(self.total, 16),), torch.uint8)
        assert d_pcm.dtype == torch.int16 and d_pcm.is_contiguous() and d_pcm.numel() >= self.pcm_elements
        assert d_out.dtype == torch.uint8 and d_out.is_contiguous() and d_out.numel() >= self.total
        _lib.check(_bind().psxhip_spu_bank_encode_device(self._h, d_pcm.data_ptr(), d_out.data_ptr(),
                                                         _lib.launch_stream(stream, d_pcm.device).cuda_stream))
        return d_out

    def encode_host(self, pcm):
        """pcm: int16 array holding every entry's samples at its pcm_offset.  Returns the bank's bytes (uint8 array)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        out = np.zeros(max(self.total, 1), np.uint8)
        rc = _bind().psxhip_spu_bank_encode_host(self._h, pcm.ctypes.data if pcm.size else None, pcm.size, out.ctypes.data, out.size)
        if rc < 0:
            _lib.check(int(rc))
        assert rc == self.total
        return out[:self.total]

    def check_device(self, d_bank, stream=None):
        """The framing of the bank in the uint8 CUDA tensor d_bank, per entry: an int32 CUDA tensor (n,) of STATUS_* bits, all zero for
        a bank this library wrote.  Asynchronous."""
        assert d_bank.dtype == torch.uint8 and d_bank.is_contiguous() and d_bank.numel() >= self.total
        d_status = _lib.new_tensor(stream, d_bank.device, (self.n,), torch.int32)
        _lib.check(_bind().psxhip_spu_bank_check_device(self._h, d_bank.data_ptr(), d_status.data_ptr(),
                                                        _lib.launch_stream(stream, d_bank.device).cuda_stream))
        return d_status

    def decode_device(self, d_bank, d_pcm_out=None, d_ref_pcm=None, stream=None):
        """Every entry's blocks back to PCM in the entries' own layout.  Returns (d_pcm_out, d_sums): d_pcm_out an int16 CUDA tensor (a
        new zeroed one of pcm_elements when None), of which only the entries' samples are stored; d_sums, with d_ref_pcm given, an
        int64 CUDA tensor (n, 2) holding the library's uint64 [sum (a - b)^2, sum b^2] per entry, else None.  Asynchronous."""
        assert d_bank.dtype == torch.uint8 and d_bank.is_contiguous() and d_bank.numel() >= self.total
        if d_pcm_out is None:
            d_pcm_out = _lib.new_tensor(stream, d_bank.device, (max(self.pcm_elements, 1),), torch.int16, 0)
        assert d_pcm_out.dtype == torch.int16 and d_pcm_out.is_contiguous() and d_pcm_out.numel() >= self.pcm_elements
        d_sums = None
        if d_ref_pcm is not None:
            assert d_ref_pcm.dtype == torch.int16 and d_ref_pcm.is_contiguous() and d_ref_pcm.numel() >= self.pcm_elements
            d_sums = _lib.new_tensor(stream, d_bank.device, (self.n, 2), torch.int64, 0)
        _lib.check(_bind().psxhip_spu_bank_decode_device(self._h, d_bank.data_ptr(), d_pcm_out.data_ptr(),
                                                         d_ref_pcm.data_ptr() if d_ref_pcm is not None else None,
                                                         d_sums.data_ptr() if d_sums is not None else None,
                                                         _lib.launch_stream(stream, d_bank.device).cuda_stream))
        return d_pcm_out, d_sums

    def set_seam(self, mode):
        """SEAM_OFF (the default) or SEAM_STEADY: how the encodes that follow treat the loop seams (include/psxav_hip.h)"""
        _lib.check(_bind().psxhip_spu_bank_set_seam(self._h, int(mode)))

    def seam_passes(self, stream=None):
        """The last encode's outcome per entry under SEAM_STEADY: an int32 CUDA tensor (n,), -1 = no seam block, k = fixed at pass k,
        SEAM_PASSES = no fixed point (pass 0 kept).  Asynchronous."""
        d_pass = _lib.new_tensor(stream, self.device, (self.n,), torch.int32)
        _lib.check(_bind().psxhip_spu_bank_seam_passes_device(self._h, d_pass.data_ptr(), _lib.launch_stream(stream, self.device).cuda_stream))
        return d_pass

    def seam_report(self, d_bank, d_ref_pcm=None, stream=None):
        """The loop seams of the bank in the uint8 CUDA tensor d_bank, judged from its bytes (and, with d_ref_pcm, against the entries'
        PCM): a uint8 CUDA tensor (n, 40) of psxhip_spu_seam_t; ``seam_records`` turns it into a numpy record array.  Asynchronous."""
        assert d_bank.dtype == torch.uint8 and d_bank.is_contiguous() and d_bank.numel() >= self.total
        if d_ref_pcm is not None:
            assert d_ref_pcm.dtype == torch.int16 and d_ref_pcm.is_contiguous() and d_ref_pcm.numel() >= self.pcm_elements
        d_seam = _lib.new_tensor(stream, d_bank.device, (self.n, C.sizeof(SpuSeam)), torch.uint8)
        _lib.check(_bind().psxhip_spu_bank_seam_device(self._h, d_bank.data_ptr(), d_ref_pcm.data_ptr() if d_ref_pcm is not None else None,
                                                       d_seam.data_ptr(), _lib.launch_stream(stream, d_bank.device).cuda_stream))
        return d_seam

    @staticmethod
    def seam_records(d_seam):
        """seam_report's tensor as a numpy record array of SEAM_DTYPE (synchronises)"""
        return d_seam.cpu().numpy().reshape(-1).view(SEAM_DTYPE)

    @staticmethod
    def snr_db(sums):
        """dB per entry from decode_device's sums (adpcm_decode.snr_db)"""
        return _snr_db(sums.cpu().numpy() if torch is not None and isinstance(sums, torch.Tensor) else sums)
