"""SPU / XA ADPCM decoder -- Python mirror of the decoder section of include/psxav_hip.h.

Unit records (the encoder's layout; a 4-bit record is an SPU block), SPU blocks or XA sectors back to int16 PCM on the device, the
sums of squared errors of two sample sets per sound unit and per chain, and ``snr_db`` for the caller's arithmetic on those sums.
The arithmetic is "psxhip ADPCM decode v1" (DESIGN.md section 12): the reconstruction inside the reference's encoder
(libpsxav/adpcm.c:120-124,135-136).
"""
import ctypes as C

import numpy as np

from . import _lib
from .adpcm import CHAIN_DTYPE, record_bytes

try:  # torch is plumbing (device memory, streams); the host-buffer paths work without it
    import torch
except Exception:  # pragma: no cover
    torch = None

FLAG_BAD_FILTER, FLAG_BAD_SHIFT = 1, 2                                         # unit flags
XA_STATUS_HEADER_COPY, XA_STATUS_SUBHEADER, XA_STATUS_CODING, XA_STATUS_EDC = 1, 2, 4, 8   # sector status bits


def _bind():
    L = _lib.lib()
    if getattr(L, "_psxhip_adpcm_decode_bound", False):
        return L
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.psxhip_adpcm_decode_chains_device.argtypes = [i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.psxhip_adpcm_decode_chains_chunked.argtypes = [i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, i32, i32, vp]
    L.psxhip_adpcm_sse_device.argtypes = [i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.psxhip_xa_disassemble_device.argtypes = [i32, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    L.psxhip_spu_decode_streams_host.argtypes = [i32, vp, i32, i64, i32, vp, vp, i64]
    L.psxhip_xa_decode_streams_host.argtypes = [i32, i32, i32, i32, i32, vp, i32, i64, i32, vp, vp, i64, vp]
    L.psxhip_adpcm_decode_kernel_rev.restype = C.c_char_p
    L.psxhip_adpcm_decode_set_timing.argtypes = [i32]
    L.psxhip_adpcm_decode_last_timing.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L._psxhip_adpcm_decode_bound = True
    return L


def kernel_rev():
    return _bind().psxhip_adpcm_decode_kernel_rev().decode()


def set_timing(on=True):
    """HIP events around the speculate launch and the verify passes of this thread's decode_chains_chunked calls"""
    _lib.check(_bind().psxhip_adpcm_decode_set_timing(1 if on else 0))


def last_timing():
    """(speculate_ms, verify_ms) of this thread's last decode_chains_chunked call with timing on"""
    a, b = C.c_float(0), C.c_float(0)
    _lib.check(_bind().psxhip_adpcm_decode_last_timing(C.byref(a), C.byref(b)))
    return float(a.value), float(b.value)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stream(dev, stream):
    return _lib.launch_stream(stream, dev).cuda_stream


def _chain_tensors(chains, unit_base, dev, stream):
    chains = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
    unit_base = np.ascontiguousarray(unit_base, dtype=np.int32)
    assert chains.size == unit_base.size
    d_chains = _lib.to_device(stream, dev, chains.view(np.uint8).reshape(chains.size, CHAIN_DTYPE.itemsize).copy())
    return chains, unit_base, d_chains, _lib.to_device(stream, dev, unit_base.copy())


def decode_chains_device(d_units, chains, unit_base, filter_count, bits, d_samples, d_states=None, d_unit_flags=None, d_tail=None,
                         stream=None):
    """psxhip_adpcm_decode_chains_device: every chain of `chains` (host CHAIN_DTYPE array) decoded serially from the uint8 CUDA tensor
    of unit records `d_units` into the int16 CUDA tensor `d_samples`, written where the encoder would have read it.  d_states
    (n_chains, 2) int32 [prev1, prev2] is read and updated (zeros when None); d_unit_flags: uint8 tensor, one byte per record index;
    d_tail: (n_chains, 28) int16, the unit sample_limit cuts.  Returns d_states; the call waits for the stream (the chain tables it
    uploaded are temporaries)."""
    dev = d_units.device
    chains, unit_base, d_chains, d_base = _chain_tensors(chains, unit_base, dev, stream)
    if d_states is None:
        d_states = _lib.new_tensor(stream, dev, (chains.size, 2), torch.int32, 0)
    _lib.check(_bind().psxhip_adpcm_decode_chains_device(dev.index or 0, d_units.data_ptr(), d_chains.data_ptr(), d_base.data_ptr(),
                                                         chains.size, filter_count, bits, d_states.data_ptr(), d_samples.data_ptr(),
                                                         _ptr(d_unit_flags), _ptr(d_tail), _stream(dev, stream)))
    _lib.launch_stream(stream, dev).synchronize()
    return d_states


def decode_chains_chunked(d_units, chains, unit_base, filter_count, bits, d_samples, d_states=None, d_unit_flags=None, d_tail=None,
                          chunk_units=0, warmup_units=-1, max_passes=0, stream=None):
    """psxhip_adpcm_decode_chains_chunked: the same result, parallel along each chain (speculate and verify).  chunk_units <= 0: the
    library's choice; warmup_units < 0: 64.  Returns (d_states, verify passes); raises PsxHipError(PSXHIP_EINVAL) when max_passes
    ran out before a pass changed nothing (d_states is left as it was then)."""
    dev = d_units.device
    chains = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
    unit_base = np.ascontiguousarray(unit_base, dtype=np.int32)
    if d_states is None:
        d_states = _lib.new_tensor(stream, dev, (chains.size, 2), torch.int32, 0)
    rc = _bind().psxhip_adpcm_decode_chains_chunked(dev.index or 0, d_units.data_ptr(), chains.ctypes.data, unit_base.ctypes.data,
                                                    chains.size, filter_count, bits, d_states.data_ptr(), d_samples.data_ptr(),
                                                    _ptr(d_unit_flags), _ptr(d_tail), chunk_units, warmup_units, max_passes,
                                                    _stream(dev, stream))
    if rc < 0:
        _lib.check(rc)
    return d_states, rc


def adpcm_sse(d_a, d_b, chains, unit_base=None, d_a_tail=None, n_records=None, chain_sums=True, stream=None):
    """psxhip_adpcm_sse_device: two int16 CUDA tensors under one chain table.  Returns (d_unit_sse | None, d_chain_sums | None):
    per-unit sums of (a - b)^2 at the units' record indices (when unit_base is given; n_records sizes the tensor) and per chain
    [sum (a - b)^2, sum b^2] -- int64 tensors holding the library's uint64.  d_a_tail: the decode call's d_tail."""
    dev = d_a.device
    base = np.zeros(len(chains), np.int32) if unit_base is None else unit_base
    chains, base, d_chains, d_base = _chain_tensors(chains, base, dev, stream)
    d_unit = None
    if unit_base is not None:
        if n_records is None:
            n_records = int((base + (chains["n_units"] - 1) * chains["unit_stride"]).max()) + 1 if chains.size else 0
        d_unit = _lib.new_tensor(stream, dev, (max(n_records, 1),), torch.int64, 0)
    d_sums = _lib.new_tensor(stream, dev, (chains.size, 2), torch.int64, 0) if chain_sums else None
    _lib.check(_bind().psxhip_adpcm_sse_device(dev.index or 0, d_a.data_ptr(), _ptr(d_a_tail), d_b.data_ptr(), d_chains.data_ptr(),
                                               chains.size, _ptr(d_unit), d_base.data_ptr() if d_unit is not None else None,
                                               _ptr(d_sums), _stream(dev, stream)))
    _lib.launch_stream(stream, dev).synchronize()
    return d_unit, d_sums


def xa_disassemble(d_sectors, settings, d_units=None, stream=None):
    """psxhip_xa_disassemble_device: uint8 CUDA tensor (n_sectors, 2336 | 2352) -> (d_units (n_sectors * 18 * U, record bytes) uint8
    in encode order, d_status (n_sectors,) int32 XA_STATUS_* bits); asynchronous."""
    dev = d_sectors.device
    n = d_sectors.shape[0]
    bits = settings.bits_per_sample
    assert d_sectors.dtype == torch.uint8 and d_sectors.is_contiguous() and d_sectors.shape[1] == (2336 if settings.format == 0 else 2352)
    if d_units is None:
        d_units = _lib.new_tensor(stream, dev, (max(n, 1) * 18 * (8 if bits == 4 else 4), record_bytes(bits)), torch.uint8, 0)
    d_status = _lib.new_tensor(stream, dev, (max(n, 1),), torch.int32, 0)
    _lib.check(_bind().psxhip_xa_disassemble_device(dev.index or 0, d_sectors.data_ptr(), n, settings.format, int(settings.stereo),
                                                    settings.frequency, bits, d_units.data_ptr(), d_status.data_ptr(),
                                                    _stream(dev, stream)))
    return d_units, d_status[:n]


def spu_decode_streams(blocks, states=None, device=0):
    """blocks: uint8 (n_streams, 16 * n_blocks) SPU blocks.  Returns int16 (n_streams, 28 * n_blocks); `states` (n_streams, 2) int32
    [prev1, prev2] is updated in place when given."""
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
    assert blocks.ndim == 2 and blocks.shape[1] % 16 == 0
    n_streams, n_blocks = blocks.shape[0], blocks.shape[1] // 16
    st = np.zeros((n_streams, 2), np.int32) if states is None else states
    assert st.dtype == np.int32 and st.shape == (n_streams, 2) and st.flags.c_contiguous
    out = np.zeros((n_streams, 28 * n_blocks), np.int16)
    rc = _bind().psxhip_spu_decode_streams_host(device, blocks.ctypes.data, n_streams, blocks.shape[1], n_blocks, st.ctypes.data,
                                                out.ctypes.data, out.shape[1])
    if rc < 0:
        _lib.check(rc)
    return out


def xa_decode_streams(settings, sectors, states=None, device=0):
    """sectors: uint8 (n_streams, n_sectors * sector size).  Returns (pcm int16 (n_streams, samples per stream), interleaved L,R when
    stereo; status int32 (n_streams, n_sectors)).  states: (n_streams, 2, 2) int32 [[l1, l2], [r1, r2]], updated in place when given."""
    sectors = np.ascontiguousarray(sectors, dtype=np.uint8)
    ssz = 2336 if settings.format == 0 else 2352
    assert sectors.ndim == 2 and sectors.shape[1] % ssz == 0
    n_streams, n_sectors = sectors.shape[0], sectors.shape[1] // ssz
    ch = 2 if settings.stereo else 1
    st = np.zeros((n_streams, 2, 2), np.int32) if states is None else states
    assert st.dtype == np.int32 and st.shape == (n_streams, 2, 2) and st.flags.c_contiguous
    st_dev = np.ascontiguousarray(st[:, :ch, :].reshape(n_streams * ch, 2))
    per = n_sectors * (4032 if settings.bits_per_sample == 4 else 2016)
    out = np.zeros((n_streams, max(per, 1)), np.int16)
    status = np.zeros((n_streams, max(n_sectors, 1)), np.int32)
    rc = _bind().psxhip_xa_decode_streams_host(device, settings.format, int(settings.stereo), settings.frequency,
                                               settings.bits_per_sample, sectors.ctypes.data, n_streams, sectors.shape[1], n_sectors,
                                               st_dev.ctypes.data, out.ctypes.data, out.shape[1], status.ctypes.data)
    if rc < 0:
        _lib.check(rc)
    st[:, :ch, :] = st_dev.reshape(n_streams, ch, 2)
    return out[:, :per], status[:, :n_sectors]


def snr_db(chain_sums):
    """dB from psxhip_adpcm_sse_device's per-chain sums (..., 2) [sum (a - b)^2, sum b^2]: 10 log10(signal / noise); inf where the
    two sample sets are equal, -inf where the original is silence and the decode is not, nan where both sums are zero."""
    s = np.asarray(chain_sums).astype(np.uint64).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(s[..., 1] / s[..., 0])
