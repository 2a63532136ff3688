"""The display back-end on the device (psxavenc_amd/display.py, MdecDecoder.decode_display_device) against the statement
(tests/display_ref.py), byte for byte: every format and option over the corpus of tests/display_corpus.py, placement inside a
larger surface, the decoder's gate, more frames than a grid dimension holds, bitstreams to pictures in one call, the host entry, and
the stream contract of both device entry points (tests/stream_cases.py).

The shapes are the smallest at which the kernel can go wrong -- a row of four lanes, a picture of one workgroup and of many, the
planes' edges and corners -- not the workload's.  Every test is one GPU step under a time limit of its own: a watchdog ends the
process if a step hangs, so nothing more is started on the device after it."""
import faulthandler
import functools

import numpy as np
import pytest

import display_corpus as K
import display_ref as R
import stream_cases as SC

pytestmark = pytest.mark.gpu

STEP_SECONDS = 120
FILL = 0xA5
DEV = SC.DEV


@pytest.fixture(autouse=True)
def step_time_limit():
    import torch
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()
    try:
        torch.cuda.synchronize()
    except Exception as e:                               # a device error: nothing more is started on the device
        pytest.exit("the device reported an error after this step: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def display():
    from psxavenc_amd import display as d
    return d


def _to_device(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)             # (a copy: the corpus is read-only)


def _same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if not np.array_equal(got, want):
        bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
        raise AssertionError("%s: %d of %d bytes differ from the statement, the first at %d: %d, statement %d" % (
            what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))


# ---------------------------------------------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("w,h", K.SIZES)
def test_formats_and_options_over_the_corpus(display, w, h, n):
    """the corpus in calls of n frames: 3 formats x 2 chroma modes, RGB555 also x dither x mask bit"""
    import torch
    frames, kinds = K.frames(w, h)
    d_frames = _to_device(frames)
    for fmt, options in R.all_option_sets():
        got = torch.cat([display.convert_device(d_frames[i:i + n], w, h, fmt, options) for i in range(0, frames.shape[0], n)])
        want = K.expected(w, h, fmt, options)
        got = got.cpu().numpy()
        for kind in sorted(set(kinds)):
            pick = [k == kind for k in kinds]
            _same(got[pick], want[pick], "%dx%d, format %d, options %d, calls of %d, %s frames" % (w, h, fmt, options, n, kind))


# ---------------------------------------------------------------------------------------------------------------- placement
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_placement_inside_a_larger_surface(display, fmt):
    """a padded frame_stride; dst_pitch of the row bytes + 4 and + 68, dst_stride with 256 spare bytes, d_dst 4, 8 and 12 bytes past
    an aligned base; every byte outside the row bytes keeps the 0xA5 it held"""
    import torch
    w, h, n = 48, 32, 3
    fb, row = w * h * 3 // 2, R.row_bytes(fmt, w)
    rng = np.random.default_rng(40 + fmt)
    padded = rng.integers(0, 256, (n, fb + 64)).astype(np.uint8)
    d_frames = _to_device(padded)[:, :fb]
    assert d_frames.stride(0) == fb + 64
    extras = (R.DITHER | R.MASK_BIT) if fmt == R.OUT_RGB555 else 0
    for options in (extras, extras | R.CHROMA_BILINEAR):
        pics = R.pictures(padded, w, h, fmt, options)
        for pitch in (row + 4, row + 68):
            stride = (h - 1) * pitch + row + 256
            for offset in (4, 8, 12):
                size = offset + n * stride + pitch
                base = torch.full((size,), FILL, dtype=torch.uint8, device=DEV)
                assert base.data_ptr() % 16 == 0
                d_dst = base[offset:].as_strided((n, h, pitch), (stride, pitch, 1))
                out = display.convert_device(d_frames, w, h, fmt, options, d_dst=d_dst)
                assert out.data_ptr() == base.data_ptr() + offset
                want = R.place(np.full(size, FILL, np.uint8), pics, pitch, stride, offset)
                _same(base, want, "format %d, options %d, pitch %d, offset %d" % (fmt, options, pitch, offset))


# ---------------------------------------------------------------------------------------------------------------- the gate
def test_frames_the_decoder_gave_up_are_skipped(display):
    import torch
    w, h = 32, 16
    statuses = [0, -5, 0, -1, 0]
    frames = np.random.default_rng(50).integers(0, 256, (5, w * h * 3 // 2)).astype(np.uint8)
    decoded = np.zeros((5, 4), np.int32)
    decoded[:, 0], decoded[:, 1], decoded[:, 2] = statuses, 7, 2
    d_frames, d_decoded = _to_device(frames), _to_device(decoded)
    for fmt, options in R.all_option_sets():
        row = R.row_bytes(fmt, w)
        d_dst = torch.full((5, h, row), FILL, dtype=torch.uint8, device=DEV)
        got = display.convert_device(d_frames, w, h, fmt, options, d_decoded=d_decoded, d_dst=d_dst).cpu().numpy()
        _same(got, R.convert(frames, w, h, fmt, options, statuses=statuses, fill=FILL), "gated, format %d, options %d" % (fmt, options))
        assert (got[[1, 3]] == FILL).all()
        d_dst.fill_(FILL)
        _same(display.convert_device(d_frames, w, h, fmt, options, d_dst=d_dst), R.pictures(frames, w, h, fmt, options),
              "no records, format %d, options %d" % (fmt, options))
    # a destination the wrapper allocates reads as zeros where a frame was skipped
    got = display.convert_device(d_frames, w, h, R.OUT_RGB24, 0, d_decoded=d_decoded)
    _same(got, R.convert(frames, w, h, R.OUT_RGB24, 0, statuses=statuses, fill=0), "gated, the wrapper's destination")


# ---------------------------------------------------------------------------------------------------------------- many frames
def test_more_frames_than_a_grid_dimension_holds(display):
    """65 537 frames of 16x16 to RGB555 (25 MB in, 34 MB out): frames are a grid dimension, cut into launches at 65 535.  The frames
    are drawn from a pool of 256 distinct noise frames, so the statement's answer is the pool's pictures in the same order"""
    w, h, n = 16, 16, 65537
    rng = np.random.default_rng(60)
    pool = rng.integers(0, 256, (256, w * h * 3 // 2)).astype(np.uint8)
    order = rng.integers(0, 256, n)
    order[[0, 65534, 65535, 65536]] = [3, 5, 7, 11]               # the seams carry known, different frames
    options = R.DITHER | R.CHROMA_BILINEAR
    pool_pictures = R.pictures(pool, w, h, R.OUT_RGB555, options)
    d_frames = _to_device(pool)[_to_device(order)]
    got = display.convert_device(d_frames, w, h, R.OUT_RGB555, options).cpu().numpy()
    assert got.shape == (n, h, 2 * w)
    for i in [0, n - 1, 65534, 65535] + sorted(rng.choice(n, 64, replace=False).tolist()):
        _same(got[i], pool_pictures[order[i]], "frame %d" % i)
    want = pool_pictures[order]
    assert int(got.astype(np.uint64).sum()) == int(want.astype(np.uint64).sum())
    _same(got, want, "all %d frames" % n)


# ---------------------------------------------------------------------------------------------------------------- decode and display
@functools.lru_cache(maxsize=None)
def _encoded(w, h, per_codec, budget, seed):
    """per_codec frames as v2 and as many as v3, rows of `budget` bytes from the oracle's encoder"""
    import oracle_lib as O
    rows, sizes = [], []
    for codec in (0, 1):
        out, res, rc = O.mdec_encode(codec, w, h, O.synth_frames(w, h, per_codec, seed=seed + codec, amp=10), budget)
        assert rc == 0
        rows.append(out)
        sizes.append(np.minimum(res[:, 1], budget))
    bs, sizes = np.concatenate(rows), np.concatenate(sizes).astype(np.int32)
    order = np.arange(2 * per_codec).reshape(2, per_codec).T.reshape(-1)        # v2, v3, v2, v3, ...
    return bs[order], sizes[order]


def _decode_statement(w, h, bs, sizes):
    """(NV21 frames, records) of the decoder's statements (the oracle's reader, tests/mdec_recon_ref.py); a frame that does not
    parse keeps zeros for its pixels"""
    import mdec_recon_ref as M
    import oracle_lib as O
    n = bs.shape[0]
    frames, decoded = np.zeros((n, w * h * 3 // 2), np.uint8), np.zeros((n, 4), np.int32)
    for i in range(n):
        rc, levels, q, v, nbits = O.mdec_decode(w, h, bs[i, :sizes[i]])
        # (include/psxav_hip.h: quant scale and version are 0 when the magic is wrong, the bits consumed 0 unless the frame parses)
        decoded[i] = (rc, q, v, nbits) if rc == 0 else (rc, 0, 0, 0) if rc == -1 else (rc, q, v, 0)
        if rc == 0:
            frames[i] = M.reconstruct(w, h, levels, q)
    return frames, decoded


def test_bitstreams_to_pictures_in_one_call(oracle, display):
    import torch
    from psxavenc_amd import MdecDecoder
    w, h, budget = 48, 32, 4096
    bs, sizes = _encoded(w, h, 3, budget, 70)
    bs = bs.copy()
    bs[2, 2:4] = (0x12, 0x34)                                      # frame 2: not the magic 00 38
    want_frames, want_decoded = _decode_statement(w, h, bs, sizes)
    assert want_decoded[:, 0].tolist() == [0, 0, -1, 0, 0, 0] and sorted(set(want_decoded[:, 2].tolist())) == [0, 2, 3]
    d_bs, d_sizes = _to_device(bs), _to_device(sizes)
    dec = MdecDecoder(w, h)
    try:
        for fmt, options in [(R.OUT_RGB24, 0), (R.OUT_RGBX32, R.CHROMA_BILINEAR), (R.OUT_RGB555, R.DITHER | R.MASK_BIT | R.CHROMA_BILINEAR)]:
            row = R.row_bytes(fmt, w)
            d_dst = torch.full((6, h, row + 4), FILL, dtype=torch.uint8, device=DEV)
            d_pictures, d_decoded = dec.decode_display_device(d_bs, d_sizes, fmt, options, d_dst=d_dst)
            _, d_frames, d_decoded2 = dec.decode_frames_device(d_bs, d_sizes, levels=False)
            d_two_steps = display.convert_device(d_frames, w, h, fmt, options, d_decoded=d_decoded2,
                                                 d_dst=torch.full((6, h, row + 4), FILL, dtype=torch.uint8, device=DEV))
            torch.cuda.synchronize()
            got = d_pictures.cpu().numpy()
            _same(d_decoded, want_decoded, "records")
            _same(d_decoded2, want_decoded, "records of decode_frames_device")
            _same(got, d_two_steps.cpu().numpy(), "format %d: one call against decode_frames_device + convert_device" % fmt)
            _same(got, R.convert(want_frames, w, h, fmt, options, statuses=want_decoded[:, 0], dst_pitch=row + 4, fill=FILL),
                  "format %d: one call against the statements" % fmt)
            assert (got[2] == FILL).all()
        # sizes as one int, a destination the wrapper allocates
        d_pictures, d_decoded = dec.decode_display_device(d_bs, budget, R.OUT_RGB24)
        _same(d_pictures, R.convert(want_frames, w, h, R.OUT_RGB24, statuses=want_decoded[:, 0]), "uniform size")
    finally:
        torch.cuda.synchronize()
        dec.close()


# ---------------------------------------------------------------------------------------------------------------- the host entry
def test_host_entry_equals_the_device_entry(display):
    w, h = 48, 32
    frames = K.frames(w, h)[0][:6]
    d_frames = _to_device(frames)
    for fmt, options in R.all_option_sets():
        got = display.convert_host(frames, w, h, fmt, options)
        _same(got, display.convert_device(d_frames, w, h, fmt, options).cpu().numpy(), "host against device, format %d, options %d" % (fmt, options))
        _same(got, K.expected(w, h, fmt, options)[:6], "host against the statement, format %d, options %d" % (fmt, options))
    assert display.convert_host(frames[:0], w, h).shape == (0, h, 3 * w)


# ---------------------------------------------------------------------------------------------------------------- the stream contract
@pytest.fixture(scope="module")
def calibrated():
    """cycles per millisecond of the delay, once per module, on an idle device"""
    return SC.cycles_per_ms()


@functools.lru_cache(maxsize=None)
def convert_case():
    """display.convert_device: 4 frames of 48x32 to dithered RGB555 with bilinear chroma, one frame skipped by its record (another
    one in the decoy): its picture keeps what the buffer held"""
    w, h, n = SC.W, SC.H, 4
    fmt, options = R.OUT_RGB555, R.DITHER | R.CHROMA_BILINEAR

    def host(seed, skipped):
        decoded = np.zeros((n, 4), np.int32)
        decoded[skipped, 0] = -5
        return dict(frames=np.random.default_rng(seed).integers(0, 256, (n, w * h * 3 // 2)).astype(np.uint8), decoded=decoded)

    def call(hd, d, out, stream):
        from psxavenc_amd import display as D
        return dict(pictures=D.convert_device(d["frames"], w, h, fmt, options, d_decoded=d["decoded"], d_dst=out.get("pictures"), stream=stream))

    def expect(x, fill):
        return dict(pictures=R.convert(x["frames"], w, h, fmt, options, statuses=x["decoded"][:, 0], fill=fill))

    return SC.Case("display.convert_device", host(91, 1), host(92, 2), dict(pictures=((n, h, R.row_bytes(fmt, w)), np.uint8)), call, expect)


@functools.lru_cache(maxsize=None)
def decode_display_case(scale=1):
    """MdecDecoder.decode_display_device over the inputs of stream_cases.mdec_decode: 48x32, 4 frames a scale, per-frame sizes"""
    base = SC.mdec_decode(scale)
    w, h, n = SC.W, SC.H, 4 * scale
    fmt, options = R.OUT_RGBX32, R.CHROMA_BILINEAR

    def call(hd, d, out, stream):
        pictures, decoded = hd.decode_display_device(d["bs"], d["sizes"], fmt, options, d_decoded=out.get("decoded"), d_dst=out.get("pictures"),
                                                     stream=stream)
        return dict(pictures=pictures, decoded=decoded)

    def expect(x, fill):
        frames, decoded = _decode_statement(w, h, x["bs"], x["sizes"])
        assert (decoded[:, 0] == 0).all()
        return dict(pictures=R.convert(frames, w, h, fmt, options, fill=fill), decoded=decoded)

    return SC.Case("MdecDecoder.decode_display_device x%d" % scale, base.real, base.decoy,
                   dict(pictures=((n, h, R.row_bytes(fmt, w)), np.uint8), decoded=((n, 4), np.int32)), call, expect, base.handle)


CONTRACT = dict([("display.convert_device", convert_case), ("MdecDecoder.decode_display_device", decode_display_case)])


@pytest.mark.parametrize("name", list(CONTRACT))
def test_late_producer_on_a_side_stream(oracle, calibrated, name):
    SC.late_producer(CONTRACT[name]())


@pytest.mark.parametrize("name", list(CONTRACT))
def test_busy_current_stream_and_outputs_the_wrapper_allocates(oracle, calibrated, name):
    SC.busy_current_stream(CONTRACT[name]())


def test_nv21_workspace_grows_between_unsynchronised_calls(oracle, calibrated):
    SC.growing_workspace(decode_display_case(1), decode_display_case(4))
