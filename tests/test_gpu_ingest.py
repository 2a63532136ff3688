"""The picture ingest on the device (psxavenc_amd/ingest.py) against the statement (tests/ingest_ref.py), byte for byte: every
format, both outputs, both chroma modes, three matrices and both ranges over the corpus of tests/ingest_corpus.py; padded pitches and
shifted planes; the bytes the call must not touch; the picture selection; more pictures than a grid dimension holds; a stream of the
caller's.

The shapes are the smallest at which the kernel can go wrong -- a lane's run of eight pixels cut short by 1 .. 7, one lane, several
wavefronts, packed rows that start off a dword, and rows that are whole dwords -- not the workload's.  Every test is one GPU step
under a time limit of its own: a watchdog ends the process if a step hangs, so nothing more is started on the device after it."""
import faulthandler

import numpy as np
import pytest

import ingest_corpus as K
import ingest_ref as R

pytestmark = pytest.mark.gpu

STEP_SECONDS = 120
FILL = 0x5A
DEV = "cuda:0"


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
def ingest():
    from psxavenc_amd import ingest as m
    return m


def _to_device(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)


def _same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if not np.array_equal(got, want):
        bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
        raise AssertionError("%s: %d of %d bytes differ from the statement, the first at %d: %d, statement %d" % (
            what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))


def _what(fmt, w, h, m, full, out, opt, extra=""):
    return "%s %dx%d matrix %d %s -> %s%s%s" % (R.NAMES[fmt], w, h, m, "full" if full else "limited", "YUV420P" if out else "RGB24",
                                                 " bilinear" if opt else "", extra)


# ---------------------------------------------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("fmt", R.ALL_FORMATS, ids=R.NAMES)
def test_every_setting_over_the_corpus(ingest, fmt):
    """noise and 0 / max checkerboards, 10-bit words with garbage in their unused bits, at every size of the corpus"""
    import torch
    unit = 2 if fmt in R.TEN_BIT else 1
    for out_format in (R.OUT_RGB24, R.OUT_YUV420P):
        settings = [s for s in K.settings_for(fmt) if s[2] == out_format]
        for w, h in K.sizes_for(fmt, out_format) if settings else []:
            planes, size = R.layout(fmt, w, h)
            src, _ = K.pictures(fmt, w, h, planes, size + 3 * unit, seed=7)
            d_src = _to_device(src)
            for m, full, out, opt in settings:
                g = ingest.Ingest(fmt, w, h, planes, m, full, out, opt)
                got = g.convert_device(d_src)
                _same(got, R.convert(src, fmt, w, h, planes, m, full, out, opt), _what(fmt, w, h, m, full, out, opt))
                g.close()
            assert torch.equal(d_src.cpu(), torch.from_numpy(src)), "the source changed"


@pytest.mark.parametrize("fmt", R.ALL_FORMATS, ids=R.NAMES)
def test_every_setting_at_sizes_of_several_wavefronts_and_workgroups(ingest, fmt):
    """the sizes the matrix above stays below (it ends at 48 lanes, inside one wavefront): two wavefronts whose bilinear rows meet across
    the seam, a wavefront per row of whole dwords, two workgroups with a ragged tail, a second workgroup of one lane, and an odd size"""
    import torch
    unit = 2 if fmt in R.TEN_BIT else 1
    lanes = []
    for out_format in (R.OUT_RGB24, R.OUT_YUV420P):
        settings = [s for s in K.settings_for(fmt) if s[2] == out_format]
        for w, h in K.wide_sizes_for(fmt, out_format) if settings else []:
            lanes.append(K.lanes_of(w, h))
            planes, size = R.layout(fmt, w, h)
            src, _ = K.pictures(fmt, w, h, planes, size + 3 * unit, seed=23)
            d_src = _to_device(src)
            for m, full, out, opt in settings:
                g = ingest.Ingest(fmt, w, h, planes, m, full, out, opt)
                got = g.convert_device(d_src)
                _same(got, R.convert(src, fmt, w, h, planes, m, full, out, opt), _what(fmt, w, h, m, full, out, opt))
                g.close()
            assert torch.equal(d_src.cpu(), torch.from_numpy(src)), "the source changed"
    assert sorted(set(lanes)) == ([85, 192, 257, 330] if fmt in R.PACKED else [85, 192, 195, 257, 330])


# ---------------------------------------------------------------------------------------------------------------- placement
@pytest.mark.parametrize("fmt", R.ALL_FORMATS, ids=R.NAMES)
def test_padded_pitches_shifted_planes_and_untouched_bytes(ingest, fmt):
    """pitches of the row bytes + 1, + 3, + 13 and plane offsets 0 .. 3 (twice that for 16-bit words); the source keeps every byte,
    and the output every byte past its packed pictures up to out_stride"""
    unit = 2 if fmt in R.TEN_BIT else 1
    for out_format in (R.OUT_RGB24, R.OUT_YUV420P):
        if out_format == R.OUT_YUV420P and not R.is_yuv(fmt):
            continue
        for w, h in [(18, 4), (16, 4)]:
            for pad in K.PADS:
                for first in K.OFFSETS:
                    planes, size = R.layout(fmt, w, h, pad * unit, first * unit, gap=(first ^ 1) * unit)
                    src, _ = K.pictures(fmt, w, h, planes, size + (5 + first) * unit, seed=11)
                    opt = R.CHROMA_BILINEAR if (first & 1 and out_format == R.OUT_RGB24) else 0
                    g = ingest.Ingest(fmt, w, h, planes, R.BT601, bool(first & 2), out_format, opt)
                    d_src = _to_device(src)
                    before = np.full((src.shape[0], g.output_bytes + 13 - first), FILL, np.uint8)
                    d_out = _to_device(before)
                    assert g.convert_device(d_src, d_out=d_out) is d_out
                    what = _what(fmt, w, h, 0, first & 2, out_format, opt, ", pad %d, first plane at %d" % (pad * unit, first * unit))
                    _same(d_out, R.convert(src, fmt, w, h, planes, R.BT601, bool(first & 2), out_format, opt, out=before), what)
                    _same(d_src, src, what + ": the source")
                    g.close()


# ---------------------------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("fmt,out_format,w,h", [(R.NV12, R.OUT_RGB24, 18, 6), (R.YUV422P10, R.OUT_YUV420P, 34, 6), (R.BGRA32, R.OUT_RGB24, 5, 7),
                                                 (R.UYVY422, R.OUT_YUV420P, 16, 4)])
def test_pictures_are_selected_by_index(ingest, fmt, out_format, w, h):
    """4 sources -> 9 outputs: duplicates, a source that is dropped, reversed order, negative entries and one past the sources; the
    outputs that are not written keep their guard pattern"""
    import torch
    planes, size = R.layout(fmt, w, h, pad=2)
    src, _ = K.pictures(fmt, w, h, planes, size + 6, seed=13)
    index = [3, 3, -1, 2, 0, 0, -5, 3, 4]                   # (source 1 is dropped; 4 is past the sources: left as it is)
    g = ingest.Ingest(fmt, w, h, planes, R.BT709 if out_format == R.OUT_RGB24 else R.BT601, False, out_format, 0)
    before = np.full((len(index), g.output_bytes + 8), FILL, np.uint8)
    d_out = _to_device(before)
    g.convert_device(_to_device(src), torch.tensor(index, dtype=torch.int32, device=DEV), d_out=d_out)
    stated = [i if i < 4 else -1 for i in index]
    want = R.convert(src, fmt, w, h, planes, R.BT709 if out_format == R.OUT_RGB24 else R.BT601, False, out_format, 0, index=stated, out=before)
    assert (want[[2, 6, 8]] == FILL).all() and not (want[0] == FILL).all()
    _same(d_out, want, "4 sources -> 9 outputs")
    # the index alone decides: reversed order into a fresh destination
    got = g.convert_device(_to_device(src), torch.tensor([3, 2, 1, 0], dtype=torch.int32, device=DEV))
    _same(got, R.convert(src, fmt, w, h, planes, R.BT709 if out_format == R.OUT_RGB24 else R.BT601, False, out_format, 0, index=[3, 2, 1, 0]), "reversed")


def test_more_outputs_than_a_grid_dimension_holds(ingest):
    """65 537 outputs of 2 x 2 from 3 sources: two launches, the second of two pictures"""
    import torch
    fmt, w, h, n = R.NV21, 2, 2, 65537
    planes, size = R.layout(fmt, w, h)
    src, _ = K.pictures(fmt, w, h, planes, size + 2, seed=17)
    src = src[:3]
    index = (np.arange(n) * 7 + np.arange(n) // 65535) % 4 - 1          # -1, 0, 1, 2
    index[-2:] = [2, 0]
    g = ingest.Ingest(fmt, w, h, planes, R.BT601, True, R.OUT_RGB24, 0)
    before = np.full((n, 16), FILL, np.uint8)
    d_out = _to_device(before)
    g.convert_device(_to_device(src), torch.from_numpy(index.astype(np.int32)).to(DEV), d_out=d_out)
    _same(d_out, R.convert(src, fmt, w, h, planes, R.BT601, True, R.OUT_RGB24, 0, index=index, out=before), "65 537 outputs")
    # ... and without an index: picture for picture across the cut
    many = np.tile(src, (21846, 1))[:n]
    got = g.convert_device(_to_device(many))
    want = R.convert(src, fmt, w, h, planes, R.BT601, True, R.OUT_RGB24, 0)
    _same(got, np.tile(want, (21846, 1))[:n], "65 537 pictures, identity")


# ---------------------------------------------------------------------------------------------------------------- streams
def test_a_stream_of_the_callers(ingest):
    """a non-default stream, the output allocated on it by the wrapper: right after stream.synchronize() alone"""
    import torch
    fmt, w, h = R.P010, 66, 10
    planes, size = R.layout(fmt, w, h, pad=4)
    src, _ = K.pictures(fmt, w, h, planes, size, seed=19)
    d_src = _to_device(src)
    torch.cuda.synchronize()                              # the upload: not this call's to order
    side = torch.cuda.Stream(device=DEV)
    for out_format, opt in ((R.OUT_RGB24, R.CHROMA_BILINEAR), (R.OUT_YUV420P, 0)):
        g = ingest.Ingest(fmt, w, h, planes, R.BT601, False, out_format, opt)
        got = g.convert_device(d_src, stream=side)
        side.synchronize()
        _same(got, R.convert(src, fmt, w, h, planes, R.BT601, False, out_format, opt), "on a side stream")
        g.close()
