"""The picture ingest in front of the scaler, on one stream (psxavenc_amd.ingest.ingest_scale_device), against the scaler fed what the
ingest is stated to hand it; and the host entry against the device entry.  The scaler is not under test here: both sides run it."""
import faulthandler

import numpy as np
import pytest

import ingest_corpus as K
import ingest_ref as R

pytestmark = pytest.mark.gpu

STEP_SECONDS = 120
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


def _to_device(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)


def test_nv12_through_the_cheap_path_is_the_scaler_fed_the_planes():
    """NV12, BT.601 limited, 64 x 48 -> YUV420P -> 32 x 32 NV21: the same bytes as the scaler fed the planes de-interleaved by hand"""
    import torch
    from psxavenc_amd import ingest
    from psxavenc_amd.frontend import PIX_YUV420P, Scaler
    w, h = 64, 48
    planes, size = R.layout(R.NV12, w, h, pad=16)
    src, _ = K.pictures(R.NV12, w, h, planes, size + 32, seed=23)
    assert ingest.recommend(R.NV12, R.BT601, w, h) == PIX_YUV420P
    g = ingest.Ingest(R.NV12, w, h, planes, R.BT601, False, PIX_YUV420P)
    scaler = Scaler(PIX_YUV420P, w, h, 32, 32, src_full_range=False)
    by_hand = []
    for pic in src:
        y = pic[planes[0][0] + np.arange(h)[:, None] * planes[0][1] + np.arange(w)[None, :]]
        c = pic[planes[1][0] + np.arange(h // 2)[:, None] * planes[1][1] + np.arange(w)[None, :]]
        by_hand.append(np.concatenate([y.reshape(-1), c[:, 0::2].reshape(-1), c[:, 1::2].reshape(-1)]))
    want = scaler.convert_device(_to_device(np.stack(by_hand)))
    side = torch.cuda.Stream(device=DEV)
    d_src = _to_device(src)
    torch.cuda.synchronize()
    got = ingest.ingest_scale_device(g, scaler, d_src, stream=side)
    side.synchronize()
    assert got.shape == (4, 32 * 32 * 3 // 2) and torch.equal(got, want)
    # ... and with frames repeated and dropped, as psxhip_ingest_pace would say
    index = [0, 0, 2, 3, 3]
    got = ingest.ingest_scale_device(g, scaler, d_src, torch.tensor(index, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(got, want[index])


def test_yuyv422_bt709_through_rgb_is_the_scaler_fed_the_statements_rgb():
    """YUYV422, BT.709 limited, 34 x 18 -> RGB24 -> 16 x 16: the same bytes as the scaler fed tests/ingest_ref.py's pictures"""
    import torch
    from psxavenc_amd import ingest
    from psxavenc_amd.frontend import PIX_RGB24, Scaler
    w, h = 34, 18
    planes, size = R.layout(R.YUYV422, w, h, pad=3)
    src, _ = K.pictures(R.YUYV422, w, h, planes, size + 1, seed=29)
    assert ingest.recommend(R.YUYV422, R.BT709, w, h) == PIX_RGB24
    g = ingest.Ingest(R.YUYV422, w, h, planes, R.BT709, False, PIX_RGB24)
    scaler = Scaler(PIX_RGB24, w, h, 16, 16)
    want = scaler.convert_device(_to_device(R.convert(src, R.YUYV422, w, h, planes, R.BT709, False, R.OUT_RGB24, 0)))
    got = ingest.ingest_scale_device(g, scaler, _to_device(src))
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("fmt", [R.YUV422P, R.NV21, R.UYVY422, R.YUV444P10, R.P010, R.GRAY8, R.BGR24], ids=lambda f: R.NAMES[f])
def test_the_host_entry_is_the_device_entry(fmt):
    from psxavenc_amd import ingest
    import torch
    w, h = 34, 6
    unit = 2 if fmt in R.TEN_BIT else 1
    planes, size = R.layout(fmt, w, h, pad=3 * unit, first=unit)
    src, _ = K.pictures(fmt, w, h, planes, size + 4 * unit, seed=31)
    index = np.array([2, -1, 0, 0, 3], np.int32)
    for out_format in (R.OUT_RGB24, R.OUT_YUV420P):
        if out_format == R.OUT_YUV420P and not R.is_yuv(fmt):
            continue
        g = ingest.Ingest(fmt, w, h, planes, R.BT601, True, out_format, R.CHROMA_BILINEAR)
        before = np.full((5, g.output_bytes + 5), 0x3C, np.uint8)
        d_out = _to_device(before)
        g.convert_device(_to_device(src), torch.from_numpy(index).to(DEV), d_out=d_out)
        host = g.convert_host(src, index, out=before.copy())
        assert np.array_equal(host, d_out.cpu().numpy()), (R.NAMES[fmt], out_format)
        assert (host[1] == 0x3C).all() and np.array_equal(g.convert_host(src), g.convert_device(_to_device(src)).cpu().numpy())
