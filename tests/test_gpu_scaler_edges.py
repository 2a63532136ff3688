"""GPU tests of the scaling front-end (psxhip_scaler_*) where its kernel has separate code: every tile
shape (PSXHIP_SCALER_TILE), the shapes the create code picks for large sources, the device entry point's strides, offsets
and the bytes between frames, launches cut at the grid limit, and content that drives every clamp.  Byte for byte against
oracle/frontend_oracle.c, and on a few geometries against the float64 model of tests/scaler_model.py, so that the kernel is
held to real arithmetic even if it and the oracle change together."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import scaler_model as M

pytestmark = pytest.mark.gpu

# the geometries of test_gpu_frontend.py's bit-exact test
FRONTEND_GEOMETRIES = [
    (0, 640, 480, True, 320, 240), (1, 640, 480, True, 320, 240), (1, 640, 480, False, 320, 240), (1, 352, 288, True, 320, 240),
    (0, 200, 150, True, 320, 240), (1, 1280, 720, False, 320, 176), (0, 320, 240, True, 320, 240), (1, 720, 576, False, 640, 480),
    (0, 97, 61, True, 48, 32), (1, 1920, 1080, True, 336, 192),
]


def _gid(g):
    return "%s_%dx%d_%s_%dx%d" % ("rgb" if g[0] == 0 else "yuv", g[1], g[2], "full" if g[3] else "limited", g[4], g[5])


@functools.lru_cache(maxsize=4)
def _case(geometry):
    """(names, pictures (n, source bytes), the oracle's frames (n, frame bytes)) of one geometry's hard content"""
    fmt, sw, sh, full, dw, dh = geometry
    pics = M.hard_pictures(fmt, sw, sh, dw, dh, limited=not full, seed=sw * 7 + dh, kinds=M.kinds_for(sw, sh))
    arr = np.stack([p for _, p in pics])
    return [n for n, _ in pics], arr, O.scaler_convert(fmt, sw, sh, full, dw, dh, arr)


def _check(got, want, names, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)
        f = int(bad[0][0])
        raise AssertionError("%s: %d bytes differ; first in picture %d (%s) at byte %d: %d, the oracle %d" % (
            what, bad[0].size, f, names[f], int(bad[1][0]), got[f, bad[1][0]], want[f, bad[1][0]]))


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
@pytest.mark.parametrize("geometry", M.TILE_GEOMETRIES, ids=_gid)
def test_every_tile_shape(geometry, tile, monkeypatch):
    """each of the four tile shapes (64x16, 32x16, 32x8, 16x8) on purpose, at one, two and the launch's own number of vertical
    segments.  Every geometry here fits every shape in an MI355X's 160 KiB of LDS, so a refusal is a failure, not a skip."""
    from psxavenc_amd.frontend import Scaler
    fmt, sw, sh, full, dw, dh = geometry
    names, pics, want = _case(geometry)
    monkeypatch.setenv("PSXHIP_SCALER_TILE", str(tile))
    sc = Scaler(fmt, sw, sh, dw, dh, src_full_range=full)
    monkeypatch.delenv("PSXHIP_SCALER_TILE")
    for segs in ("1", "2", None):
        if segs is None:
            monkeypatch.delenv("PSXHIP_SCALER_VSEGS", raising=False)
        else:
            monkeypatch.setenv("PSXHIP_SCALER_VSEGS", segs)
        _check(sc.convert_host(pics), want, names, "tile %d, vertical segments %s" % (tile, segs or "default"))
    sc.close()


def test_tile_switch_refusals(monkeypatch):
    """a forced shape whose one workgroup needs more LDS than a CU has is refused with a message that says so; so is a switch
    value that names no shape"""
    from psxavenc_amd import _lib
    from psxavenc_amd.frontend import Scaler
    monkeypatch.setenv("PSXHIP_SCALER_TILE", "0")
    with pytest.raises(_lib.PsxHipError, match="LDS"):
        Scaler(O.PIX_YUV420P, 6000, 4000, 384, 256)
    monkeypatch.setenv("PSXHIP_SCALER_TILE", "4")
    with pytest.raises(_lib.PsxHipError, match="PSXHIP_SCALER_TILE"):
        Scaler(O.PIX_RGB24, 640, 480, 320, 240)


@pytest.mark.parametrize("geometry", M.EXTREME_GEOMETRIES, ids=_gid)
def test_natural_tile_at_the_extremes(geometry, monkeypatch):
    """without the switch: the shapes the create code picks for large sources, banks up to 64 taps"""
    from psxavenc_amd.frontend import Scaler
    monkeypatch.delenv("PSXHIP_SCALER_TILE", raising=False)
    monkeypatch.delenv("PSXHIP_SCALER_VSEGS", raising=False)
    fmt, sw, sh, full, dw, dh = geometry
    names, pics, want = _case(geometry)
    sc = Scaler(fmt, sw, sh, dw, dh, src_full_range=full)
    _check(sc.convert_host(pics), want, names, "natural tile")
    sc.close()


def test_acceptance_boundary():
    """RGB chroma is filtered from full resolution to half the target: 2560x1440 -> 320x240 is exactly 16x there and accepted,
    2561x1441 is refused by the chroma bank, and the message says so"""
    from psxavenc_amd import _lib
    from psxavenc_amd.frontend import Scaler
    Scaler(O.PIX_RGB24, 2560, 1440, 320, 240).close()
    with pytest.raises(_lib.PsxHipError, match="chroma horizontal"):
        Scaler(O.PIX_RGB24, 2561, 1441, 320, 240)


STRIDE_GEOMETRIES = [(0, 200, 148, True, 96, 64), (1, 350, 286, True, 320, 240)]
SENTINEL = 0xA7


def _strided_source(torch, n, nbytes, offset, stride):
    """room for n pictures as rows of a wider tensor: the view starts `offset` bytes into it, rows `stride` bytes apart"""
    buf = torch.full((offset + n * stride + 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
    view = buf[offset:offset + n * stride].view(n, stride)[:, :nbytes]
    return buf, view


def _sentinel_frames(torch, n, frame_bytes, fstride):
    buf = torch.full((n * fstride + 256,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    return buf, buf[:n * fstride].view(n, fstride)[:, :frame_bytes]


def _check_frames(buf, n, frame_bytes, fstride, want, names, what):
    host = buf.cpu().numpy()
    rows = host[:n * fstride].reshape(n, fstride)
    _check(rows[:, :frame_bytes], want, names, what)
    outside = np.concatenate([rows[:, frame_bytes:].ravel(), host[n * fstride:]])
    assert (outside == SENTINEL).all(), "%s: %d bytes outside the frames written" % (what, int((outside != SENTINEL).sum()))


@pytest.mark.parametrize("geometry", STRIDE_GEOMETRIES, ids=_gid)
def test_strides_offsets_and_bytes_between_frames(geometry, monkeypatch):
    """sources at base offsets 0..3 with src_stride = source bytes + 0, 1, 3, 64 (the aligned staging paths and the byte
    fallbacks); frames frame_stride = frame bytes + 0, 4, 256 apart in a sentinel-filled tensor: every frame equals the oracle,
    every byte outside the frames keeps the sentinel"""
    import torch
    from psxavenc_amd.frontend import Scaler
    monkeypatch.delenv("PSXHIP_SCALER_VSEGS", raising=False)
    fmt, sw, sh, full, dw, dh = geometry
    names, pics, want = _case(geometry)
    sc = Scaler(fmt, sw, sh, dw, dh, src_full_range=full)
    n, fb = pics.shape[0], sc.frame_bytes
    d_pics = torch.from_numpy(pics).to("cuda:0")
    for offset in range(4):
        for extra in (0, 1, 3, 64):
            _, src = _strided_source(torch, n, sc.source_bytes, offset, sc.source_bytes + extra)
            src.copy_(d_pics)
            for fextra in (0, 4, 256):
                out, frames = _sentinel_frames(torch, n, fb, fb + fextra)
                sc.convert_device(src, frames)
                torch.cuda.synchronize()
                _check_frames(out, n, fb, fb + fextra, want, names, "offset %d, src_stride +%d, frame_stride +%d" % (offset, extra, fextra))
    sc.close()


def test_strided_call_on_a_side_stream():
    """the input written on a non-default stream right before the call, the call on that stream, read back after that stream's
    synchronize"""
    import torch
    from psxavenc_amd.frontend import Scaler
    geometry = STRIDE_GEOMETRIES[1]
    fmt, sw, sh, full, dw, dh = geometry
    names, pics, want = _case(geometry)
    sc = Scaler(fmt, sw, sh, dw, dh, src_full_range=full)
    n, fb = pics.shape[0], sc.frame_bytes
    h_pics = torch.from_numpy(pics).pin_memory()
    _, src = _strided_source(torch, n, sc.source_bytes, 3, sc.source_bytes + 3)
    out, frames = _sentinel_frames(torch, n, fb, fb + 256)
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        src.copy_(h_pics, non_blocking=True)
        sc.convert_device(src, frames, stream=side)
    side.synchronize()
    _check_frames(out, n, fb, fb + 256, want, names, "side stream")
    sc.close()


def test_padded_frames_into_the_encoder():
    """a padded frame_stride output goes straight into MdecEncoder.encode_frames_device: against oracle scaler + oracle
    encoder (the hard content twice: more than 12 frames, the frame kernel's launch)"""
    import torch
    from psxavenc_amd.frontend import Scaler
    from psxavenc_amd.mdec import MdecEncoder
    geometry, budget = STRIDE_GEOMETRIES[1], 32768
    fmt, sw, sh, full, dw, dh = geometry
    names, pics, want = _case(geometry)
    names, pics, want = names * 2, np.concatenate([pics, pics]), np.concatenate([want, want])
    sc = Scaler(fmt, sw, sh, dw, dh, src_full_range=full)
    enc = MdecEncoder(0, dw, dh, max_frame_size=budget)
    n, fb = pics.shape[0], sc.frame_bytes
    _, src = _strided_source(torch, n, sc.source_bytes, 1, sc.source_bytes + 1)
    src.copy_(torch.from_numpy(pics).to("cuda:0"))
    out, frames = _sentinel_frames(torch, n, fb, fb + 256)
    sc.convert_device(src, frames)
    d_bs, d_res = enc.encode_frames_device(out[:n * (fb + 256)].view(n, fb + 256), budget)
    torch.cuda.synchronize()
    _check_frames(out, n, fb, fb + 256, want, names, "frames for the encoder")
    want_bs, want_res, rc = O.mdec_encode(0, dw, dh, want, budget)
    assert rc == 0
    assert np.array_equal(d_res.cpu().numpy(), want_res)
    assert np.array_equal(d_bs.cpu().numpy()[:, :budget], want_bs)
    sc.close()
    enc.close()


def test_launch_past_the_grid_limit():
    """65 537 pictures of RGB 32x32 -> 16x16, src_stride = source bytes + 1: the launch is cut at 65 535 pictures, and the second
    part's base (65 535 odd strides in) is misaligned.  Seven hard pictures in turn, so picture 65 535 falls mid-cycle; every
    frame equals its cycle member's oracle answer.  n_frames = 0 writes nothing."""
    import torch
    from psxavenc_amd.frontend import Scaler, _bind
    fmt, sw, sh, dw, dh, n, cycle = O.PIX_RGB24, 32, 32, 16, 16, 65537, 7
    pics = M.hard_pictures(fmt, sw, sh, dw, dh, seed=11)[:cycle]
    names = [p[0] for p in pics]
    base = np.stack([p[1] for p in pics])
    want = O.scaler_convert(fmt, sw, sh, True, dw, dh, base)
    sc = Scaler(fmt, sw, sh, dw, dh)
    fb, stride = sc.frame_bytes, sc.source_bytes + 1
    _, src = _strided_source(torch, n, sc.source_bytes, 0, stride)
    src.copy_(torch.from_numpy(base).to("cuda:0")[torch.arange(n, device="cuda:0") % cycle])
    out, frames = _sentinel_frames(torch, n, fb, fb)
    sc.convert_device(src, frames)
    torch.cuda.synchronize()
    which = np.arange(n) % cycle
    _check_frames(out, n, fb, fb, want[which], [names[k] for k in which], "65 537 pictures")
    # n_frames = 0: accepted, and nothing is written
    out0, frames0 = _sentinel_frames(torch, 1, fb, fb)
    rc = _bind().psxhip_scaler_convert_device(sc._h, src.data_ptr(), stride, 0, frames0.data_ptr(), fb,
                                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert (out0.cpu().numpy() == SENTINEL).all()
    sc.close()


@pytest.mark.parametrize("geometry", FRONTEND_GEOMETRIES, ids=_gid)
def test_hard_content_through_convert_host(geometry, monkeypatch):
    """test_gpu_frontend.py's ten geometries on the hard content"""
    from psxavenc_amd.frontend import Scaler
    monkeypatch.delenv("PSXHIP_SCALER_VSEGS", raising=False)
    fmt, sw, sh, full, dw, dh = geometry
    names, pics, want = _case(geometry)
    sc = Scaler(fmt, sw, sh, dw, dh, src_full_range=full)
    _check(sc.convert_host(pics), want, names, "convert_host")
    sc.close()


MODEL_GEOMETRIES = [(0, 640, 480, True, 320, 240), (1, 720, 576, False, 640, 480), (1, 350, 286, True, 320, 240), (1, 16384, 64, True, 1024, 16)]


@pytest.mark.parametrize("geometry", MODEL_GEOMETRIES, ids=_gid)
def test_kernel_against_the_real_valued_model(geometry, monkeypatch):
    """the kernel's bytes against the float64 model directly: within the derived bound per plane, and unbiased on noise"""
    from psxavenc_amd.frontend import Scaler
    monkeypatch.delenv("PSXHIP_SCALER_VSEGS", raising=False)
    fmt, sw, sh, full, dw, dh = geometry
    names, pics, _ = _case(geometry)
    bounds = M.convert_bounds(fmt, sw, sh, full, dw, dh, O.scaler_filter)
    sc = Scaler(fmt, sw, sh, dw, dh, src_full_range=full)
    got_all = sc.convert_host(pics)
    sc.close()
    for name, pic, out in zip(names, pics, got_all):
        got, want = M.nv21_planes(out, dw, dh), M.model_convert(fmt, sw, sh, full, dw, dh, pic)
        for plane, g, w, b in zip(("Y", "Cr", "Cb"), got, want, (bounds[0], bounds[1], bounds[1])):
            err = np.abs(g - w).max()
            assert err <= b, "%s, plane %s: max |err| %.3f over the bound %.3f" % (name, plane, err, b)
        if name == "noise":
            d = np.concatenate([(g - w).ravel() for g, w in zip(got, want)])
            assert np.abs(d).mean() <= 0.30 and abs(d.mean()) <= 0.05, (np.abs(d).mean(), d.mean())
