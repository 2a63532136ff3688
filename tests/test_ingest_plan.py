"""The picture ingest's host layer, which needs no device: the library's matrix against the statement (tests/ingest_ref.py), the two
planners against restatements of psxavenc/decoding.c:275-285 and :412-461, the recommendation, and every argument rule of create and
convert with the rule named in the error text."""
import ctypes as C

import numpy as np
import pytest

import ingest_ref as R


def _mod():
    from psxavenc_amd import ingest
    return ingest


def _create(fmt=R.NV12, w=16, h=8, planes=None, matrix=R.BT601, full=False, out=R.OUT_RGB24, options=0, n_planes=None):
    """psxhip_ingest_create's return code and handle, with sound arguments except those given"""
    ingest = _mod()
    planes = R.layout(fmt, w, h)[0] if planes is None else planes
    arr = (ingest.Plane * max(1, len(planes)))(*[ingest.Plane(o, p) for o, p in planes])
    h_ = C.c_void_p()
    rc = ingest._bind().psxhip_ingest_create(C.byref(h_), 0, fmt, w, h, C.cast(arr, C.c_void_p), len(planes) if n_planes is None else n_planes,
                                            matrix, int(full), out, options)
    return rc, h_


def _error():
    from psxavenc_amd import _lib
    return _lib.lib().psxhip_last_error().decode()


def test_the_librarys_matrix_is_the_statements_for_all_twenty_combinations():
    ingest = _mod()
    assert ingest.kernel_rev() == "ingest-k1.0"
    seen = 0
    for m in range(5):
        for full in (False, True):
            for fmt, bits in ((R.YUV420P, 8), (R.NV12, 8), (R.GRAY8, 8), (R.YUV422P10, 10), (R.P010, 10)):
                g = ingest.Ingest(fmt, 16, 8, R.layout(fmt, 16, 8)[0], m, full)
                assert g.matrix() == R.coefficients(m, full, bits), (m, full, fmt)
                g.close()
                seen += 1
    assert seen == 20 * 5 // 2
    g = ingest.Ingest(R.NV21, 16, 8, R.layout(R.NV21, 16, 8)[0], R.BT601, True)
    assert g.matrix() == (65536, 91881, -22553, -46802, 116130, 0, 128)                # the display back-end's constants
    g = ingest.Ingest(R.BGRA32, 5, 3, R.layout(R.BGRA32, 5, 3)[0], R.BT2020, False)
    assert g.matrix() == (0,) * 7 and g.output_bytes == 45 and g.source_bytes == 60


def test_sizes_of_a_handle():
    ingest = _mod()
    for fmt in R.ALL_FORMATS:
        for pad, first in ((0, 0), (6, 2)):
            planes, size = R.layout(fmt, 18, 6, pad, first, gap=2)
            for out in (R.OUT_RGB24, R.OUT_YUV420P):
                if out == R.OUT_YUV420P and not R.is_yuv(fmt):
                    continue
                g = ingest.Ingest(fmt, 18, 6, planes, out_format=out)
                assert g.source_bytes == size and g.output_bytes == R.output_bytes(out, 18, 6), (fmt, pad, out)


SOURCES = [(w, h) for w in range(1, 65) for h in range(1, 65)] + [(320, 240), (1280, 720), (1920, 1080), (720, 576), (853, 480)]


def _fit_expected(sw, sh):
    """decoding.c:275-285 for every target of the grid at once, in float64 as the reference computes it: (w, h) arrays, 0 = EINVAL"""
    mw, mh = np.meshgrid(np.arange(16, 656, 16), np.arange(16, 528, 16), indexing="ij")
    src_ratio = np.float64(sw) / np.float64(sh)
    dst_ratio = mw.astype(np.float64) / mh.astype(np.float64)

    def c_round(x):                                   # half away from zero (x >= 0 here); x - floor(x) is exact
        f = np.floor(x)
        return (f + (x - f >= 0.5)).astype(np.int64)
    narrow = src_ratio < dst_ratio
    w = np.where(narrow, (c_round(mh.astype(np.float64) * src_ratio) + 15) & ~15, mw)
    h = np.where(narrow, mh, (c_round(mw.astype(np.float64) / src_ratio) + 15) & ~15)
    bad = (w < 1) | (h < 1) | (w > mw) | (h > mh)
    return np.where(bad, 0, w), np.where(bad, 0, h)


def test_fit_is_the_references_aspect_fit():
    from psxavenc_amd import _lib
    f = _mod()._bind().psxhip_ingest_fit
    w, h = C.c_int(), C.c_int()
    pw, ph = C.byref(w), C.byref(h)
    targets = [(mw, mh) for mw in range(16, 656, 16) for mh in range(16, 528, 16)]
    n_bad = 0
    for sw, sh in SOURCES:
        got = []
        for mw, mh in targets:
            rc = f(sw, sh, mw, mh, 0, pw, ph)
            got.append((w.value, h.value) if rc == 0 else (0, 0))
        ew, eh = _fit_expected(sw, sh)
        got = np.array(got, np.int64).reshape(ew.shape + (2,))
        assert np.array_equal(got[..., 0], ew) and np.array_equal(got[..., 1], eh), (sw, sh)
        n_bad += int((ew == 0).sum())
    assert n_bad > 0                                   # a side that comes out 0 is EINVAL
    # the scalar restatement says the same, here and there
    for sw, sh, mw, mh in [(1920, 1080, 320, 240), (720, 576, 320, 240), (853, 480, 640, 512), (3, 64, 320, 240), (64, 1, 16, 16), (1, 64, 16, 16)]:
        want = R.fit(sw, sh, mw, mh)
        rc = f(sw, sh, mw, mh, 0, pw, ph)
        assert (None if rc else (w.value, h.value)) == want, (sw, sh, mw, mh)
    assert _mod().fit(1920, 1080, 320, 240) == (320, 192) and _mod().fit(1920, 1080, 320, 240, ignore_aspect=True) == (320, 240)
    assert f(64, 1, 16, 16, 0, pw, ph) == _lib.PSXHIP_EINVAL and "a side is 0" in _error()
    for mw, mh in [(0, 240), (320, 250), (1040, 240), (320, 8)]:
        assert f(320, 240, mw, mh, 0, pw, ph) == _lib.PSXHIP_EINVAL and "multiple of 16" in _error()
    assert f(0, 240, 320, 240, 0, pw, ph) == _lib.PSXHIP_EINVAL and f(320, 240, 320, 240, 0, None, ph) == _lib.PSXHIP_EINVAL


def _pts_lists():
    rng = np.random.default_rng(412)
    even = np.arange(0, 200)
    out = {
        "lower_rate_duplicates": (even * 1000, 1, 12000, 30, 1),                  # 12 fps -> 30
        "higher_rate_drops": (even * 1000, 1, 60000, 15, 1),                      # 60 fps -> 15
        "equal_rates": (even * 512, 1, 15360, 30, 1),
        "negative_first_pts": (even * 1001 - 7007, 1, 30000, 15, 1),
        "jitter_of_one_tick": (even * 40 + rng.integers(-1, 2, even.size), 1, 1000, 25, 1),
        "a_gap_of_seconds": (np.concatenate([np.arange(50), np.arange(50) + 50 + 25 * 7]) * 40, 1, 1000, 25, 1),
        "non_monotone": (even * 40 + rng.permutation(even.size)[:even.size] % 5 * 40 - 80, 1, 1000, 25, 1),
        "ntsc": (even * 3003, 1, 90000, 30000, 1001),
        "ntsc_to_15": (even * 1001 + rng.integers(-1, 2, even.size), 1, 30000, 15, 1),
        "film_to_ntsc": (even * 1001, 1, 24000, 30000, 1001),
        "random_walk": (np.cumsum(rng.integers(-20, 120, 300)), 1, 1000, 30000, 1001),
        "time_base_with_a_numerator": (even * 3, 1001, 90000, 10, 1),
        "one_picture": (np.array([5]), 1, 25, 15, 1),
        "none": (np.array([], np.int64), 1, 25, 15, 1),
    }
    return out


@pytest.mark.parametrize("name", sorted(_pts_lists()))
def test_pace_is_the_references_frame_pacing(name):
    ingest = _mod()
    pts, tb_num, tb_den, fps_num, fps_den = _pts_lists()[name]
    want = R.pace([int(t) for t in pts], tb_num, tb_den, fps_num, fps_den)
    got = ingest.pace(pts, tb_num, tb_den, fps_num, fps_den)
    assert got.dtype == np.int32 and got.tolist() == want, name
    if name == "lower_rate_duplicates":
        assert len(want) > 2 * len(pts) and want[:4] == [0, 0, 0, 1]
    if name == "higher_rate_drops":
        assert len(want) < len(pts) / 3 and sorted(set(want)) == want
    if name == "equal_rates":                          # (the reference's accumulated `next` drifts by ulps: stray repeats and drops are its own)
        assert abs(len(want) - len(pts)) <= 2
    if name == "a_gap_of_seconds":
        assert want.count(49) > 25 * 6
    if len(want) > 3:                                  # a cap that is too small: the needed count, and only cap entries written
        small = np.full(5, -7, np.int32)
        p64 = np.ascontiguousarray(pts, np.int64)
        assert ingest._bind().psxhip_ingest_pace(p64.ctypes.data, p64.size, tb_num, tb_den, fps_num, fps_den, small.ctypes.data, 3) == len(want)
        assert small.tolist() == want[:3] + [-7, -7]


def test_pace_refuses_bad_arguments():
    from psxavenc_amd import _lib
    f = _mod()._bind().psxhip_ingest_pace
    pts = np.arange(4, dtype=np.int64)
    out = np.zeros(8, np.int32)
    for args in [(None, 4, 1, 25, 15, 1, out.ctypes.data, 8), (pts.ctypes.data, -1, 1, 25, 15, 1, out.ctypes.data, 8),
                 (pts.ctypes.data, 4, 0, 25, 15, 1, out.ctypes.data, 8), (pts.ctypes.data, 4, 1, 0, 15, 1, out.ctypes.data, 8),
                 (pts.ctypes.data, 4, 1, 25, 0, 1, out.ctypes.data, 8), (pts.ctypes.data, 4, 1, 25, 15, 0, out.ctypes.data, 8),
                 (pts.ctypes.data, 4, 1, 25, 15, 1, None, 8)]:
        assert f(*args) == _lib.PSXHIP_EINVAL, args


def test_recommend_is_the_cheap_path_where_create_takes_it():
    from psxavenc_amd import _lib
    ingest = _mod()
    for fmt in R.ALL_FORMATS:
        for m in range(5):
            for w, h in [(16, 8), (15, 8), (16, 7), (2, 2)]:
                if fmt in R.PACKED and w % 2:
                    continue
                want = R.OUT_YUV420P if R.yuv420p_allowed(fmt, m, w, h) else R.OUT_RGB24
                assert ingest.recommend(fmt, m, w, h) == want, (fmt, m, w, h)
                rc, g = _create(fmt, w, h, matrix=m, out=R.OUT_YUV420P)
                assert (rc == 0) == (want == R.OUT_YUV420P), (fmt, m, w, h)
                ingest._bind().psxhip_ingest_destroy(g)
    assert ingest._bind().psxhip_ingest_recommend(16, 0, 16, 8) == _lib.PSXHIP_EINVAL


def test_creates_rules_are_einval_and_name_the_rule():
    from psxavenc_amd import _lib
    nv12 = R.layout(R.NV12, 16, 8)[0]
    p10 = R.layout(R.YUV420P10, 16, 8)[0]
    bad = dict(
        overlapping_planes=(dict(planes=[nv12[0], (nv12[1][0] - 1, nv12[1][1])]), "overlap"),
        a_plane_inside_anothers_pitch=(dict(fmt=R.YUV420P, planes=[(0, 32), (16, 32), (8 * 32, 8)]), "overlap"),
        odd_pitch_on_a_16_bit_format=(dict(fmt=R.YUV420P10, planes=[(0, 33), (p10[1][0] + 8, 16), (p10[2][0] + 8, 16)]), "even offset and pitch"),
        odd_offset_on_a_16_bit_format=(dict(fmt=R.P010, planes=[(1, 32), (257, 32)]), "even offset and pitch"),
        odd_width_with_yuv420p=(dict(w=15, out=R.OUT_YUV420P), "even width and height"),
        odd_height_with_yuv420p=(dict(h=7, out=R.OUT_YUV420P), "even width and height"),
        bt709_with_yuv420p=(dict(matrix=R.BT709, out=R.OUT_YUV420P), "BT.601"),
        rgb_source_with_yuv420p=(dict(fmt=R.RGB24, out=R.OUT_YUV420P), "not packed RGB"),
        pitch_below_the_row=(dict(planes=[(0, 15), (128, 16)]), "below its row"),
        odd_width_packed_422=(dict(fmt=R.YUYV422, w=15), "even width"),
        unknown_format=(dict(fmt=16, planes=[(0, 64)]), "unknown source format"),
        unknown_matrix=(dict(matrix=5), "unknown matrix"),
        unknown_out_format=(dict(out=2), "out_format"),
        unknown_option=(dict(options=2), "option"),
        empty_picture=(dict(w=0), "1 .. 16384"),
        too_large=(dict(h=16385), "1 .. 16384"),
        too_few_planes=(dict(planes=[nv12[0]]), "planes"),
        null_planes=(dict(n_planes=0, planes=[]), "planes"),
    )
    for name, (kw, text) in bad.items():
        rc, g = _create(**kw)
        assert rc == _lib.PSXHIP_EINVAL and not g.value, name
        assert _error().startswith("psxhip_ingest_create:") and text in _error(), (name, _error())
    L = _mod()._bind()
    assert L.psxhip_ingest_create(None, 0, R.GRAY8, 4, 4, None, 1, 0, 0, 0, 0) == _lib.PSXHIP_EINVAL
    h_ = C.c_void_p()
    assert L.psxhip_ingest_create(C.byref(h_), 0, R.GRAY8, 4, 4, None, 1, 0, 0, 0, 0) == _lib.PSXHIP_EINVAL and "NULL" in _error()
    assert L.psxhip_ingest_matrix(None, None) == _lib.PSXHIP_EINVAL
    # what the rules allow: odd sizes for RGB24, planes in any order, touching planes
    for kw in [dict(w=15, h=7), dict(fmt=R.YUV420P, planes=[(200, 16), (0, 8), (100, 9)]), dict(fmt=R.YUV444P10, w=3, h=3, planes=[(0, 6), (18, 6), (36, 6)])]:
        rc, g = _create(**kw)
        assert rc == 0, (kw, _error())
        L.psxhip_ingest_destroy(g)


def _convert(g, src=1 << 20, src_stride=None, n_src=1, index=None, n_out=1, out=2 << 20, out_stride=None, host=False):
    """the device (or host) entry with sound arguments except those given; the addresses are never dereferenced: every case is
    decided before anything is read"""
    L = _mod()._bind()
    src_stride = L.psxhip_ingest_source_bytes(g) if src_stride is None else src_stride
    out_stride = L.psxhip_ingest_output_bytes(g) if out_stride is None else out_stride
    if host:
        return L.psxhip_ingest_convert_host(g, src, src_stride, n_src, index, n_out, out, out_stride)
    return L.psxhip_ingest_convert_device(g, src, src_stride, n_src, index, n_out, out, out_stride, None)


def test_converts_rules_are_einval_with_or_without_a_gpu():
    from psxavenc_amd import _lib
    rc, g = _create()
    rc16, g16 = _create(fmt=R.P010)
    assert rc == 0 and rc16 == 0
    for host in (False, True):
        who = "psxhip_ingest_convert_host:" if host else "psxhip_ingest_convert_device:"
        bad = dict(
            null_handle=dict(g=None, src_stride=192, out_stride=384),
            null_source=dict(src=None),
            null_output=dict(out=None),
            negative_n_out=dict(n_out=-1),
            negative_n_src=dict(n_src=-1),
            outputs_without_sources=dict(n_src=0),
            src_stride_too_small=dict(src_stride=16 * 8 * 3 // 2 - 1),
            out_stride_too_small=dict(out_stride=16 * 8 * 3 - 1),
            odd_src_stride_16_bit=dict(g=g16, src_stride=16 * 8 * 3 + 1),
        )
        for name, kw in bad.items():
            kw = dict(kw)
            handle = kw.pop("g", g)
            assert _convert(handle, host=host, **kw) == _lib.PSXHIP_EINVAL, (host, name)
            assert _error().startswith(who), (name, _error())
        assert "strides too small" in (_convert(g, host=host, src_stride=10) and _error())
        # n_out = 0: OK, nothing touched (the pointers would fault)
        assert _convert(g, host=host, n_out=0, src=None, out=None, n_src=0) == _lib.PSXHIP_OK
        assert _convert(g, host=host, n_out=0, src=8, out=8) == _lib.PSXHIP_OK
    assert _convert(g16, src=(1 << 20) + 1) == _lib.PSXHIP_EINVAL and "even source address" in _error()
    assert _convert(g, src=1 << 20, out=(1 << 20) + 100) == _lib.PSXHIP_EINVAL and "overlaps" in _error()
    assert _convert(g, src=1 << 20, n_src=3, src_stride=4096, out=(1 << 20) + 8192 + 100) == _lib.PSXHIP_EINVAL and "overlaps" in _error()
    _mod()._bind().psxhip_ingest_destroy(g)
    _mod()._bind().psxhip_ingest_destroy(g16)


def test_without_a_gpu_a_sound_conversion_fails_loudly():
    """sound arguments: PSXHIP_EDEVICE without a device, like every other entry point (with one, tests/test_gpu_ingest.py converts)"""
    import torch
    from psxavenc_amd import _lib
    if torch.cuda.is_available():
        return
    rc, g = _create()
    src, out = np.zeros(192, np.uint8), np.zeros(384, np.uint8)
    assert _convert(g, src=src.ctypes.data, out=out.ctypes.data, host=True) == _lib.PSXHIP_EDEVICE
    assert "no HIP device" in _error()
    assert _convert(g, src=src.ctypes.data, out=out.ctypes.data) == _lib.PSXHIP_EDEVICE
    _mod()._bind().psxhip_ingest_destroy(g)
