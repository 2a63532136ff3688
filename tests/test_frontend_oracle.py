"""The CPU checker of the colour-conversion / scaling front-end (oracle/frontend_oracle.c) against what can
be known without libswscale (parity with the reference's scaler is UNPINNED -- FFmpeg is absent): the filter bank's
invariants, exact identities, and closeness to a double-precision bicubic + BT.601 full-range model.  Tolerances are the
fixed-point format's: 14-bit coefficients, 15-bit intermediates.  On hard content the statement is held to the float64 model of
tests/scaler_model.py within a bound derived from each geometry's banks; impulses pin the banks' placement exactly."""
import numpy as np
import pytest

import scaler_model as M


def _cubic(x, B=0.0, Cc=0.6):
    x = np.abs(x)
    w1 = ((12 - 9 * B - 6 * Cc) * x ** 3 + (-18 + 12 * B + 6 * Cc) * x ** 2 + (6 - 2 * B)) / 6
    w2 = ((-B - 6 * Cc) * x ** 3 + (6 * B + 30 * Cc) * x ** 2 + (-12 * B - 48 * Cc) * x + (8 * B + 24 * Cc)) / 6
    return np.where(x < 1, w1, np.where(x < 2, w2, 0.0))


def _float_scale(plane, dw, dh):
    """double-precision separable bicubic with the same geometry (centres, support widening, edge replication)"""
    def one(p, d):
        s = p.shape[1]
        ratio = s / d
        scale = max(1.0, ratio)
        out = np.zeros((p.shape[0], d))
        for i in range(d):
            c = (i + 0.5) * ratio - 0.5
            lo = int(np.floor(c - 2 * scale)) + 1
            ks = np.arange(lo, lo + int(np.ceil(4 * scale)) + 1)
            w = _cubic((ks - c) / scale)
            w /= w.sum()
            out[:, i] = (p[:, np.clip(ks, 0, s - 1)] * w).sum(axis=1)
        return out
    return one(one(plane.astype(np.float64), dw).T, dh).T


@pytest.mark.parametrize("src,dst", [(640, 320), (320, 320), (352, 320), (1280, 320), (160, 320), (720, 304), (853, 320), (17, 16)])
def test_filter_bank_invariants(oracle, src, dst):
    taps, left, coef = oracle.scaler_filter(src, dst)
    assert (coef.astype(np.int64).sum(axis=1) == 16384).all()
    ratio = max(1.0, src / dst)
    assert taps == int(np.ceil(4 * ((src * 65536 + dst // 2) // dst if src > dst else 65536) / 65536)) or taps >= 4
    centres = (np.arange(dst) + 0.5) * src / dst - 0.5
    assert (left <= np.floor(centres)).all() and (left + taps - 1 >= np.floor(centres)).all()
    # against the real-valued kernel: quantisation to 14 bits, and positions that advance by a 16.16 increment (as
    # libswscale's do): up to dst * 2^-17 source pixels off at the far end
    for i in (0, dst // 3, dst - 1):
        ks = left[i] + np.arange(taps)
        w = _cubic((ks - centres[i]) / ratio)
        w = w / w.sum() * 16384
        assert np.abs(coef[i] - w).max() < 12 + 16384 * 1.5 * dst / 131072, (i, coef[i], w)
    if src == dst:
        assert (coef.max(axis=1) == 16384).all()          # identity: one tap of weight 1


def test_identity_geometry_is_exact(oracle):
    """same size in and out: YUV420P full range comes back byte for byte (as NV21); RGB grey ramps give Y = the grey"""
    rng = np.random.default_rng(1)
    w, h = 64, 48
    pic = rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8)
    out = oracle.scaler_convert(oracle.PIX_YUV420P, w, h, True, w, h, pic[None])[0]
    assert np.array_equal(out[:w * h], pic[:w * h])
    u, v = pic[w * h:w * h + w * h // 4], pic[w * h + w * h // 4:]
    assert np.array_equal(out[w * h::2], v) and np.array_equal(out[w * h + 1::2], u)        # NV21: Cr first
    grey = np.repeat(np.tile(np.arange(w, dtype=np.uint8) * 4, h)[:, None], 3, axis=1).reshape(-1)
    out = oracle.scaler_convert(oracle.PIX_RGB24, w, h, True, w, h, grey[None])[0]
    assert np.array_equal(out[:w * h], np.tile(np.arange(w, dtype=np.uint8) * 4, h))
    assert (out[w * h:] == 128).all()


@pytest.mark.parametrize("fmt,sw,sh,dw,dh", [(0, 640, 480, 320, 240), (1, 640, 480, 320, 240), (1, 352, 288, 320, 240), (0, 200, 150, 320, 240),
                                             (1, 1280, 720, 320, 176)])
def test_close_to_the_real_valued_model(oracle, fmt, sw, sh, dw, dh):
    """|fixed point - double| <= 1 everywhere and < 0.6 in the mean: what 14-bit coefficients and a 15-bit intermediate give"""
    rng = np.random.default_rng(sw + dw)
    yy, xx = np.mgrid[0:sh, 0:sw]
    base = (96 + 64 * np.sin(xx / 17.0) * np.cos(yy / 23.0) + 40 * ((xx // 32 + yy // 32) % 2)).astype(np.float64)
    if fmt == 0:
        rgb = np.stack([np.clip(base + rng.integers(-6, 7, base.shape), 0, 255), np.clip(base * 0.8 + 20, 0, 255),
                        np.clip(255 - base, 0, 255)], axis=-1).astype(np.uint8)
        out = oracle.scaler_convert(fmt, sw, sh, True, dw, dh, rgb.reshape(1, -1))[0]
        r, g, b = (rgb[..., k].astype(np.float64) for k in range(3))
        # the model scales the same 8-bit planes the integer path builds (the colour matrix's own rounding is checked apart)
        y8 = np.floor((19595 * r + 38470 * g + 7471 * b + 32768) / 65536)
        cb8 = np.clip(np.floor((-11059 * r - 21709 * g + 32768 * b + 32768) / 65536) + 128, 0, 255)
        cr8 = np.clip(np.floor((32768 * r - 27439 * g - 5329 * b + 32768) / 65536) + 128, 0, 255)
        assert np.abs(y8 - (0.299 * r + 0.587 * g + 0.114 * b)).max() <= 1.0
        assert np.abs(cb8 - (128 - 0.168736 * r - 0.331264 * g + 0.5 * b)).max() <= 1.0
        planes = [(y8, dw, dh), (cr8, dw // 2, dh // 2), (cb8, dw // 2, dh // 2)]
    else:
        y = np.clip(base + rng.integers(-6, 7, base.shape), 0, 255).astype(np.uint8)
        u = np.clip(128 + 40 * np.sin(xx[::2, ::2] / 29.0), 0, 255).astype(np.uint8)
        v = np.clip(128 - 50 * np.cos(yy[::2, ::2] / 31.0), 0, 255).astype(np.uint8)
        out = oracle.scaler_convert(fmt, sw, sh, True, dw, dh, np.concatenate([y.ravel(), u.ravel(), v.ravel()])[None])[0]
        planes = [(y.astype(np.float64), dw, dh), (v.astype(np.float64), dw // 2, dh // 2), (u.astype(np.float64), dw // 2, dh // 2)]
    got = [out[:dw * dh].reshape(dh, dw), out[dw * dh::2].reshape(dh // 2, dw // 2), out[dw * dh + 1::2].reshape(dh // 2, dw // 2)]
    for (p, w_, h_), g_ in zip(planes, got):
        want = np.clip(_float_scale(p, w_, h_), 0, 255)
        err = np.abs(g_.astype(np.float64) - want)
        assert err.max() <= 1.0 + 1e-9 and err.mean() < 0.6, (err.max(), err.mean())


def test_limited_range_input_expands_to_full_range(oracle):
    """MPEG-range YUV (16..235 / 16..240) -> the full range the encoder expects (decoding.c:301-311: dst range = JPEG)"""
    w, h = 64, 32
    for yv, want in ((16, 0), (235, 255), (126, 128)):
        pic = np.concatenate([np.full(w * h, yv, np.uint8), np.full(w * h // 2, 128, np.uint8)])
        out = oracle.scaler_convert(oracle.PIX_YUV420P, w, h, False, w, h, pic[None])[0]
        assert abs(int(out[0]) - want) <= 1 and (out[:w * h] == out[0]).all()
        assert (np.abs(out[w * h:].astype(int) - 128) <= 1).all()
    pic = np.concatenate([np.full(w * h, 128, np.uint8), np.full(w * h // 4, 240, np.uint8), np.full(w * h // 4, 16, np.uint8)])
    out = oracle.scaler_convert(oracle.PIX_YUV420P, w, h, False, w, h, pic[None])[0]
    assert (out[w * h::2] <= 1).all() and (out[w * h + 1::2] >= 254).all()       # Cr from V = 16, Cb from U = 240


# ---------------------------------------------------------------- hard content against the float64 model (tests/scaler_model.py)
@pytest.mark.parametrize("fmt,sw,sh,full,dw,dh", M.TILE_GEOMETRIES + M.EXTREME_GEOMETRIES)
def test_hard_content_within_the_derived_bound(oracle, fmt, sw, sh, full, dw, dh):
    """the CPU statement against the real-valued model on content that drives every clamp: per plane within the bound the
    geometry's own banks allow (scaler_model.plane_bound, derived, not fitted), and on noise unbiased to within 0.05 with a
    mean error of a rounding (about 0.25): a wrong rounding constant moves both to about 0.5"""
    bounds = M.convert_bounds(fmt, sw, sh, full, dw, dh, oracle.scaler_filter)
    pics = M.hard_pictures(fmt, sw, sh, dw, dh, limited=not full, seed=sw * 7 + dh, kinds=M.kinds_for(sw, sh))
    for name, pic in pics:
        out = oracle.scaler_convert(fmt, sw, sh, full, dw, dh, pic[None])[0]
        got, want = M.nv21_planes(out, dw, dh), M.model_convert(fmt, sw, sh, full, dw, dh, pic)
        for plane, g, w, b in zip(("Y", "Cr", "Cb"), got, want, (bounds[0], bounds[1], bounds[1])):
            err = np.abs(g - w).max()
            assert err <= b, "%s, plane %s: max |err| %.3f over the bound %.3f" % (name, plane, err, b)
        if name == "noise":
            d = np.concatenate([(g - w).ravel() for g, w in zip(got, want)])
            assert np.abs(d).mean() <= 0.30 and abs(d.mean()) <= 0.05, (np.abs(d).mean(), d.mean())


def _impulse_spec(taps, left, coef, n_src, p):
    """sum of the bank's coefficients that land on source sample p (edge replication), per output: int64"""
    idx = np.clip(left[:, None].astype(np.int64) + np.arange(taps)[None, :], 0, n_src - 1)
    return (coef.astype(np.int64) * (idx == p)).sum(axis=1)


@pytest.mark.parametrize("sw,sh,dw,dh", [(4096, 256, 256, 16), (2, 2, 1024, 1024)])
def test_impulse_response_is_the_bank(oracle, sw, sh, dw, dh):
    """one sample of 255 in a black plane (Y, and V under it), at the first, middle and last column and row: every output byte
    is the specification evaluated for that one sample from scaler_filter's bank -- a shifted `left`, or a tap applied to the
    wrong source column, fails.  16x down: 64-tap banks; 2 -> 1024: `left` runs below 0 and past the end."""
    lh, lv = oracle.scaler_filter(sw, dw), oracle.scaler_filter(sh, dh)
    ch, cv = oracle.scaler_filter(sw // 2, dw // 2), oracle.scaler_filter(sh // 2, dh // 2)

    def plane(hb, vb, n_w, n_h, p, q):
        a = _impulse_spec(*hb, n_w, p)
        b = _impulse_spec(*vb, n_h, q)
        t = np.clip((255 * a) >> 7, 0, 32767)
        return np.clip((b[:, None] * t[None, :] + (1 << 20)) >> 21, 0, 255)

    for p in sorted({0, sw // 2, sw - 1}):
        for q in sorted({0, sh // 2, sh - 1}):
            y = np.zeros((sh, sw), np.uint8)
            u = np.zeros((sh // 2, sw // 2), np.uint8)
            v = np.zeros((sh // 2, sw // 2), np.uint8)
            y[q, p] = 255
            v[q // 2, p // 2] = 255
            pic = np.concatenate([y.ravel(), u.ravel(), v.ravel()])
            out = oracle.scaler_convert(oracle.PIX_YUV420P, sw, sh, True, dw, dh, pic[None])[0]
            gy, gcr, gcb = M.nv21_planes(out, dw, dh)
            assert np.array_equal(gy, plane(lh, lv, sw, sh, p, q)), (p, q)
            assert np.array_equal(gcr, plane(ch, cv, sw // 2, sh // 2, p // 2, q // 2)), (p, q)
            assert (gcb == 0).all()


def test_acceptance_is_sixteen_times_per_bank(oracle):
    """a bank exists exactly when its 16.16 increment is at most 16 (64 taps); RGB chroma is filtered from full resolution to
    half the target, so RGB 2560x1440 -> 320x240 is accepted (chroma 2560 -> 160: exactly 16x) and 2561x1441 -> 320x240 is
    refused by its chroma bank although luma shrinks only 8x"""
    for src, dst in ((1024, 64), (1025, 64), (1039, 64), (1040, 64), (1041, 64), (2560, 160), (2561, 160), (16384, 1024), (16385, 1024),
                     (16384, 1023), (4096, 256), (4104, 256), (4105, 256)):
        assert oracle.scaler_filter_accepts(src, dst) == (M.xinc(src, dst) <= 16 * 65536), (src, dst)

    def banks(fmt, sw, sh, dw, dh):
        csw, csh = (sw, sh) if fmt == 0 else (sw // 2, sh // 2)
        return [(sw, dw), (sh, dh), (csw, dw // 2), (csh, dh // 2)]

    assert all(oracle.scaler_filter_accepts(s, d) for s, d in banks(0, 2560, 1440, 320, 240))
    refused = [k for k, (s, d) in enumerate(banks(0, 2561, 1441, 320, 240)) if not oracle.scaler_filter_accepts(s, d)]
    assert refused == [2], refused        # the chroma horizontal bank alone
    assert M.xinc(2561, 320) <= 8 * 65536 + 65536 // 8
