"""The device decoder end to end: encode on the device, decode on the device, compare with the oracle's reader (O.mdec_decode) and the
numpy statement of the reconstruction (tests/mdec_recon_ref.py) byte for byte; per-frame sizes, padded strides and guard bytes; the
NULL-output variants; the host entry point; the corrupted corpus (after the CPU run of the same corpus in the same tree); SSE.

Every test is one GPU step under a time limit of its own: a watchdog ends the process if a step hangs, so nothing more is started
on the device after it."""
import faulthandler
import os
import sys

import numpy as np
import pytest

import mdec_decode_corpus as DC
import mdec_recon_ref as R
from test_mdec_parse_cpu import sim  # noqa: F401  (the sanitizer build of the parse core: the corpus passes it first)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 600
GUARD = 0xA5


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _encode(torch, codec, w, h, d_frames, budget):
    from psxavenc_amd.mdec import MdecEncoder
    enc = MdecEncoder(codec, w, h, max_frame_size=budget, device=0)
    d_out, d_res = enc.encode_frames_device(d_frames, budget)
    torch.cuda.synchronize()
    enc.close()
    return d_out, d_res


def _encoder(cache, codec, w, h, budget):
    from psxavenc_amd.mdec import MdecEncoder
    key = (codec, w, h)
    if key not in cache:
        cache[key] = MdecEncoder(codec, w, h, max_frame_size=budget, device=0)
    return cache[key]


def test_geometry_matrix(oracle, torch):
    """the self-golden geometry matrix: 3 codecs x 4 sizes x 6 budgets x 3 amplitudes"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_mdec_golden import CASES
    from psxavenc_amd import MdecDecoder
    O = oracle
    decs, encs = {}, {}
    fits = 0
    for (codec, w, h, budget, amp) in CASES:
        n = 2 if w >= 640 else 4
        fr = O.synth_frames(w, h, n, seed=100 + amp, amp=amp, first=3)
        d_out, d_res = _encoder(encs, codec, w, h, 32768).encode_frames_device(torch.from_numpy(fr).cuda(), budget)
        key = (w, h, codec == 2)
        if key not in decs:
            decs[key] = MdecDecoder(w, h, dc_wrap=codec == 2)
        d_lv, d_fr, d_dec = decs[key].decode_frames_device(d_out, budget)
        torch.cuda.synchronize()
        rows, res, dec = d_out.cpu().numpy(), d_res.cpu().numpy(), d_dec.cpu().numpy()
        lv, px = d_lv.cpu().numpy(), d_fr.cpu().numpy()
        for i in range(n):
            rc, want, q, v, nbits = DC.oracle_decode(DC.Case("", w, h, codec == 2, rows[i], budget))
            assert dec[i, 0] == rc, ((codec, w, h, budget, amp), i, dec[i], rc)
            if res[i, 0] > 63:
                assert rc == -1                              # a frame that fits no scale is a zero row: no header
                continue
            fits += 1
            assert rc == 0 and tuple(dec[i]) == (0, q, v, nbits) and q == res[i, 0] and v == (2 if codec == 0 else 3)
            assert nbits <= 8 * (res[i, 1] - 8)
            assert np.array_equal(lv[i], want), (codec, w, h, budget, amp, i)
            assert np.array_equal(px[i], R.reconstruct(w, h, want, q)), (codec, w, h, budget, amp, i)
    assert fits > 500
    for d in list(decs.values()) + list(encs.values()):
        d.close()


def _big_batch(oracle, torch, codec, w, h, n, budget, amp, level_every, pixel_every):
    from psxavenc_amd import MdecDecoder, synth
    d_frames = synth.frames_device(w, h, 1, 0, n, amp, device=0)
    d_out, d_res = _encode(torch, codec, w, h, d_frames, budget)
    dec = MdecDecoder(w, h, dc_wrap=codec == 2)
    d_lv, d_fr, d_dec = dec.decode_frames_device(d_out, budget)
    torch.cuda.synchronize()
    res, got = d_res.cpu().numpy(), d_dec.cpu().numpy()
    assert (res[:, 0] <= 63).all() and (got[:, 0] == 0).all(), (res[:, 0].max(), np.unique(got[:, 0]))
    assert np.array_equal(got[:, 1], res[:, 0]) and (got[:, 2] == (2 if codec == 0 else 3)).all()
    assert (got[:, 3] <= 8 * (res[:, 1] - 8)).all()
    rows = d_out.cpu().numpy()
    sel = torch.arange(0, n, level_every, device="cuda")
    lv = dict(zip(range(0, n, level_every), d_lv[sel].cpu().numpy()))
    px = dict(zip(range(0, n, level_every), d_fr[sel].cpu().numpy()))
    for i in range(n):                                   # every frame's record; levels and pixels on their strides
        rc, want, q, v, nbits = DC.oracle_decode(DC.Case("", w, h, codec == 2, rows[i], budget))
        assert rc == 0 and tuple(got[i]) == (0, q, v, nbits), (i, got[i], (rc, q, v, nbits))
        if i % level_every == 0:
            assert np.array_equal(lv[i], want), i
        if i % pixel_every == 0:
            assert np.array_equal(px[i], R.reconstruct(w, h, want, q)), i
    dec.close()


def test_1000_frames_320x240_v2(oracle, torch):
    _big_batch(oracle, torch, 0, 320, 240, 1000, 8192, 4, level_every=1, pixel_every=4)


def test_1250_frames_640x480_v3(oracle, torch):
    _big_batch(oracle, torch, 1, 640, 480, 1250, 8192, 4, level_every=8, pixel_every=64)


def _small_batch(oracle, torch, codec=2, w=320, h=240, n=24, budget=9000, amp=8):
    fr = oracle.synth_frames(w, h, n, seed=11, amp=amp)
    d_out, d_res = _encode(torch, codec, w, h, torch.from_numpy(fr).cuda(), budget)
    return fr, d_out, d_res


def test_per_frame_sizes_padded_strides_and_guards(oracle, torch):
    from psxavenc_amd import MdecDecoder
    w, h, n, budget = 320, 240, 24, 9000
    fr, d_out, d_res = _small_batch(oracle, torch)
    res = d_res.cpu().numpy()
    fb, nblk = w * h * 3 // 2, (w // 16) * (h // 16) * 6
    # bitstream rows 64 bytes apart from each other; each frame's size is what the encoder used, everything after it is guard
    bs_stride = ((budget + 3) & ~3) + 64
    rows = np.full((n, bs_stride), GUARD, np.uint8)
    out = d_out.cpu().numpy()
    sizes = np.minimum(res[:, 1], budget).astype(np.int32)
    for i in range(n):
        rows[i, :sizes[i]] = out[i, :sizes[i]]
    d_rows = torch.from_numpy(rows).cuda()
    d_levels = torch.full((n + 2, nblk, 64), 0x5A5A, dtype=torch.int16, device="cuda")
    d_frames = torch.full((n + 2, fb + 128), GUARD, dtype=torch.uint8, device="cuda")
    d_dec = torch.full((n + 2, 4), -99, dtype=torch.int32, device="cuda")
    dec = MdecDecoder(w, h, dc_wrap=True)
    dec.decode_frames_device(d_rows, torch.from_numpy(sizes).cuda(), d_levels=d_levels[1:n + 1], d_frames=d_frames[1:n + 1, :fb],
                             d_decoded=d_dec[1:n + 1])
    torch.cuda.synchronize()
    lv, px, got = d_levels.cpu().numpy(), d_frames.cpu().numpy(), d_dec.cpu().numpy()
    assert (lv[0] == 0x5A5A).all() and (lv[-1] == 0x5A5A).all()
    assert (px[0] == GUARD).all() and (px[-1] == GUARD).all() and (px[:, fb:] == GUARD).all()
    assert (got[0] == -99).all() and (got[-1] == -99).all()
    assert np.array_equal(d_rows.cpu().numpy(), rows)
    for i in range(n):
        rc, want, q, v, nbits = DC.oracle_decode(DC.Case("", w, h, 1, rows[i], int(sizes[i])))
        assert rc == 0 and tuple(got[i + 1]) == (0, q, v, nbits)
        assert np.array_equal(lv[i + 1], want) and np.array_equal(px[i + 1, :fb], R.reconstruct(w, h, want, q))
    dec.close()


def test_null_outputs_and_host_entry_point(oracle, torch):
    from psxavenc_amd import MdecDecoder
    w, h, n, budget = 320, 240, 24, 9000
    fr, d_out, d_res = _small_batch(oracle, torch)
    dec = MdecDecoder(w, h, dc_wrap=True)
    lv, px, rec = (t.cpu().numpy() for t in dec.decode_frames_device(d_out, budget))
    assert (rec[:, 0] == 0).all()
    a, b, c = dec.decode_frames_device(d_out, budget, levels=False)          # pixels through the context's workspace
    torch.cuda.synchronize()
    assert a is None and np.array_equal(b.cpu().numpy(), px) and np.array_equal(c.cpu().numpy(), rec)
    a, b, c = dec.decode_frames_device(d_out, budget, frames=False)
    torch.cuda.synchronize()
    assert b is None and np.array_equal(a.cpu().numpy(), lv) and np.array_equal(c.cpu().numpy(), rec)
    a, b, c = dec.decode_frames_device(d_out, budget, levels=False, frames=False)      # the verify step: parse only
    torch.cuda.synchronize()
    assert a is None and b is None and np.array_equal(c.cpu().numpy(), rec)
    rows = d_out.cpu().numpy()
    wide = np.full((n, budget + 1), GUARD, np.uint8)                                     # a host stride that is not a multiple of 4
    wide[:, :budget] = rows[:, :budget]
    for sizes in (budget, np.minimum(d_res.cpu().numpy()[:, 1], budget)):
        for host_rows in (rows, wide):
            hl, hp, hr = dec.decode_frames_host(host_rows, sizes)
            assert np.array_equal(hl, lv) and np.array_equal(hp, px) and np.array_equal(hr, rec)
    hl, hp, hr = dec.decode_frames_host(rows, budget, levels=False, frames=False)
    assert hl is None and hp is None and np.array_equal(hr, rec)
    dec.close()


def test_host_entry_point_small_larger_small_on_one_handle(oracle, torch):
    """1, then 5, then 1 frame through decode_frames_host of ONE decoder, with and without pixels: the handle's staging buffers are
    allocated, outgrown and reused; each call against the oracle's reader and the numpy reconstruction"""
    from psxavenc_amd import MdecDecoder
    w, h, budget = 32, 16, 1024
    fr = oracle.synth_frames(w, h, 7, seed=21, amp=8)
    rows, res, rc = oracle.mdec_encode(0, w, h, fr, budget)
    assert rc == 0 and (res[:, 0] <= 63).all()
    want = [DC.oracle_decode(DC.Case("", w, h, False, rows[i], budget)) for i in range(7)]
    dec = MdecDecoder(w, h, dc_wrap=False)
    for pixels in (True, False, True):
        for lo, hi in ((0, 1), (1, 6), (6, 7)):
            hl, hp, hr = dec.decode_frames_host(rows[lo:hi], budget, frames=pixels)
            assert (hp is None) == (not pixels)
            for i in range(lo, hi):
                rc, levels, q, v, nbits = want[i]
                assert rc == 0 and tuple(hr[i - lo]) == (0, q, v, nbits), (pixels, lo, i)
                assert np.array_equal(hl[i - lo], levels), (pixels, lo, i)
                if pixels:
                    assert np.array_equal(hp[i - lo], R.reconstruct(w, h, levels, q)), (pixels, lo, i)
    dec.close()


def test_corrupted_corpus_on_the_device(oracle, torch, sim):  # noqa: F811
    """status against the oracle, guard bytes intact; run once, after the CPU run of the same corpus"""
    from psxavenc_amd import MdecDecoder
    cases = list(DC.corrupted_cases())
    want = [DC.oracle_decode(c) for c in cases]
    DC.check_corpus_reaches_every_error(cases, [x[0] for x in want])
    cpu = sim(cases, False)
    assert [g[0] for g in cpu] == [x[0] for x in want], "the corpus must pass on the CPU before the kernel sees it"
    groups = {}
    for k, c in enumerate(cases):
        groups.setdefault((c.w, c.h, c.wrap), []).append(k)
    seen = set()
    for (w, h, wrap), ks in sorted(groups.items()):
        n = len(ks)
        fb, nblk = w * h * 3 // 2, (w // 16) * (h // 16) * 6
        stride = ((max(cases[k].size for k in ks) + 3) & ~3) + 32
        rows = np.full((n, stride), GUARD, np.uint8)         # bytes past a frame's size are guard: a read past the size would change the status
        for r, k in enumerate(ks):
            rows[r, :cases[k].size] = cases[k].data[:cases[k].size]
        sizes = np.array([cases[k].size for k in ks], np.int32)
        d_levels = torch.full((n + 2, nblk, 64), 0x5A5A, dtype=torch.int16, device="cuda")
        d_frames = torch.full((n + 2, fb + 64), GUARD, dtype=torch.uint8, device="cuda")
        d_dec = torch.full((n + 2, 4), -99, dtype=torch.int32, device="cuda")
        dec = MdecDecoder(w, h, dc_wrap=bool(wrap))
        dec.decode_frames_device(torch.from_numpy(rows).cuda(), torch.from_numpy(sizes).cuda(), d_levels=d_levels[1:n + 1],
                                 d_frames=d_frames[1:n + 1, :fb], d_decoded=d_dec[1:n + 1])
        torch.cuda.synchronize()
        lv, px, got = d_levels.cpu().numpy(), d_frames.cpu().numpy(), d_dec.cpu().numpy()
        assert (lv[0] == 0x5A5A).all() and (lv[-1] == 0x5A5A).all()
        assert (px[0] == GUARD).all() and (px[-1] == GUARD).all() and (px[:, fb:] == GUARD).all()
        assert (got[0] == -99).all() and (got[-1] == -99).all()
        for r, k in enumerate(ks):
            rc, levels, q, v, nbits = want[k]
            assert got[r + 1, 0] == rc, (cases[k].name, got[r + 1], rc)
            seen.add(int(rc))
            if rc == 0:
                assert tuple(got[r + 1]) == (0, q, v, nbits) and np.array_equal(lv[r + 1], levels), cases[k].name
                assert np.array_equal(px[r + 1, :fb], R.reconstruct(w, h, levels, q)), cases[k].name
            else:
                assert got[r + 1, 3] == 0 and (px[r + 1] == GUARD).all(), cases[k].name      # a frame that does not parse leaves its pixels alone
        dec.close()
    assert seen == DC.REACHABLE[2] | DC.REACHABLE[3]


def test_sse_against_numpy(oracle, torch):
    from psxavenc_amd import MdecDecoder, decode, psnr
    w, h, n, budget = 320, 240, 24, 9000
    fr, d_out, d_res = _small_batch(oracle, torch)
    dec = MdecDecoder(w, h, dc_wrap=True)
    _, d_px, _ = dec.decode_frames_device(d_out, budget, levels=False)
    d_src = torch.from_numpy(fr).cuda()
    got = decode.sse_device(d_px, d_src, w, h).cpu().numpy()
    want = R.sse(w, h, d_px.cpu().numpy(), fr)
    assert np.array_equal(got.astype(np.uint64), want) and (want[:, 0] > 0).all()
    db = psnr(got, w, h)[:, 0]                           # luma of quantised noise: lossy, and not ruined
    assert (db > 20).all() and (db < 70).all(), db
    dec.close()
    # extremes, a padded stride, a single macroblock and the largest frame: 255^2 per sample must not overflow anything
    for (w, h, n) in ((16, 16, 5), (1024, 1024, 3), (320, 240, 7)):
        fb = w * h * 3 // 2
        a = torch.zeros((n, fb + 36), dtype=torch.uint8, device="cuda")
        b = torch.full((n, fb + 36), 255, dtype=torch.uint8, device="cuda")
        a[:, fb:] = 77                                                       # the padding is not part of any frame
        got = decode.sse_device(a[:, :fb], b[:, :fb], w, h).cpu().numpy()
        assert np.array_equal(got, np.tile(np.array([w * h, w * h // 4, w * h // 4], np.int64) * 255 * 255, (n, 1)))
        assert np.array_equal(decode.sse_device(b[:, :fb], b[:, :fb], w, h).cpu().numpy(), np.zeros((n, 3), np.int64))
        rng = np.random.default_rng(w)
        x, y = rng.integers(0, 256, (n, fb + 36), dtype=np.uint8), rng.integers(0, 256, (n, fb + 36), dtype=np.uint8)
        got = decode.sse_device(torch.from_numpy(x).cuda()[:, :fb], torch.from_numpy(y).cuda()[:, :fb], w, h).cpu().numpy()
        assert np.array_equal(got.astype(np.uint64), R.sse(w, h, x, y))
