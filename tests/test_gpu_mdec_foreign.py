"""The device BS decoder on streams of an independent writer (tests/mdec_foreign_streams.py): escapes for coded pairs, escape level 0,
level +511, quant scales over the whole 16-bit field, coefficients that saturate, v3 DCs of every size class and past ten and
sixteen bits, blocks of 63 escapes and of DC + end of block.  Records and levels against what was written, pixels against the numpy
statement (tests/mdec_recon_ref.py) byte for byte and against a float64 IDCT within the statement's own bound; guard rows and guard
bytes round everything the kernels write.  The corpus passes the CPU build of the parse core (under the host sanitizers, as a
program of its own) before the kernel sees it.

Every test is one GPU step under a time limit of its own, as in tests/test_gpu_mdec_decode.py."""
import faulthandler

import numpy as np
import pytest

import mdec_decode_corpus as DC
import mdec_foreign_streams as FS
import mdec_recon_ref as R
from test_mdec_parse_cpu import sim  # noqa: F401  (the sanitizer build of the parse core: the corpus passes it first)

pytestmark = pytest.mark.gpu

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


def _decode_groups(torch, cases):
    """One decoder and one launch per (w, h, wrap): per-frame sizes, bytes past each frame's size are guard, a guard row before and
    after the levels, pixels and records, guard bytes after every row of pixels.  Returns per case (record, levels, pixels row
    with its guard bytes), after checking the guards and that the input rows are unchanged."""
    from psxavenc_amd import MdecDecoder
    groups = {}
    for k, c in enumerate(cases):
        groups.setdefault((c.w, c.h, c.wrap), []).append(k)
    out = [None] * len(cases)
    for (w, h, wrap), ks in sorted(groups.items()):
        n = len(ks)
        fb, nblk = w * h * 3 // 2, (w // 16) * (h // 16) * 6
        stride = ((max(cases[k].size for k in ks) + 3) & ~3) + 32
        rows = np.full((n, stride), GUARD, np.uint8)
        for r, k in enumerate(ks):
            rows[r, :cases[k].size] = cases[k].data[:cases[k].size]
        sizes = np.array([cases[k].size for k in ks], np.int32)
        d_rows = torch.from_numpy(rows).cuda()
        d_levels = torch.full((n + 2, nblk, 64), 0x5A5A, dtype=torch.int16, device="cuda")
        d_frames = torch.full((n + 2, fb + 64), GUARD, dtype=torch.uint8, device="cuda")
        d_dec = torch.full((n + 2, 4), -99, dtype=torch.int32, device="cuda")
        dec = MdecDecoder(w, h, dc_wrap=bool(wrap))
        dec.decode_frames_device(d_rows, torch.from_numpy(sizes).cuda(), d_levels=d_levels[1:n + 1], d_frames=d_frames[1:n + 1, :fb],
                                 d_decoded=d_dec[1:n + 1])
        torch.cuda.synchronize()
        lv, px, got = d_levels.cpu().numpy(), d_frames.cpu().numpy(), d_dec.cpu().numpy()
        dec.close()
        assert (lv[0] == 0x5A5A).all() and (lv[-1] == 0x5A5A).all()
        assert (px[0] == GUARD).all() and (px[-1] == GUARD).all() and (px[:, fb:] == GUARD).all()
        assert (got[0] == -99).all() and (got[-1] == -99).all()
        assert np.array_equal(d_rows.cpu().numpy(), rows)
        for r, k in enumerate(ks):
            out[k] = (tuple(int(x) for x in got[r + 1]), lv[r + 1], px[r + 1])
    return out


def _check_clean(pairs, got):
    for (c, want), (rec, lv, px) in zip(pairs, got):
        fb = c.w * c.h * 3 // 2
        assert rec == (0, want[2], want[3], want[4]), (c.name, rec, want[2:])
        assert np.array_equal(lv, want[1]), c.name
        assert np.array_equal(px[:fb], R.reconstruct(c.w, c.h, want[1], want[2])), c.name


def _sim_first(sim, pairs):
    cases = [c for c, _ in pairs]
    cpu = sim(cases, True, windowed=True)
    for (c, want), g in zip(pairs, cpu):
        assert g[0] == 0 and (g[2], g[3], g[4]) == want[2:] and np.array_equal(g[1], want[1]), \
            "the corpus must pass on the CPU before the kernel sees it: " + c.name
    return cases


@pytest.fixture(scope="module")
def decoded(torch, sim):  # noqa: F811
    """the whole clean corpus through the device once, shared by the tests that look at it"""
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    try:
        pairs = FS.clean_cases()
        return pairs, _decode_groups(torch, _sim_first(sim, pairs))
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_foreign_streams_decode_to_what_was_written(decoded):
    pairs, got = decoded
    assert len(pairs) == len(got) == 1260 and {(c.w, c.h, c.wrap) for c, _ in pairs} == {(w, h, wr) for (w, h) in FS.SIZES for wr in (0, 1)}
    _check_clean(pairs, got)


def test_foreign_negative_cases_on_the_device(oracle, torch, sim):  # noqa: F811
    """statuses as the oracle gives them; the pixels of a frame that does not parse are left alone"""
    pairs = FS.negative_cases()
    cases = [c for c, _ in pairs]
    want = [DC.oracle_decode(c) for c in cases]
    assert all(s is None or s == o[0] for (_, s), o in zip(pairs, want))
    cpu = sim(cases, False, windowed=True)
    assert [g[0] for g in cpu] == [o[0] for o in want], "the corpus must pass on the CPU before the kernel sees it"
    got = _decode_groups(torch, cases)
    seen = set()
    for c, o, (rec, lv, px) in zip(cases, want, got):
        assert o[0] != 0 and rec == (o[0], o[2], o[3], 0), (c.name, rec, o[0])
        assert (px == GUARD).all(), c.name
        seen.add(o[0])
    assert {-3, -6, -7} <= seen and -8 not in seen


def test_reconstruction_at_saturation_against_float64(decoded):
    """what the kernel wrote, against clip(rint(float64 IDCT of the saturated coefficients + 128)), within the statement's derived
    bound per block: every case, and the saturating blocks counted per header scale"""
    pairs, got = decoded
    worst, largest, nsat, nclean = 0, 0, {}, 0
    for (c, want), (rec, lv, px) in zip(pairs, got):
        qs = want[2]
        f8 = R.dequantise(want[1], qs)
        bound = R.pixel_bound(f8)
        real = R.place(c.w, c.h, R.real_pixels(f8)).astype(np.int64)
        limit = R.place(c.w, c.h, np.minimum(np.broadcast_to(bound[:, None, None], f8.shape), 255)).astype(np.int64)
        d = np.abs(px[:c.w * c.h * 3 // 2].astype(np.int64) - real)
        assert (d <= limit).all(), (c.name, int(d.max()), int(limit.max()))
        sat = R.saturating_blocks(want[1], qs)
        nsat[qs] = nsat.get(qs, 0) + int(sat.sum())
        nclean += int((~sat).sum())
        if sat.any():
            worst, largest = max(worst, int(d.max())), max(largest, int(bound.max()))
    print("device vs float64 on saturating frames: worst |difference| %d, largest bound %d; saturating blocks per scale %s" % (worst, largest, sorted(nsat.items())))
    assert all(nsat[qs] > 0 for qs in FS.SCALES if qs >= 63) and nclean > 0


def test_320x240_frames_of_63_escapes_per_block_and_of_empty_blocks(torch, sim):  # noqa: F811
    """many workgroups and the longest serial walks in one launch each: 1800 blocks of up to 1404 bits, and 1800 of 12"""
    pairs = FS.large_cases()
    assert sorted(c.written.cls for c, _ in pairs) == ["dense", "dense", "empty"]
    bits = {n for c, _ in pairs for n in c.written.block_bits}
    assert 12 in bits and 1404 in bits
    _check_clean(pairs, _decode_groups(torch, _sim_first(sim, pairs)))
