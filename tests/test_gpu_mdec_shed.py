"""psxhip_mdec_refine_frames_device ("psxhip MDEC shed v1") on the device, held to the numpy statement (tests/mdec_shed_ref.py) on the
corpus of tests/mdec_shed_corpus.py: launches of 1 frame, of 13 frames with a budget each, of 6 frames with one odd budget and of 2
frames of 320x240, for v2, v3 and v3dc.  The statement itself is checked against brute force in tests/test_mdec_shed_ref.py and the
C++ core under the host sanitizers in tests/test_mdec_shed_core_cpu.py.

The corpus refines frames in magnitude class 1 only (its first fits in classes 2 and 3 are declined), so the emit kernel's rows are
checked on the device for steps of class 1; the decisions are checked for all three classes.

Every test is one GPU step under a time limit of its own: a watchdog ends the process if a step hangs, so nothing more is started on the
device after it."""
import faulthandler

import numpy as np
import pytest

import mdec_shed_corpus as C

pytestmark = pytest.mark.gpu

STEP_SECONDS = 300
GUARD = 0xA5
FRAME_PAD, ROW_PAD = 64, 32


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def encoders():
    """one encoder context per group, kept for the module"""
    from psxavenc_amd.mdec import MdecEncoder
    cache = {}

    def get(gi):
        g = C.groups()[gi]
        if gi not in cache:
            cache[gi] = MdecEncoder(g.codec, g.w, g.h, max_frame_size=g.max_size, device=0)
        return cache[gi]
    yield get
    for e in cache.values():
        e.close()


class Buffers:
    """a group's frames, rows and results in device memory, with padded strides whose padding holds GUARD"""

    def __init__(self, torch, g, stream, budgets=None):
        fb = g.frames.shape[1]
        self.ostride = ((g.max_size + 3) & ~3) + ROW_PAD
        with torch.cuda.stream(stream):
            self.frames = torch.full((g.n, fb + FRAME_PAD), GUARD, dtype=torch.uint8, device="cuda:0")
            self.frames[:, :fb] = torch.from_numpy(g.frames).to("cuda:0")
            self.out = torch.full((g.n, self.ostride), GUARD, dtype=torch.uint8, device="cuda:0")
            self.res = torch.zeros((g.n, 4), dtype=torch.int32, device="cuda:0")
            b = g.budgets if budgets is None else budgets
            self.sizes = g.uniform if (g.uniform is not None and budgets is None) else torch.from_numpy(np.asarray(b, np.int32)).to("cuda:0")
        self.budgets = np.asarray(b)


def _encode_refine(torch, enc, g, K, with_records, stream, lanes=1, budgets=None):
    """encode, then refine, on `stream`, with nothing in between but a copy of the plain rows on the same stream (one lane only: with
    two, only the refinement orders itself behind the encode).  Returns (buffers, plain rows or None, plain results or None, records)"""
    bufs = Buffers(torch, g, stream, budgets)
    enc.set_lanes(lanes)
    enc.encode_frames_device(bufs.frames, bufs.sizes, d_out=bufs.out, d_results=bufs.res, stream=stream)
    plain = plain_res = None
    if lanes == 1:
        with torch.cuda.stream(stream):
            plain, plain_res = bufs.out.clone(), bufs.res.clone()
    rec = enc.refine_frames_device(bufs.frames, bufs.sizes, bufs.out, bufs.res, max_magnitude=K, stream=stream, want_refine=with_records)
    stream.synchronize()
    enc.set_lanes(1)
    return bufs, plain, plain_res, rec


@pytest.mark.parametrize("lanes", (1, 2))
@pytest.mark.parametrize("with_records", (True, False), ids=("records", "no_records"))
@pytest.mark.parametrize("K", C.KS)
def test_rows_results_and_records_equal_the_statement(torch, encoders, K, with_records, lanes):
    """fails without the refinement: the library has no psxhip_mdec_refine_frames_device"""
    from psxavenc_amd.mdec import refine_records
    stream = torch.cuda.Stream(device="cuda:0")
    refined = 0
    for gi, g in enumerate(C.groups()):
        want_rows, want_res, want_rec = C.expected(gi, K)
        bufs, plain, plain_res, rec = _encode_refine(torch, encoders(gi), g, K, with_records, stream, lanes)
        out, res = bufs.out.cpu().numpy(), bufs.res.cpu().numpy()
        assert np.array_equal(res, want_res), (g.name, res, want_res)
        for i in range(g.n):                                 # all frame_max_size bytes of every row, and nothing behind them
            b = int(g.budgets[i])
            assert np.array_equal(out[i, :b], want_rows[i, :b]), (g.name, i)
            assert (out[i, b:] == GUARD).all(), (g.name, i)
        assert (bufs.frames.cpu().numpy()[:, g.frames.shape[1]:] == GUARD).all()
        if with_records:
            assert np.array_equal(refine_records(rec.cpu().numpy()), want_rec), (g.name, refine_records(rec.cpu().numpy()), want_rec)
        else:
            assert rec is None
        if plain is not None:                                # untouched and declined frames: bit for bit the plain encode's
            keep = want_rec[:, 0] == 0
            assert np.array_equal(out[keep], plain.cpu().numpy()[keep]) and np.array_equal(res[keep], plain_res.cpu().numpy()[keep]), g.name
            assert np.array_equal(plain_res.cpu().numpy(), C.plain(gi)[1]), g.name
        refined += int((want_rec[:, 0] != 0).sum())
    assert refined >= 20


def test_device_decoder_reads_every_refined_row(torch, encoders):
    from psxavenc_amd import MdecDecoder
    stream = torch.cuda.Stream(device="cuda:0")
    K = 3
    for gi, g in enumerate(C.groups()):
        bufs, plain, _, _ = _encode_refine(torch, encoders(gi), g, K, False, stream)
        dec = MdecDecoder(g.w, g.h, dc_wrap=g.codec == 2)
        sizes = torch.from_numpy(g.budgets.astype(np.int32)).to("cuda:0")
        d_lv, _, d_dec = dec.decode_frames_device(bufs.out, sizes, frames=False)
        d_lv0, _, _ = dec.decode_frames_device(plain, sizes, frames=False)
        torch.cuda.synchronize()
        lv, lv0, rep = d_lv.cpu().numpy(), d_lv0.cpu().numpy(), d_dec.cpu().numpy()
        for i in range(g.n):
            o = C.outcome(gi, i, K)
            if o.state != "refined":
                continue
            assert rep[i].tolist() == [0, o.M, 2 if g.codec == 0 else 3, int(o.bits[o.step])], (g.name, i, rep[i])
            assert np.array_equal(lv[i][:, 1:], o.lv[:, 1:]) and np.array_equal(lv[i][:, 0], lv0[i][:, 0]), (g.name, i)
        dec.close()


def test_host_entry_gives_the_device_pair_s_bytes(torch, encoders):
    K = 2
    for gi, g in enumerate(C.groups()):
        want_rows, want_res, want_rec = C.expected(gi, K)
        keep = want_res[:, 0] != 64                          # (a frame that fits no scale makes the call PSXHIP_ENOFIT: below)
        sizes = g.uniform if g.uniform is not None else g.budgets[keep]
        out, res, rec = encoders(gi).encode_refine_frames_host(g.frames[keep], sizes, max_magnitude=K)
        assert np.array_equal(res, want_res[keep]) and np.array_equal(rec, want_rec[keep]), g.name
        for k, i in enumerate(np.flatnonzero(keep)):
            assert np.array_equal(out[k, :g.budgets[i]], want_rows[i, :g.budgets[i]]), (g.name, i)


def test_host_entry_reports_a_frame_that_fits_no_scale(encoders):
    from psxavenc_amd import _lib
    gi = next(i for i, g in enumerate(C.groups()) if (C.plain(i)[1][:, 0] == 64).any())
    g = C.groups()[gi]
    with pytest.raises(_lib.PsxHipError) as e:
        encoders(gi).encode_refine_frames_host(g.frames, g.budgets, max_magnitude=1)
    assert e.value.code == _lib.PSXHIP_ENOFIT


def test_refined_frames_gain_in_pixels(torch, encoders):
    """sum of SSE (psxhip_mdec_sse_device, reconstruction by the device decoder) over the refined frames against the plain encodes'"""
    from psxavenc_amd import MdecDecoder
    from psxavenc_amd.decode import sse_device
    stream = torch.cuda.Stream(device="cuda:0")
    K = 1
    total_plain = total_shed = 0
    for gi, g in enumerate(C.groups()):
        refined = np.array([C.outcome(gi, i, K).state == "refined" for i in range(g.n)])
        if not refined.any():
            continue
        bufs, plain, _, _ = _encode_refine(torch, encoders(gi), g, K, False, stream)
        dec = MdecDecoder(g.w, g.h, dc_wrap=g.codec == 2)
        sizes = torch.from_numpy(g.budgets.astype(np.int32)).to("cuda:0")
        px = [torch.zeros_like(bufs.frames) for _ in range(2)]
        for rows, dst in ((plain, px[0]), (bufs.out, px[1])):
            _, _, d_dec = dec.decode_frames_device(rows, sizes, levels=False, d_frames=dst)
        sse = [sse_device(bufs.frames, p, g.w, g.h).cpu().numpy().sum(axis=1) for p in px]
        torch.cuda.synchronize()
        total_plain += int(sse[0][refined].sum())
        total_shed += int(sse[1][refined].sum())
        dec.close()
    print("sum of SSE over the refined frames: %d (plain %d)" % (total_shed, total_plain))
    assert 0 < total_shed < total_plain


def test_frame_with_a_budget_out_of_range_is_left_as_it_was(torch, encoders):
    from psxavenc_amd.mdec import refine_records
    stream = torch.cuda.Stream(device="cuda:0")
    gi = next(i for i, g in enumerate(C.groups()) if g.n == 13)
    g = C.groups()[gi]
    budgets = g.budgets.copy()
    want_rows, want_res, want_rec = C.expected(gi, 1)
    victims = [i for i in range(g.n) if want_rec[i, 0] != 0][:3]
    assert len(victims) == 3
    budgets[victims[0]], budgets[victims[1]], budgets[victims[2]] = 4, g.max_size + 4, -1
    bufs, plain, plain_res, rec = _encode_refine(torch, encoders(gi), g, 1, True, stream, budgets=budgets)
    out, res, rec = bufs.out.cpu().numpy(), bufs.res.cpu().numpy(), refine_records(rec.cpu().numpy())
    for i in range(g.n):
        if i in victims:
            assert np.array_equal(out[i], plain.cpu().numpy()[i]) and np.array_equal(res[i], plain_res.cpu().numpy()[i]) and not rec[i].any(), i
            assert (out[i] == GUARD).all()
        else:
            assert np.array_equal(res[i], want_res[i]) and np.array_equal(rec[i], want_rec[i]), i
            assert want_res[i, 0] == 64 or np.array_equal(out[i, :budgets[i]], want_rows[i, :budgets[i]]), i


def test_no_frames_touches_nothing(torch, encoders):
    from psxavenc_amd import _lib
    gi = 0
    g = C.groups()[gi]
    enc = encoders(gi)
    bufs = Buffers(torch, g, torch.cuda.current_stream())
    rec = torch.full((g.n, 3), -1, dtype=torch.int64, device="cuda:0")
    rc = _lib.lib().psxhip_mdec_refine_frames_device(enc._h, bufs.frames.data_ptr(), bufs.frames.stride(0), 0, None, g.max_size, 3,
                                                     bufs.out.data_ptr(), bufs.out.stride(0), bufs.res.data_ptr(), rec.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert (bufs.out == GUARD).all() and (bufs.res == 0).all() and (rec == -1).all()
