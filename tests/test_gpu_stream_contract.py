"""Every device entry point held to "asynchronous on `stream`" (include/psxav_hip.h) and the Python layer to its `stream=` argument.

The other GPU tests call on torch's current stream, or make a side stream the current one first: a library that ignored its stream
argument, or a wrapper that zero-filled its outputs on another stream than the one it launches on, passes them all.  Here the side
stream is never the current one, and a bounded delay (tests/stream_cases.py) stands where an unordered read, fill or launch would
win the race.  What comes out is compared with the CPU statements byte for byte, canaries and guard bytes included.

Scenario B against the wrappers as they were before psxavenc_amd/_lib.new_tensor (their torch.zeros on the current stream): see
NOTEBOOK.md, "Stream contract".

Every test is one GPU step under a time limit of its own: a watchdog ends the process if a step hangs, so nothing more is started
on the device after it."""
import faulthandler

import numpy as np
import pytest

import stream_cases as SC

pytestmark = pytest.mark.gpu

STEP_SECONDS = 120
# the calls documented to wait for their stream: the only ones scenario A does not hold to "returned before its input was there"
MAY_BLOCK = ["decode_chains_device", "decode_chains_chunked", "adpcm_sse", "disc_read without a reader"]


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


@pytest.fixture(scope="module", autouse=True)
def calibrated():
    """cycles per millisecond of the delay, once per module, on an idle device"""
    return SC.cycles_per_ms()


def test_the_calls_that_may_block_are_exactly_the_documented_ones():
    names = sorted({n.split(" pitch ")[0] for n in SC.SYNCHRONISING})
    assert names == sorted(MAY_BLOCK)
    for make in SC.SYNCHRONISING.values():
        assert make().synchronises
    for make in list(SC.ASYNCHRONOUS.values()) + list(SC.ENCODER_SIDE.values()):
        assert not make().synchronises
    assert len(SC.ASYNCHRONOUS) == 10 and len(SC.ENCODER_SIDE) == 4


def test_the_delay_is_a_bounded_wait(calibrated):
    import torch
    assert 1e4 < calibrated < 1e7, calibrated                  # a device clock between 10 MHz and 10 GHz
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    SC.sleep_on_current_stream(SC.MIN_DELAY_MS)
    t1.record()
    torch.cuda.synchronize()
    assert 0.5 * SC.MIN_DELAY_MS < t0.elapsed_time(t1) < 4 * SC.MIN_DELAY_MS
    assert SC.delay_ms(0.1) == SC.MIN_DELAY_MS and SC.delay_ms(7.0) == 70.0 and SC.delay_ms(1e6) == SC.MAX_DELAY_MS


# ---- A. a late producer on a side stream that is not the current one: the C contract
@pytest.mark.parametrize("name", list(SC.ASYNCHRONOUS))
def test_late_producer_on_a_side_stream(name):
    SC.late_producer(SC.ASYNCHRONOUS[name]())


@pytest.mark.parametrize("name", list(SC.SYNCHRONISING))
def test_late_producer_on_a_side_stream_calls_that_synchronise(name):
    SC.late_producer(SC.SYNCHRONISING[name]())


# ---- B. a busy current stream, the wrapper allocates: the Python layer
@pytest.mark.parametrize("name", list(SC.ASYNCHRONOUS) + list(SC.ENCODER_SIDE))
def test_busy_current_stream_and_outputs_the_wrapper_allocates(name):
    SC.busy_current_stream((SC.ASYNCHRONOUS.get(name) or SC.ENCODER_SIDE[name])())


# ---- C. one handle, its workspace grows between two calls nothing synchronises
@pytest.mark.parametrize("name", list(SC.GROWING))
def test_workspace_grows_between_unsynchronised_calls(name):
    SC.growing_workspace(SC.GROWING[name](1), SC.GROWING[name](4))


def test_resampler_pieces_carry_the_history_between_unsynchronised_calls():
    """3 000 and 12 000 frames of one signal through one fresh handle, on a side stream behind a delay: the second call reads the
    history the first one's kernel leaves, and the staging of the first is outgrown"""
    import torch
    pieces = [3000, 12000]
    x = SC.resample_signal(sum(pieces), 95)
    want = SC.resample_statement(x)
    d = [torch.from_numpy(np.ascontiguousarray(p)).to(SC.DEV) for p in (x[:pieces[0]], x[pieces[0]:])]
    r = SC.new_resampler()
    try:
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            SC.sleep_on_current_stream(SC.MIN_DELAY_MS)
        first = r.convert_device(d[0], flush=False, stream=side)
        second = r.convert_device(d[1], flush=True, stream=side)
        side.synchronize()
        torch.cuda.synchronize()
        got = np.concatenate([first.cpu().numpy(), second.cpu().numpy()])
        assert first.shape[0] > 0 and got.shape == want.shape
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, ("frames differ from the statement", bad[:8].tolist(), "the seam is at", first.shape[0])
    finally:
        torch.cuda.synchronize()
        r.close()


# ---- D. two handles on two side streams at once: the per-device tables they share
@pytest.mark.parametrize("name", list(SC.SHARED_TABLES))
def test_two_handles_on_two_side_streams(name):
    SC.two_handles(SC.SHARED_TABLES[name]())
