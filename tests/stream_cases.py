"""The cases and the scenarios of tests/test_gpu_stream_contract.py: every device entry point held to the stream it is given.

A case names one entry point at the smallest shape at which its path still runs: the host inputs (a real one, and a decoy of the
same shape whose answer differs in every compared output), how to call the wrapper on a given stream, and the answer of the CPU
statement the suite already has for it -- never another run of the library.  The scenarios put a delay (torch.cuda._sleep, a bounded
wait) where an unordered read, fill or launch would show:

  A  the input arrives late on a side stream that is NOT torch's current stream; the call must not read early and must not block
  B  torch's current stream is busy, the call goes to a side stream and the wrapper allocates the outputs
  C  one handle, a small call and a four times larger one behind a delay, nothing synchronised in between (the workspace grows)
  D  two handles on two side streams at once, each behind its own delay, each with its own input

Test infrastructure only; the streams it muxes on the device are inputs, what they are compared with is a statement's.
"""
import functools
import time

import numpy as np

CANARY = 0xA5              # every byte of a buffer the test hands in, and of the GUARD bytes before and behind it
GUARD = 256
DEV = "cuda:0"
MIN_DELAY_MS, MAX_DELAY_MS = 30.0, 500.0


class Case:
    """name; real / decoy: dict name -> numpy array, the device inputs; outputs: dict name -> (shape, numpy dtype) of what the caller
    may hand in; required: the names of those the wrapper cannot allocate itself; handle(): a new handle (None: the entry point has
    none); call(h, d_in, d_out, stream) -> dict name -> tensor of every compared output (d_out: the tensors handed in, by name);
    expect(host, fill) -> dict name -> numpy array, the statement's answer where the outputs handed in held `fill` in every byte
    (0: the wrapper's own zeroed outputs); rewind(h): what puts a handle with a history back to its start (device idle);
    synchronises: the call is documented to wait for its stream"""

    def __init__(self, name, real, decoy, outputs, call, expect, handle=None, required=(), rewind=None, synchronises=False):
        self.name, self.real, self.decoy, self.outputs, self.call, self._expect = name, real, decoy, outputs, call, expect
        self.handle = handle or (lambda: None)
        self.required, self.rewind, self.synchronises = tuple(required), rewind or (lambda h: None), synchronises
        self._answers = {}

    def expect(self, which, fill):
        """the statement's answer for 'real' or 'decoy', computed once and left unchanged"""
        key = (which, fill)
        if key not in self._answers:
            ans = self._expect(getattr(self, which), fill)
            for v in ans.values():
                v.setflags(write=False)
            self._answers[key] = ans
        return self._answers[key]

    def check_decoy(self):
        assert {k: (v.shape, v.dtype) for k, v in self.real.items()} == {k: (v.shape, v.dtype) for k, v in self.decoy.items()}, self.name
        real, decoy = self.expect("real", CANARY), self.expect("decoy", CANARY)
        assert real.keys() == decoy.keys()
        for k in real:
            assert real[k].shape == decoy[k].shape and not np.array_equal(real[k], decoy[k]), \
                "%s: the decoy's %s equals the real one's: a call that read the decoy would pass" % (self.name, k)


def canvas(shape, dtype, fill):
    """an array of `shape` whose every byte is `fill`"""
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, fill, np.uint8).view(dtype).reshape(shape)


def close(h):
    if h is not None and hasattr(h, "close"):
        h.close()


# ---------------------------------------------------------------------------------------------------------------- the delay
_cal = {}


def cycles_per_ms():
    """torch.cuda._sleep counts device clock cycles: calibrated once, with events, on an idle device"""
    import torch
    if "cycles" not in _cal:
        torch.cuda.synchronize()
        torch.cuda._sleep(1000000)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        probe = 20000000
        t0.record()
        torch.cuda._sleep(probe)
        t1.record()
        torch.cuda.synchronize()
        _cal["cycles"] = probe / t0.elapsed_time(t1)
        print("stream contract: torch.cuda._sleep runs %.0f cycles per millisecond" % _cal["cycles"])
    return _cal["cycles"]


def delay_ms(call_ms):
    return min(MAX_DELAY_MS, max(MIN_DELAY_MS, 10.0 * call_ms))


def sleep_on_current_stream(ms):
    import torch
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(ms * cycles_per_ms()))
    else:                                                # a chain of elementwise passes over one large tensor
        x = _cal.setdefault("ballast", torch.zeros(1 << 26, device=DEV))
        for _ in range(int(ms * 4)):
            x.add_(1.0)


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _pinned(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()


def _device_inputs(host):
    import torch
    return {k: torch.empty(v.shape, dtype=torch.from_numpy(v[:0].copy()).dtype, device=DEV) for k, v in host.items()}


def _guarded(case, names):
    """per name: (flat uint8 buffer, the view of the output between GUARD bytes); every byte CANARY"""
    import torch
    bufs, views = {}, {}
    for k in names:
        shape, dtype = case.outputs[k]
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        buf = torch.full((2 * GUARD + nbytes,), CANARY, dtype=torch.uint8, device=DEV)
        bufs[k] = buf
        views[k] = buf[GUARD:GUARD + nbytes].view(torch.from_numpy(np.zeros(0, dtype)).dtype).view(shape)
    return bufs, views


def _same(case, got, want, what):
    assert got.keys() == want.keys(), (case.name, what, sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (case.name, what, k, g.shape, g.dtype, w.shape, w.dtype)
        if not np.array_equal(g, w):
            bad = np.nonzero(g.reshape(-1) != w.reshape(-1))[0]
            raise AssertionError("%s, %s: %s differs from the statement in %d of %d elements, the first at %d: %s, statement %s%s" % (
                case.name, what, k, bad.size, g.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]],
                " -- every element is zero: the output was wiped" if not g.any() else ""))


def _guards_kept(case, bufs, what):
    for k, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:GUARD] == CANARY).all() and (h[-GUARD:] == CANARY).all(), "%s, %s: guard bytes round %s changed" % (case.name, what, k)


def _warm(case, h, d_in, d_out, stream=None):
    """two calls of the measured shape on an idle device, the second timed from the host (launch and run): milliseconds"""
    import torch
    case.rewind(h)
    case.call(h, d_in, d_out, stream)
    torch.cuda.synchronize()
    case.rewind(h)
    t = time.perf_counter()
    case.call(h, d_in, d_out, stream)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) * 1000.0
    case.rewind(h)
    return ms


# ---------------------------------------------------------------------------------------------------------------- scenario A
def late_producer(case):
    import torch
    case.check_decoy()
    h = case.handle()
    try:
        d_in = _device_inputs(case.real)
        real, decoy = {k: _pinned(v) for k, v in case.real.items()}, {k: _pinned(v) for k, v in case.decoy.items()}
        bufs, d_out = _guarded(case, case.outputs)
        for k, t in d_in.items():
            t.copy_(decoy[k])
        torch.cuda.synchronize()
        ms = delay_ms(_warm(case, h, d_in, d_out))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):                    # the producer: nothing of it is ordered against torch's current stream
            for k, t in d_in.items():
                t.copy_(decoy[k], non_blocking=True)
            for b in bufs.values():
                b.fill_(CANARY)
            sleep_on_current_stream(ms)
            for k, t in d_in.items():
                t.copy_(real[k], non_blocking=True)
        assert torch.cuda.current_stream() != side
        got = case.call(h, d_in, d_out, side)
        returned_early = not side.query()
        with torch.cuda.stream(side):
            clones = {k: v.clone() for k, v in got.items()}
        side.synchronize()
        print("%s: delay %.0f ms, the call returned with its input still to come: %s" % (case.name, ms, returned_early))
        if not case.synchronises:
            assert returned_early, "%s: the call returned only after its stream had run dry: it waited, or the delay (%.0f ms) was too short" % (case.name, ms)
        want = case.expect("real", CANARY)
        _same(case, clones, want, "late producer, cloned on the stream")
        torch.cuda.synchronize()
        _same(case, got, want, "late producer")
        _guards_kept(case, bufs, "late producer")
    finally:
        torch.cuda.synchronize()
        close(h)


# ---------------------------------------------------------------------------------------------------------------- scenario B
def busy_current_stream(case):
    import torch
    h = case.handle()
    try:
        d_in = _device_inputs(case.real)
        for k, t in d_in.items():
            t.copy_(_pinned(case.real[k]))
        bufs, d_out = _guarded(case, case.required)
        for b in bufs.values():
            b.zero_()                                    # what the wrapper cannot allocate is handed in zeroed: one answer for all
        torch.cuda.synchronize()
        # (warmed up on a side stream of its own: a split launch of the MDEC encoder -- at most 12 frames -- orders itself behind
        #  whatever the stream of the device's previous split launch holds when the call is made, psxhip_api.cpp's SplitGate; after a
        #  warm-up on the current stream that would be the delay below, and the side stream would rightly wait for it)
        ms = delay_ms(_warm(case, h, d_in, d_out, torch.cuda.Stream()))
        for b in bufs.values():
            b.zero_()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        sleep_on_current_stream(ms)
        got = case.call(h, d_in, d_out, side)
        side.synchronize()
        still_busy = not torch.cuda.current_stream().query()
        torch.cuda.synchronize()
        print("%s: delay %.0f ms on the current stream, still busy when the side stream was done: %s" % (case.name, ms, still_busy))
        assert still_busy, "%s: the current stream was idle when the side stream finished: the delay (%.0f ms) was too short, nothing shown" % (case.name, ms)
        _same(case, got, case.expect("real", 0), "busy current stream")
    finally:
        torch.cuda.synchronize()
        close(h)


# ---------------------------------------------------------------------------------------------------------------- scenario C
def growing_workspace(small, large):
    """small then large on one fresh handle, on a side stream behind a delay, no host synchronisation in between"""
    import torch
    h = small.handle()
    try:
        loaded = []
        for case in (small, large):
            d_in = _device_inputs(case.real)
            for k, t in d_in.items():
                t.copy_(_pinned(case.real[k]))
            bufs, d_out = _guarded(case, case.required)
            for b in bufs.values():
                b.zero_()
            loaded.append((d_in, d_out))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            sleep_on_current_stream(MIN_DELAY_MS)
        got = [case.call(h, d_in, d_out, side) for case, (d_in, d_out) in zip((small, large), loaded)]
        side.synchronize()
        torch.cuda.synchronize()
        _same(small, got[0], small.expect("real", 0), "small call before the workspace grew")
        _same(large, got[1], large.expect("real", 0), "large call after the workspace grew")
    finally:
        torch.cuda.synchronize()
        close(h)


# ---------------------------------------------------------------------------------------------------------------- scenario D
def two_handles(case):
    import torch
    case.check_decoy()
    handles = [case.handle(), case.handle()]
    try:
        loaded = []
        for host in (case.real, case.decoy):
            d_in = _device_inputs(host)
            for k, t in d_in.items():
                t.copy_(_pinned(host[k]))
            bufs, d_out = _guarded(case, case.required)
            for b in bufs.values():
                b.zero_()
            loaded.append((d_in, d_out))
        torch.cuda.synchronize()
        sides = [torch.cuda.Stream(), torch.cuda.Stream()]
        for side, ms in zip(sides, (MIN_DELAY_MS, 1.5 * MIN_DELAY_MS)):
            with torch.cuda.stream(side):
                sleep_on_current_stream(ms)
        got = [case.call(h, d_in, d_out, side) for h, (d_in, d_out), side in zip(handles, loaded, sides)]
        for side in sides:
            side.synchronize()
        torch.cuda.synchronize()
        _same(case, got[0], case.expect("real", 0), "two handles, the first stream")
        _same(case, got[1], case.expect("decoy", 0), "two handles, the second stream")
    finally:
        torch.cuda.synchronize()
        for h in handles:
            close(h)


# ================================================================================================================ the cases
W, H = 48, 32                    # pictures of the BS decoder's cases
BUDGET = 4096


@functools.lru_cache(maxsize=None)
def mdec_decode(scale=1):
    """MdecDecoder.decode_frames_device: 48x32, 4 frames, a per-frame sizes tensor; levels, frames and records"""
    import mdec_decode_corpus as DC
    import mdec_recon_ref as R
    import oracle_lib as O
    n, fb, blocks = 4 * scale, W * H * 3 // 2, (W // 16) * (H // 16) * 6

    def host(seed, amp):
        out, res, rc = O.mdec_encode(0, W, H, O.synth_frames(W, H, n, seed=seed, amp=amp), BUDGET)
        assert rc == 0 and ((res[:, 0] >= 1) & (res[:, 0] <= 63)).all()
        return dict(bs=out, sizes=np.minimum(res[:, 1], BUDGET).astype(np.int32))

    def call(h, d, out, stream):
        lv, fr, dec = h.decode_frames_device(d["bs"], d["sizes"], d_levels=out.get("levels"), d_frames=out.get("frames"),
                                             d_decoded=out.get("decoded"), stream=stream)
        return dict(levels=lv, frames=fr, decoded=dec)

    def expect(x, fill):
        lv, fr, dec = np.zeros((n, blocks, 64), np.int16), np.zeros((n, fb), np.uint8), np.zeros((n, 4), np.int32)
        for i in range(n):
            rc, lv[i], q, v, nbits = DC.oracle_decode(DC.Case("", W, H, False, x["bs"][i], int(x["sizes"][i])))
            assert rc == 0
            fr[i], dec[i] = R.reconstruct(W, H, lv[i], q), (0, q, v, nbits)
        return dict(levels=lv, frames=fr, decoded=dec)

    def handle():
        from psxavenc_amd import MdecDecoder
        return MdecDecoder(W, H)

    return Case("MdecDecoder.decode_frames_device x%d" % scale, host(21, 6), host(22, 30),
                dict(levels=((n, blocks, 64), np.int16), frames=((n, fb), np.uint8), decoded=((n, 4), np.int32)), call, expect, handle)


@functools.lru_cache(maxsize=None)
def sse():
    import mdec_recon_ref as R
    import oracle_lib as O
    n = 4

    def host(seed):
        a = O.synth_frames(W, H, n, seed=seed, amp=20)
        b = a ^ np.random.default_rng(seed).integers(0, 8, a.shape).astype(np.uint8)
        return dict(a=a, b=b)

    def call(h, d, out, stream):
        from psxavenc_amd.decode import sse_device
        return dict(sse=sse_device(d["a"], d["b"], W, H, d_sse=out.get("sse"), stream=stream))

    return Case("sse_device", host(31), host(32), dict(sse=((n, 3), np.int64)), call,
                lambda x, fill: dict(sse=R.sse(W, H, x["a"], x["b"]).view(np.int64)))


def _xa_settings():
    from psxavenc_amd.adpcm import XaSettings
    return XaSettings(1, True, 37800, 4, 1, 2)


@functools.lru_cache(maxsize=None)
def xa_disassemble():
    """two stereo 4-bit XACD sectors, one with a wrong EDC byte (status bit 8: tests/test_gpu_adpcm_decode.py, sector status bits)"""
    import adpcm_decode_ref as R
    import adpcm_encode_corpus as EC
    sectors, _ = EC.xa_sectors(1, 1, 4, False, lba=40)
    real, decoy = sectors[0:2].copy(), sectors[2:4].copy()
    real[1, 2352 - 4 + 2] ^= 0x01
    decoy[0, 2352 - 4 + 1] ^= 0x40
    status = {real.tobytes(): [0, 8], decoy.tobytes(): [8, 0]}

    def call(h, d, out, stream):
        from psxavenc_amd import xa_disassemble
        units, st = xa_disassemble(d["sectors"], _xa_settings(), d_units=out.get("units"), stream=stream)
        return dict(units=units, status=st)

    def expect(x, fill):
        return dict(units=np.concatenate([R.xa_sector_records(s, 4) for s in x["sectors"]]).reshape(2 * 144, 16),
                    status=np.array(status[x["sectors"].tobytes()], np.int32))

    return Case("xa_disassemble", dict(sectors=real), dict(sectors=decoy), dict(units=((2 * 144, 16), np.uint8)), call, expect)


@functools.lru_cache(maxsize=None)
def spu_deinterleave():
    """five chunks out of six rows through a device-side row table, one chunk skipped: its records keep what the buffer held"""
    import strspu_demux_ref as R
    rows, n_chunks, lane, ch = 6, 5, 16 * 63, 2
    records = n_chunks * ch * (lane // 16)

    def host(seed, table):
        return dict(chunks=np.random.default_rng(seed).integers(0, 256, (rows, 2048)).astype(np.uint8), src_chunk=np.array(table, np.int32))

    def call(h, d, out, stream):
        from psxavenc_amd import spu_deinterleave_device
        return dict(units=spu_deinterleave_device(d["chunks"], lane, ch, lane_offset=0x20, d_src_chunk=d["src_chunk"], d_units=out.get("units"),
                                                  stream=stream))

    def expect(x, fill):
        units = canvas((records, 16), np.uint8, fill)
        R.deinterleave(x["chunks"], 0x20, lane, ch, units, x["src_chunk"])
        return dict(units=units.reshape(1, records, 16))

    return Case("spu_deinterleave_device", host(41, [3, -1, 0, 5, 2]), host(42, [1, 4, 2, -1, 0]), dict(units=((1, records, 16), np.uint8)),
                call, expect)


SW, SH = 64, 48                  # pictures of the STR readers' streams
BS_STRIDE = 10 * 2016


def _mux_on_device(s, frames, pcm):
    """one stream from the library's muxer: an input of the reader's cases (what the reader makes of it is the statement's to say)"""
    import torch
    from psxavenc_amd import strmux
    mux = strmux.StrMuxer((0,))
    d_out, p = mux.encode_device(s, torch.from_numpy(frames).to(DEV), torch.from_numpy(pcm).to(DEV) if pcm is not None else None)
    torch.cuda.synchronize()
    out = d_out[0].cpu().numpy()
    mux.close()
    return out, p


@functools.lru_cache(maxsize=None)
def str_demux(scale=1):
    """StrReader.demux_device: a 64x48 STRCD stream of 5 frames with stereo XA; the decoy has lost a video and an audio sector"""
    import oracle_lib as O
    import str_demux_corpus as K
    import str_demux_ref as D
    from psxavenc_amd import strmux
    n_frames = 5 * scale
    s = strmux.settings(fmt=7, codec=0, width=SW, height=SH, fps_num=15, channels=2, tail=strmux.TAIL_COMPLETE)
    pl = strmux.plan(s, n_frames)
    n_pcm = pl.audio_samples_per_sector * (pl.n_audio_sectors + 2) + 100

    def host(seed, lose):
        sectors, p = _mux_on_device(s, O.synth_frames(SW, SH, n_frames, seed=seed, amp=6), K.pcm_for(2, n_pcm, seed + 1))
        assert p.n_frames_encoded == n_frames and p.n_audio_sectors >= 2
        if lose:
            table = strmux.plan_sectors(s, n_frames, n_pcm)
            sectors[np.nonzero(table[:, 0] == strmux.SECTOR_VIDEO)[0][1]] = 0
            sectors[np.nonzero(table[:, 0] == strmux.SECTOR_AUDIO)[0][0]] = 0
        return dict(sectors=sectors)

    real, decoy = host(51, False), host(53, True)
    n = real["sectors"].shape[0]
    shapes = dict(bs=((1, n_frames, BS_STRIDE), np.uint8), sizes=((1, n_frames), np.int32), info=((1, n_frames, 8), np.int32),
                  xa=((1, n, 2352), np.uint8), table=((1, n, 4), np.int32), summary=((1, 8), np.int32))

    def call(h, d, out, stream):
        return h.demux_device(s, d["sectors"], n_frames, BS_STRIDE, d_bs=out.get("bs"), d_sizes=out.get("sizes"), d_info=out.get("info"),
                              d_xa=out.get("xa"), d_table=out.get("table"), d_summary=out.get("summary"), stream=stream)

    def expect(x, fill):
        bs, xa = canvas((n_frames, BS_STRIDE), np.uint8, fill), canvas((n, 2352), np.uint8, fill)
        out = D.demux(s, x["sectors"], -1, n_frames, bs, xa)
        out.update(bs=bs, xa=xa)
        return {k: np.ascontiguousarray(v).reshape(shapes[k][0]) for k, v in out.items()}

    def handle():
        from psxavenc_amd import StrReader
        return StrReader(0)

    return Case("StrReader.demux_device x%d" % scale, real, decoy, shapes, call, expect, handle)


@functools.lru_cache(maxsize=None)
def strspu_demux(scale=1):
    """StrReader.demux_strspu_device: the STRSPU equivalent, muxed by the muxer's statement (tests/strspu_ref.py)"""
    import oracle_lib as O
    import strspu_demux_cases as X
    import strspu_demux_ref as R
    import strspu_ref as M
    from psxavenc_amd import strmux
    n_frames, ch, freq, speed = 5 * scale, 2, 44100, 2
    ns = X.settings(ch, freq, speed, width=SW, height=SH)
    s = strmux.settings(fmt=8, codec=0, width=SW, height=SH, fps_num=X.FPS[0], fps_den=X.FPS[1], cd_speed=speed, video_id=ns.str_video_id,
                        channels=ch, frequency=freq, tail=strmux.TAIL_COMPLETE, audio_id=ns.strspu_options & 0xFFFF)
    rows, _, K = M.schedule(ch, freq, speed, X.FPS[0], X.FPS[1], False, n_frames)

    def host(seed, lose):
        pcm = X.pcm_for(ch, (K + 1) * 28 * (126 // ch) + 100, seed + 1)
        sectors, _, _, _ = M.encode_stream(0, SW, SH, X.FPS[0], X.FPS[1], speed, O.synth_frames(SW, SH, n_frames, seed=seed, amp=6), pcm, channels=ch,
                                           frequency=freq, trailing_audio=False, video_id=ns.str_video_id, options=ns.strspu_options)
        sectors = np.array(sectors)
        if lose:
            audio = [i for i in range(len(sectors)) if R.is_audio(sectors[i], ch, ns.strspu_options & 0xFFFF)]
            video = [i for i in range(len(sectors)) if i not in audio]
            sectors[audio[1]] = 0
            sectors[video[2]] = 0
        return dict(sectors=sectors)

    real, decoy = host(61, False), host(63, True)
    n = real["sectors"].shape[0]
    assert K >= 2
    shapes = dict(bs=((1, n_frames, BS_STRIDE), np.uint8), sizes=((1, n_frames), np.int32), info=((1, n_frames, 8), np.int32),
                  units=((1, n * 126, 16), np.uint8), chunk_info=((1, n, 8), np.int32), table=((1, n, 4), np.int32), summary=((1, 8), np.int32),
                  audio_summary=((1, 4), np.int32))

    def call(h, d, out, stream):
        return h.demux_strspu_device(s, d["sectors"], n_frames, BS_STRIDE, d_bs=out.get("bs"), d_sizes=out.get("sizes"), d_info=out.get("info"),
                                     d_units=out.get("units"), d_chunk_info=out.get("chunk_info"), d_table=out.get("table"),
                                     d_summary=out.get("summary"), d_audio_summary=out.get("audio_summary"), stream=stream)

    def expect(x, fill):
        out = X.run_statement(ns, x["sectors"], -1, n_frames, BS_STRIDE, n, fill)
        return {k: np.ascontiguousarray(v).reshape(shapes[k][0]) for k, v in out.items()}

    def handle():
        from psxavenc_amd import StrReader
        return StrReader(0)

    return Case("StrReader.demux_strspu_device x%d" % scale, real, decoy, shapes, call, expect, handle)


SLOTS, START_LBA = [0, 1], 100


def _two_sources(seed, counts=(6, 6)):
    """2 sources x 6 sectors for the finisher: a 2336-byte one of mixed forms and a 2048-byte one"""
    import disc_read_corpus as K
    import disc_ref as R
    rng = np.random.default_rng(seed)
    return [R.Source(K.sectors(rng, counts[0], 2336, forms=rng.integers(1, 3, counts[0]).tolist()), 2336, file=1, channel=0),
            R.Source(K.sectors(rng, counts[1], 2048), 2048, file=2, channel=0)]


@functools.lru_cache(maxsize=None)
def disc_finish():
    import disc_ref as R

    def host(seed):
        a, b = _two_sources(seed)
        return dict(src0=a.data, src1=b.data)

    def sources(x):
        a, b = _two_sources(0)
        return [a._replace(data=x["src0"]), b._replace(data=x["src1"])]

    def call(h, d, out, stream):
        from psxavenc_amd import disc
        keep = [disc.source(d["src0"], 2336, 1, 0), disc.source(d["src1"], 2048, 2, 0)]
        return dict(image=disc.disc_finish(disc.layout(SLOTS, START_LBA), keep, d_out=out.get("image"), stream=stream))

    return Case("disc_finish", host(71), host(72), dict(image=((12, 2352), np.uint8)), call,
                lambda x, fill: dict(image=R.finish(SLOTS, START_LBA, sources(x))))


@functools.lru_cache(maxsize=None)
def disc_check():
    import disc_ref as R

    def host(seed, damage):
        image = R.finish(SLOTS, START_LBA, _two_sources(seed))
        for k, at in damage:
            image[k, at] ^= 0x10
        return dict(image=image)

    def call(h, d, out, stream):
        from psxavenc_amd import disc
        st, summary = disc.disc_check(d["image"], stream=stream)
        return dict(status=st, summary=summary)

    def expect(x, fill):
        st, summary = R.check(x["image"])
        return dict(status=st, summary=np.array([summary[f] for f in R.SUMMARY_FIELDS], np.int32))

    return Case("disc_check", host(73, [(3, 0x400), (7, 5)]), host(74, [(1, 0x300), (5, 0x11), (9, 0x500)]), {}, call, expect)


@functools.lru_cache(maxsize=None)
def disc_read(scale=1, through_function=False):
    """DiscReader.read_device: 40 sectors, 2 tracks, 3 damaged sectors (the decoy: other counts per track, 5 damaged)"""
    import disc_read_corpus as K
    import disc_read_ref as D
    import disc_ref as R
    n, cap = 40 * scale, 24 * scale
    tracks = [D.Track(2336, cap, 1, 0), D.Track(2048, cap, 2, 0)]

    def host(seed, counts, n_damaged):
        rng = np.random.default_rng(seed)
        image = R.finish(SLOTS, 20000, _two_sources(seed, counts))
        assert image.shape[0] == n
        form1 = [k for k in range(n) if not image[k, 0x12] & 0x20 and image[k, 0x12] & 0x0E]
        for k in form1[1:1 + 4 * n_damaged:4]:
            image[k] = K.scattered(image[k], 2, rng)
        return dict(image=image)

    def call(h, d, out, stream):
        from psxavenc_amd import discread
        keep = [discread.track(out["track%d" % t], T.size, T.file, T.channel, T.mask, T.value) for t, T in enumerate(tracks)]
        got = discread.disc_read(d["image"], keep, stream=stream) if through_function else h.read_device(d["image"], keep, stream=stream)
        return dict(track0=out["track0"], track1=out["track1"], table=got["table"], counts=got["counts"], summary=got["summary"])

    def expect(x, fill):
        want = D.read(x["image"], tracks, into=[canvas((cap, T.size), np.uint8, fill) for T in tracks])
        summary = np.zeros(16, np.int32)
        summary[:14] = [want.summary[f] for f in D.SUMMARY_FIELDS[:14]]
        summary[14:].view(np.int64)[0] = want.summary["n_corrections"]
        assert want.summary["n_repaired"] >= 3
        return dict(track0=want.tracks[0], track1=want.tracks[1], table=want.table, counts=want.counts, summary=summary)

    def handle():
        from psxavenc_amd import DiscReader
        return None if through_function else DiscReader(0)

    return Case(("disc_read without a reader" if through_function else "DiscReader.read_device") + " x%d" % scale,
                host(81, (20 * scale, 20 * scale), 3), host(82, (20 * scale, 12 * scale), 5),
                dict(track0=((cap, 2336), np.uint8), track1=((cap, 2048), np.uint8)), call, expect, handle, required=("track0", "track1"),
                synchronises=through_function)


RESAMPLE = (0, 2, 48000, 2, 37800)         # S16 interleaved, stereo -> stereo


def resample_statement(x):
    import resample_ref as R
    from psxavenc_amd import resample
    fmt, sch, src, dch, dst = RESAMPLE
    _, _, coef = resample.design(src, dst)
    return R.statement(fmt, [x.reshape(-1)], sch, src, dst, resample.default_matrix(sch, dch), coef, flush=True)


def resample_signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    x = 0.45 * np.sin(2 * np.pi * t * np.array([[0.013, 0.02]])) + 0.25 * rng.standard_normal((n, 2))
    return np.clip(x * 40000, -32768, 32767).astype(np.int16)


def new_resampler():
    from psxavenc_amd import resample
    fmt, sch, src, dch, dst = RESAMPLE
    return resample.Resampler(fmt, sch, src, dch, dst)


@functools.lru_cache(maxsize=None)
def resampler():
    """Resampler.convert_device: 3 000 stereo frames at 48 000 -> 37 800, one flushed call"""
    n = 3000
    real, decoy = dict(pcm=resample_signal(n, 91)), dict(pcm=resample_signal(n, 92))
    want = resample_statement(real["pcm"]).shape

    def call(h, d, out, stream):
        return dict(out=h.convert_device(d["pcm"], d_out=out.get("out"), flush=True, stream=stream))

    return Case("Resampler.convert_device", real, decoy, dict(out=(want, np.int16)), call, lambda x, fill: dict(out=resample_statement(x["pcm"])),
                new_resampler, rewind=lambda h: h.reset())


# ---- ADPCM: 3 chains of 9 units, the second cut mid-unit
N_CHAINS, N_UNITS = 3, 9


def _adpcm_layout(pitch):
    import test_gpu_adpcm_decode as AD
    return AD.layout(N_CHAINS, N_UNITS, pitch)


@functools.lru_cache(maxsize=None)
def decode_chains(pitch, chunked=False):
    import adpcm_decode_ref as R
    import test_gpu_adpcm_decode as AD
    chains, base, total, n_records = _adpcm_layout(pitch)
    assert (chains["sample_limit"] % 28 != 0).sum() == 1

    def host(seed):
        rec = R.random_records(seed, 4, 256)[:N_CHAINS * N_UNITS].reshape(N_CHAINS, N_UNITS, -1)
        states = np.random.default_rng(seed).integers(-32768, 32768, (N_CHAINS, 2)).astype(np.int32)
        return dict(units=AD.scatter_records(rec, chains, base, n_records), states=states)

    def call(h, d, out, stream):
        from psxavenc_amd import decode_chains_chunked, decode_chains_device
        fn = decode_chains_chunked if chunked else decode_chains_device
        fn(d["units"], chains, base, 5, 4, out["samples"], d["states"], out["flags"], out["tail"], stream=stream)
        return dict(samples=out["samples"], states=d["states"], flags=out["flags"], tail=out["tail"])

    def expect(x, fill):
        samples, flags, tail = canvas((total,), np.int16, fill), canvas((n_records,), np.uint8, fill), canvas((N_CHAINS, 28), np.int16, fill)
        states = np.zeros((N_CHAINS, 2), np.int32)
        for c in range(N_CHAINS):
            at = base[c] + int(chains["unit_stride"][c]) * np.arange(N_UNITS)
            pcm, _, flags[at] = R.decode_chain(x["units"][at], 4, 5, x["states"][c])
            lim = int(chains["sample_limit"][c])
            samples[int(chains["sample_offset"][c]) + pitch * np.arange(lim)] = pcm[:lim]
            states[c] = AD.state_after(pcm, x["states"][c], N_UNITS)
            if lim % 28:
                tail[c] = pcm[28 * (lim // 28):28 * (lim // 28) + 28]
        return dict(samples=samples, states=states, flags=flags, tail=tail)

    shapes = dict(samples=((total,), np.int16), flags=((n_records,), np.uint8), tail=((N_CHAINS, 28), np.int16))
    return Case("%s pitch %d" % ("decode_chains_chunked" if chunked else "decode_chains_device", pitch), host(100 + pitch), host(200 + pitch),
                shapes, call, expect, required=tuple(shapes), synchronises=True)


@functools.lru_cache(maxsize=None)
def adpcm_sse(pitch):
    chains, base, total, n_records = _adpcm_layout(pitch)

    def host(seed):
        rng = np.random.default_rng(seed)
        return dict(a=rng.integers(-32768, 32768, total).astype(np.int16), b=rng.integers(-32768, 32768, total).astype(np.int16))

    def call(h, d, out, stream):
        from psxavenc_amd import adpcm_sse as fn
        unit, sums = fn(d["a"], d["b"], chains, base, n_records=n_records, stream=stream)
        return dict(unit=unit, sums=sums)

    def expect(x, fill):
        unit, sums = np.zeros(n_records, np.int64), np.zeros((N_CHAINS, 2), np.int64)
        for c in range(N_CHAINS):
            lim = int(chains["sample_limit"][c])
            idx = int(chains["sample_offset"][c]) + pitch * np.arange(lim)
            aa, bb = np.zeros(28 * N_UNITS, np.int64), np.zeros(28 * N_UNITS, np.int64)
            aa[:lim], bb[:lim] = x["a"][idx], x["b"][idx]
            per_unit = ((aa - bb) ** 2).reshape(-1, 28).sum(axis=1)
            unit[base[c] + int(chains["unit_stride"][c]) * np.arange(N_UNITS)] = per_unit
            sums[c] = (per_unit.sum(), (bb ** 2).sum())
        return dict(unit=unit, sums=sums)

    return Case("adpcm_sse pitch %d" % pitch, host(300 + pitch), host(400 + pitch), {}, call, expect, synchronises=True)


# ---- the encoder side: scenario B only (its own side-stream tests make that stream the current one first)
@functools.lru_cache(maxsize=None)
def mdec_encode():
    import oracle_lib as O
    n = 4
    frames = O.synth_frames(W, H, n, seed=5, amp=4)

    def call(h, d, out, stream):
        rows, res = h.encode_frames_device(d["frames"], BUDGET, stream=stream)
        return dict(rows=rows, results=res)

    def expect(x, fill):
        rows, res, rc = O.mdec_encode(0, W, H, x["frames"], BUDGET)
        assert rc == 0
        return dict(rows=rows, results=res)

    def handle():
        from psxavenc_amd.mdec import MdecEncoder
        return MdecEncoder(0, W, H, max_frame_size=BUDGET, device=0)

    return Case("MdecEncoder.encode_frames_device", dict(frames=frames), dict(frames=frames), {}, call, expect, handle)


SCALE = (0, 200, 148, True, 96, 64)        # tests/test_gpu_scaler_edges.py: STRIDE_GEOMETRIES[0]


@functools.lru_cache(maxsize=None)
def scaler():
    import oracle_lib as O
    fmt, sw, sh, full, dw, dh = SCALE

    def handle():
        from psxavenc_amd.frontend import Scaler
        return Scaler(fmt, sw, sh, dw, dh, src_full_range=full)

    probe = handle()
    pictures = np.random.default_rng(7).integers(0, 256, (3, probe.source_bytes)).astype(np.uint8)
    probe.close()
    return Case("Scaler.convert_device", dict(pictures=pictures), dict(pictures=pictures), {},
                lambda h, d, out, stream: dict(frames=h.convert_device(d["pictures"], stream=stream)),
                lambda x, fill: dict(frames=O.scaler_convert(fmt, sw, sh, full, dw, dh, x["pictures"])), handle)


@functools.lru_cache(maxsize=None)
def xa_assemble():
    import adpcm_encode_corpus as EC
    rec = np.ascontiguousarray(EC.xa_stream(1, 4)[3][:2 * 144])

    def call(h, d, out, stream):
        from psxavenc_amd.adpcm import xa_assemble_device
        return dict(sectors=xa_assemble_device(d["rec"], 2, _xa_settings(), first_lba=40, stream=stream))

    return Case("xa_assemble_device", dict(rec=rec), dict(rec=rec), {}, call,
                lambda x, fill: dict(sectors=np.ascontiguousarray(EC.xa_sectors(1, 1, 4, False, lba=40)[0][:2])))


@functools.lru_cache(maxsize=None)
def str_mux():
    """StrMuxer.encode_device on format 8, whose sectors the muxer's statement gives (tests/strspu_ref.py)"""
    import strspu_demux_cases as X
    from psxavenc_amd import strmux
    ns, frames, pcm, sectors, rows, K, budgets = X.stream(X.CROSSING[6])
    assert ns.audio_channels == 2 and K >= 1
    s = strmux.settings(fmt=8, codec=ns.video_codec, width=ns.video_width, height=ns.video_height, fps_num=ns.str_fps_num, fps_den=ns.str_fps_den,
                        cd_speed=ns.str_cd_speed, video_id=ns.str_video_id, trailing_audio=bool(ns.trailing_audio), channels=ns.audio_channels,
                        frequency=ns.audio_frequency, tail=strmux.TAIL_COMPLETE, audio_id=ns.strspu_options & 0xFFFF,
                        spu_loop=bool(ns.strspu_options & strmux.STRSPU_LOOP), spu_no_leading_dummy=bool(ns.strspu_options & strmux.STRSPU_NO_LEADING_DUMMY))
    host = dict(frames=np.array(frames), pcm=np.array(pcm))

    def call(h, d, out, stream):
        d_out, p = h.encode_device(s, d["frames"], d["pcm"], stream=stream)
        return dict(sectors=d_out)

    return Case("StrMuxer.encode_device", host, host, {}, call, lambda x, fill: dict(sectors=np.array(sectors).reshape((1,) + sectors.shape)),
                lambda: strmux.StrMuxer((0,)))


# what each scenario runs over, by name
ASYNCHRONOUS = dict([("MdecDecoder.decode_frames_device", mdec_decode), ("sse_device", sse), ("xa_disassemble", xa_disassemble),
                     ("spu_deinterleave_device", spu_deinterleave), ("StrReader.demux_device", str_demux),
                     ("StrReader.demux_strspu_device", strspu_demux), ("disc_finish", disc_finish), ("disc_check", disc_check),
                     ("DiscReader.read_device", disc_read), ("Resampler.convert_device", resampler)])
ENCODER_SIDE = dict([("MdecEncoder.encode_frames_device", mdec_encode), ("Scaler.convert_device", scaler), ("xa_assemble_device", xa_assemble),
                     ("StrMuxer.encode_device", str_mux)])
SYNCHRONISING = dict([("decode_chains_device pitch 1", lambda: decode_chains(1)), ("decode_chains_device pitch 2", lambda: decode_chains(2)),
                      ("decode_chains_chunked pitch 1", lambda: decode_chains(1, True)), ("decode_chains_chunked pitch 2", lambda: decode_chains(2, True)),
                      ("adpcm_sse pitch 1", lambda: adpcm_sse(1)), ("adpcm_sse pitch 2", lambda: adpcm_sse(2)),
                      ("disc_read without a reader", lambda: disc_read(1, True))])
GROWING = dict([("MdecDecoder", mdec_decode), ("StrReader.demux_device", str_demux), ("StrReader.demux_strspu_device", strspu_demux),
                ("DiscReader", disc_read)])
SHARED_TABLES = dict([("MdecDecoder", mdec_decode), ("StrReader.demux_device", str_demux), ("StrReader.demux_strspu_device", strspu_demux),
                      ("DiscReader", disc_read)])
