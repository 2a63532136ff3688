"""The reference's own call patterns, driven through the drop-in C functions of libpsxav_hip.so with the
reference's struct layouts (ctypes): encode_file_sbs (filefmt.c:633-662), encode_file_str for config
'strcd v2' (filefmt.c:391-520) and encode_file_spu for config 'spu' (filefmt.c:212-293), each diffed
against the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu


class MdecState(C.Structure):           # mdec_encoder_state_t, include/psxav_mdec.h (psxavenc/mdec.h:32-55)
    _fields_ = [("frame_index", C.c_int), ("frame_data_offset", C.c_int), ("frame_max_size", C.c_int),
                ("frame_block_base_overflow", C.c_int), ("frame_block_overflow_num", C.c_int),
                ("frame_block_overflow_den", C.c_int), ("block_type", C.c_int), ("last_dc_values", C.c_int16 * 3),
                ("bits_value", C.c_uint16), ("bits_left", C.c_int), ("frame_output", C.c_void_p),
                ("bytes_used", C.c_int), ("blocks_used", C.c_int), ("uncomp_hwords_used", C.c_int),
                ("quant_scale", C.c_int), ("quant_scale_sum", C.c_int), ("dct_context", C.c_void_p),
                ("ac_huffman_map", C.c_void_p), ("dc_huffman_map", C.c_void_p), ("coeff_clamp_map", C.c_void_p),
                ("dct_block_lists", C.c_void_p * 6)]


class MdecEncoderT(C.Structure):        # mdec_encoder_t
    _fields_ = [("video_codec", C.c_int), ("video_width", C.c_int), ("video_height", C.c_int), ("state", MdecState)]


class XaSettingsT(C.Structure):         # psx_audio_xa_settings_t
    _fields_ = [("format", C.c_int), ("stereo", C.c_bool), ("frequency", C.c_int), ("bits_per_sample", C.c_int),
                ("file_number", C.c_int), ("channel_number", C.c_int)]


class ChanT(C.Structure):               # psx_audio_encoder_channel_state_t
    _fields_ = [("qerr", C.c_int), ("mse", C.c_uint64), ("prev1", C.c_int), ("prev2", C.c_int)]


class StateT(C.Structure):
    _fields_ = [("left", ChanT), ("right", ChanT)]


@pytest.fixture(scope="module")
def L():
    from psxavenc_amd import _lib
    lib = _lib.lib()
    lib.init_mdec_encoder.argtypes = [C.POINTER(MdecEncoderT), C.c_int, C.c_int, C.c_int]
    lib.init_mdec_encoder.restype = C.c_bool
    lib.destroy_mdec_encoder.argtypes = [C.POINTER(MdecEncoderT)]
    lib.encode_frame_bs.argtypes = [C.POINTER(MdecEncoderT), C.c_void_p]
    lib.encode_frame_bs.restype = None
    lib.encode_sector_str.argtypes = [C.POINTER(MdecEncoderT), C.c_int, C.c_uint16, C.c_void_p, C.c_void_p]
    lib.psx_audio_spu_encode.argtypes = [C.POINTER(ChanT), C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.psx_audio_spu_encode_simple.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.psx_audio_xa_encode.argtypes = [XaSettingsT, C.POINTER(StateT), C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.psx_audio_xa_encode_finalize.argtypes = [XaSettingsT, C.c_void_p, C.c_int]
    lib.psx_audio_xa_get_samples_per_sector.argtypes = [XaSettingsT]
    lib.psx_audio_xa_get_sector_interleave.argtypes = [XaSettingsT]
    lib.psx_cdrom_init_sector.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.psx_cdrom_calculate_checksums.argtypes = [C.c_void_p, C.c_int]
    return lib


def test_encode_file_sbs_loop(L):
    w, h, align, n = 320, 240, 8192, 6
    fr = O.synth_frames(w, h, n, seed=31, amp=8)
    want, want_res, _ = O.mdec_encode(0, w, h, fr, align)
    enc = MdecEncoderT()
    assert L.init_mdec_encoder(C.byref(enc), 0, w, h)
    out = np.zeros(align, np.uint8)
    enc.state.frame_output = out.ctypes.data          # the caller owns frame_output (filefmt.c:637)
    enc.state.frame_data_offset = 0
    enc.state.frame_max_size = align
    enc.state.quant_scale_sum = 0
    for j in range(n):
        L.encode_frame_bs(C.byref(enc), fr[j].ctypes.data)
        assert np.array_equal(out, want[j]), j
        assert [enc.state.quant_scale, enc.state.bytes_used, enc.state.blocks_used, enc.state.uncomp_hwords_used] == want_res[j].tolist()
    assert enc.state.quant_scale_sum == int(want_res[:, 0].sum())
    L.destroy_mdec_encoder(C.byref(enc))
    L.destroy_mdec_encoder(C.byref(enc))                # idempotent (mdec.c:553-578)
    assert not enc.state.dct_context


def test_encode_file_str_strcd_config(L):
    """config 'strcd v2': 320x240 @15 fps, 2x speed, 37800 Hz 4-bit stereo XA: interleave 8 (1 audio : 7 video),
    budgets cycling 16128 / 18144 x3.  Whole sector stream vs the oracle's restatement."""
    w, h, fps_num, fps_den, cd_speed, n_frames = 320, 240, 15, 1, 2, 5
    xs = XaSettingsT(1, True, 37800, 4, 1, 0)
    oxs = O.XaSettings(1, 1, 37800, 4, 1, 0)
    interleave = L.psx_audio_xa_get_sector_interleave(xs) * cd_speed
    assert interleave == 8
    sps = L.psx_audio_xa_get_samples_per_sector(xs)
    vspb = interleave - 1
    fr = O.synth_frames(w, h, n_frames + 1, seed=8, amp=8)
    n_audio = 8
    pcm = np.zeros((n_audio * sps + 4032) * 2, np.int16)
    pcm[0:2 * n_audio * sps:2] = O.synth_pcm(4, 0, 0, n_audio * sps, 0)
    pcm[1:2 * n_audio * sps:2] = O.synth_pcm(4, 1, 0, n_audio * sps, 0)

    enc = MdecEncoderT()
    assert L.init_mdec_encoder(C.byref(enc), 0, w, h)
    base = 75 * cd_speed * vspb * fps_den
    den = interleave * fps_num
    cap = 2016 * -(-base // den)
    fo = np.zeros(cap, np.uint8)
    enc.state.frame_block_base_overflow = base
    enc.state.frame_block_overflow_den = den
    enc.state.frame_output = fo.ctypes.data
    enc.state.frame_index = 0
    enc.state.frame_data_offset = 0
    enc.state.frame_max_size = 0
    enc.state.frame_block_overflow_num = 0
    enc.state.quant_scale_sum = 0
    astate = StateT()

    ofo = np.zeros(cap, np.uint8)
    ost = O.StrState(0, 0, 0, base, 0, den, 0, 0, ofo.ctypes.data)
    oastate = O.State()

    budgets = []
    frame_cursor, audio_cursor = 0, 0
    for sector_count in range(44):
        got = np.zeros(2352, np.uint8)
        want = np.zeros(2352, np.uint8)
        if sector_count % interleave > 0:
            if frame_cursor >= n_frames and enc.state.frame_data_offset >= enc.state.frame_max_size:
                break
            L.psx_cdrom_init_sector(got.ctypes.data, sector_count, 1)          # init_sector_buffer_video, filefmt.c:73-91
            got[16:20] = [1, 0, 0x08 | 0x40, 0]
            got[20:24] = got[16:20]
            used = L.encode_sector_str(C.byref(enc), 7, 0x8001, fr[frame_cursor].ctypes.data, got.ctypes.data)
            L.psx_cdrom_calculate_checksums(got.ctypes.data, 1)
            O.lib().orc_cdrom_init_sector(O.ptr(want, O.u8p), sector_count, 1)
            want[16:20] = [1, 0, 0x08 | 0x40, 0]
            want[20:24] = want[16:20]
            oused = O.lib().orc_mdec_encode_sector_str(C.byref(ost), 0, w, h, O.FMT_STRCD, 0x8001, O.ptr(fr[frame_cursor], O.u8p), O.ptr(want, O.u8p))
            O.lib().orc_cdrom_calculate_checksums(O.ptr(want, O.u8p), 1)
            assert used == oused
            if used:
                budgets.append(enc.state.frame_max_size)
            frame_cursor += used
        else:
            chunk = pcm[2 * audio_cursor:]
            ln = L.psx_audio_xa_encode(xs, C.byref(astate), chunk.ctypes.data, sps, sector_count, got.ctypes.data)
            w_, oastate = O.xa_encode(oxs, chunk, sps, lba=sector_count, state=oastate)
            assert ln == 2352
            want[:] = w_
            audio_cursor += sps
        assert np.array_equal(got, want), sector_count
    assert budgets[:5] == [16128, 18144, 18144, 18144, 16128]
    assert enc.state.quant_scale_sum == ost.quant_scale_sum and enc.state.frame_index == ost.frame_index
    L.destroy_mdec_encoder(C.byref(enc))


def test_encode_file_spu_config(L):
    """config 'spu': mono 22050 Hz 1 s sine -> leading dummy block, 788 blocks by 28-sample calls, trap block,
    padded to 64-byte alignment: 12672 bytes"""
    i = np.arange(22050)
    sine = np.rint(16384 * np.sin(2 * np.pi * 440 * i / 22050)).astype(np.int16)
    st, ost = ChanT(), O.Chan(0, 0)
    blocks, oblocks = [np.zeros(16, np.uint8)], [np.zeros(16, np.uint8)]
    for pos in range(0, sine.size, 28):
        cnt = min(28, sine.size - pos)
        blk = np.zeros(16, np.uint8)
        ln = L.psx_audio_spu_encode(C.byref(st), sine[pos:].ctypes.data, cnt, 1, blk.ctypes.data)
        assert ln == 16
        blocks.append(blk)
        oblk, ost = O.spu_encode(sine[pos:pos + cnt], state=ost, n=cnt)
        oblocks.append(oblk)
    trap = np.zeros(16, np.uint8)
    trap[1] = 5
    got = np.concatenate(blocks + [trap])
    want = np.concatenate(oblocks + [trap])
    assert got.size == 12640 and np.array_equal(got, want)
    pad = (-got.size) % 64
    assert got.size + pad == 12672
    assert got[16:20].tobytes() == bytes([0x24, 0x00, 0x70, 0x13])
    # and the one-shot convenience entry point
    buf = np.zeros(13000, np.uint8)
    ln = L.psx_audio_spu_encode_simple(sine.ctypes.data, sine.size, buf.ctypes.data, -1)
    assert ln == 12624 and np.array_equal(buf[:ln - 16], got[16:16 + ln - 16])


def test_c_example_program_builds_runs_and_matches_oracle(tmp_path):
    """examples/sbs_encode.c: a plain-C host program over the drop-in + batched surfaces (gcc only, no HIP headers)"""
    import os
    import subprocess
    root = O.ROOT
    subprocess.run(["make", "-s", "-C", os.path.join(root, "examples")], check=True)
    out = tmp_path / "t.sbs"
    r = subprocess.run([os.path.join(root, "examples", "sbs_encode"), str(out), "5", "320", "240", "8192", "1"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "identical to per-frame path: yes" in r.stdout
    data = np.fromfile(out, dtype=np.uint8).reshape(5, 8192)
    # regenerate the program's frames (integer ramp + LCG) and diff against the oracle
    w, h = 320, 240
    frames = np.zeros((5, w * h * 3 // 2), np.uint8)
    for i in range(5):
        lcg = (12345 + 977 * i) & 0xFFFFFFFF
        yy = np.zeros((h, w), np.int64)
        for y in range(h):
            for x in range(w):
                lcg = (lcg * 1664525 + 1013904223) & 0xFFFFFFFF
                yy[y, x] = ((x + 2 * i) % w) * 255 // w // 2 + y * 255 // h // 2 + ((lcg >> 24) % 9) - 4
        frames[i, :w * h] = np.clip(yy, 0, 255).astype(np.uint8).ravel()
        c = frames[i, w * h:].reshape(h // 2, w)
        xs = np.arange(w // 2)
        ys = np.arange(h // 2)
        c[:, 0::2] = (96 + xs * 64 // (w // 2)).astype(np.uint8)[None, :]
        c[:, 1::2] = (160 - ys * 64 // (h // 2)).astype(np.uint8)[:, None]
    want, _, rc = O.mdec_encode(1, w, h, frames, 8192)
    assert rc == 0 and np.array_equal(data, want)


@pytest.mark.parametrize("fmt,codec,w,h,n_frames,channels", [(7, 0, 320, 240, 160, 2), (6, 1, 160, 112, 40, 1), (9, 2, 96, 64, 30, 0),
                                                            (7, 0, 320, 240, 240, 2)])     # 2400 sectors: the threaded interleave
def test_batched_str_mux_whole_stream_vs_reference_loop(fmt, codec, w, h, n_frames, channels):
    """psxhip_str_encode_host (product code: one batched MDEC call + one XA stream + host interleave), default tail =
    the reference's, against encode_file_str restated call for call over the oracle with its decoder's end-of-input model
    (tests/str_reference_loop.py: filefmt.c:391-520, decoding.c:510-586), whole stream, for config 'strcd v2' (160 frames)
    and the other two STR flavours."""
    import str_reference_loop as R
    from psxavenc_amd import strmux
    s = strmux.settings(fmt=fmt, codec=codec, width=w, height=h, channels=channels, frequency=37800, bits=4)
    frames = O.synth_frames(w, h, n_frames, seed=21, amp=6)
    if channels:
        pl = strmux.plan(s, n_frames)
        n = (pl.n_audio_sectors + 2) * pl.audio_samples_per_sector + 100      # a little more audio than video
        pcm = np.zeros(n * channels, np.int16)
        for c in range(channels):
            pcm[c::channels] = O.synth_pcm(9, c, 0, n, 0)
    else:
        pcm = np.zeros(0, np.int16)
    got, p2 = strmux.encode(s, frames, pcm)
    want, qsum, frames_encoded = R.encode_file_str(fmt, codec, w, h, 15, 1, 2, frames, pcm, channels=channels)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "sectors differ: %s" % bad[:8].tolist()
    assert p2.quant_scale_sum == qsum and p2.n_frames_encoded == frames_encoded == n_frames - 2
    if channels:        # every audio sector after the decoder saw the end carries EOF; more than one does
        sub = 0x12 if fmt == 7 else 0x02
        rows = strmux.plan_sectors(s, n_frames, pcm.size // channels)
        eof = [int(got[k, sub] >> 7) for k in np.nonzero(rows[:, 0] == 1)[0]]
        assert eof == rows[rows[:, 0] == 1, 3].tolist() and eof[0] == 0
        assert sum(eof) >= 1 or channels == 1       # (mono: one sector in 16 is audio, the tail may hold none)


@pytest.mark.parametrize("n_audio_sectors_x10", [0, 5, 30, 87])
def test_batched_str_mux_audio_shorter_than_video(n_audio_sectors_x10):
    """the reference's stream ends with whichever input ends first (decoding.c:540-553): audio of 0 / 0.5 / 3 / 8.7 sectors
    against 24 frames of video -- short last sector completed from the decoder's zero padding, empty audio slots, EOF flags"""
    import str_reference_loop as R
    from psxavenc_amd import strmux
    w, h, n_frames = 160, 112, 24
    s = strmux.settings(fmt=7, codec=0, width=w, height=h)
    frames = O.synth_frames(w, h, n_frames, seed=5, amp=6)
    n = 2016 * n_audio_sectors_x10 // 10
    pcm = np.zeros(2 * n, np.int16)
    for c in range(2):
        pcm[c::2] = O.synth_pcm(11, c, 0, n, 0)
    got, p = strmux.encode(s, frames, pcm)
    want, qsum, frames_encoded = R.encode_file_str(7, 0, w, h, 15, 1, 2, frames, pcm)
    assert got.shape == want.shape and np.array_equal(got, want), (got.shape, want.shape)
    assert (p.quant_scale_sum, p.n_frames_encoded) == (qsum, frames_encoded)
    assert frames_encoded < n_frames - 2            # the audio ended the stream


@pytest.mark.parametrize("fmt,codec,w,h,n_frames,channels", [(7, 0, 320, 240, 160, 2), (6, 1, 160, 112, 40, 1), (9, 2, 96, 64, 30, 0)])
def test_batched_str_mux_complete_tail(fmt, codec, w, h, n_frames, channels):
    """PSXHIP_STR_TAIL_COMPLETE (every frame in the stream, EOF on the last audio sector, silence when the audio runs out):
    the convention of the earlier rounds, reachable by flag only; config 'strcd v2' stays pinned by its SHA-256"""
    import str_reference_loop as R
    from psxavenc_amd import strmux
    s = strmux.settings(fmt=fmt, codec=codec, width=w, height=h, channels=channels, frequency=37800, bits=4, tail=strmux.TAIL_COMPLETE)
    frames = O.synth_frames(w, h, n_frames, seed=21, amp=6)
    p = strmux.plan(s, n_frames)
    if channels:
        n = p.n_audio_sectors * p.audio_samples_per_sector
        pcm = np.zeros((n + 4032) * channels, np.int16)
        for c in range(channels):
            pcm[c:channels * n:channels] = O.synth_pcm(9, c, 0, n, 0)
    else:
        pcm = np.zeros(0, np.int16)
    got, p2 = strmux.encode(s, frames, pcm)
    want, qsum = R.encode_stream_complete(fmt, codec, w, h, 15, 1, 2, frames, pcm, channels=channels)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "sectors differ: %s" % bad[:8].tolist()
    assert p2.quant_scale_sum == qsum and p2.n_frames_encoded == n_frames
    if fmt == 7 and n_frames == 160:
        b = strmux.frame_budgets(s, 0, 5).tolist()
        assert b == [16128, 18144, 18144, 18144, 16128]
        import hashlib
        # pinned: 160 frames of config 'strcd v2' (seed 21, noise +-6) = 1600 sectors
        assert hashlib.sha256(got.tobytes()).hexdigest() == "f2eb7256f1a0e02d681d030651011cfeb9d0ee7cf2c59687a68f579d2b697add"


def test_str_handles_are_independent_and_multi_device_equals_single():
    """no process-global state: two muxer handles with different geometries used alternately and from two threads; a handle
    over the device list {0, 0} (two encoder contexts on one GPU) produces the single-device stream byte for byte"""
    import threading
    from psxavenc_amd import strmux
    a, b, ab = strmux.StrMuxer((0,)), strmux.StrMuxer((0,)), strmux.StrMuxer((0, 0))
    sa = strmux.settings(fmt=7, codec=0, width=320, height=240)
    sb = strmux.settings(fmt=6, codec=1, width=96, height=64, channels=1)
    fa = O.synth_frames(320, 240, 50, seed=2, amp=6)
    fb = O.synth_frames(96, 64, 30, seed=3, amp=6)
    pa = np.zeros(2 * 2016 * 80, np.int16)
    pa[0::2] = O.synth_pcm(1, 0, 0, 2016 * 80, 0)
    pa[1::2] = O.synth_pcm(1, 1, 0, 2016 * 80, 0)
    pb = O.synth_pcm(2, 0, 0, 4032 * 40, 0)
    ra, _ = a.encode(sa, fa, pa)
    rb, _ = b.encode(sb, fb, pb)
    r2, _ = ab.encode(sa, fa, pa)
    assert np.array_equal(r2, ra)
    assert np.array_equal(ab.encode(sb, fb, pb)[0], rb)          # geometry change on one handle
    assert np.array_equal(ab.encode(sa, fa, pa)[0], ra)
    res = {}

    def work(name, m, s, f, p):
        for _ in range(3):
            res[name] = m.encode(s, f, p)[0]

    ths = [threading.Thread(target=work, args=("a", a, sa, fa, pa)), threading.Thread(target=work, args=("b", b, sb, fb, pb))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert np.array_equal(res["a"], ra) and np.array_equal(res["b"], rb)
    for m in (a, b, ab):
        m.close()


def test_strcd_config3_at_1000_frames():
    """BASELINE config 3 at its full size: 1000 frames 320x240 @15 fps + 37800 Hz 4-bit stereo XA, 2x -> STRCD sectors,
    the reference's tail; whole stream against the reference loop over the oracle"""
    import str_reference_loop as R
    from psxavenc_amd import strmux
    w, h, n_frames = 320, 240, 1000
    s = strmux.settings()
    frames = O.synth_frames(w, h, n_frames, seed=1, amp=4)
    n = 2016 * 1260
    pcm = np.zeros(2 * n, np.int16)
    for c in range(2):
        pcm[c::2] = O.synth_pcm(1, c, 0, n, 0)
    got, p = strmux.encode(s, frames, pcm)
    assert p.n_frames_encoded == 998 and p.n_sectors == got.shape[0]
    want, qsum, frames_encoded = R.encode_file_str(7, 0, w, h, 15, 1, 2, frames, pcm)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "sectors differ: %s" % bad[:8].tolist()
    assert (p.quant_scale_sum, frames_encoded) == (qsum, 998)


def test_c_multi_device_program_builds_runs_and_matches(tmp_path):
    """examples/multi_encode.c: a plain-C host program (gcc only) that shards one batch over a device list with one call;
    here over {0, 0, 0} with the host ticket queue -- the program itself compares against the single-device call"""
    import os
    import subprocess
    root = O.ROOT
    subprocess.run(["make", "-s", "-C", os.path.join(root, "examples")], check=True)
    for sched in ("static", "tickets"):
        r = subprocess.run([os.path.join(root, "examples", "multi_encode"), "0,0,0", "1100", "320", "240", "8192", "0", sched],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "identical to the single-device call: yes" in r.stdout
        assert r.stdout.count("worker") == 3


def test_str_mux_randomised_settings_vs_reference_loop():
    """seeded fuzz over what encode_file_str's behaviour depends on: container flavour, codec, frame rate (incl. NTSC's
    30000/1001), CD speed, audio layout (mono / stereo, 4 / 8 bit, 18900 / 37800 Hz), trailing audio, frame count and the amount
    of audio (none, less than the video, more) -- whole stream against the reference's sector loop over the oracle"""
    import str_reference_loop as R
    from psxavenc_amd import strmux
    rng = np.random.default_rng(20260929)
    mux = strmux.StrMuxer((0,))
    done = 0
    for trial in range(40):
        fmt = int(rng.choice([6, 7, 9]))
        codec = int(rng.integers(0, 3))
        w, h = int(rng.choice([48, 64, 96, 160])), int(rng.choice([32, 48, 64, 112]))
        fps = [(15, 1), (10, 1), (25, 1), (30000, 1001), (12, 1), (24000, 1001)][int(rng.integers(0, 6))]
        speed = int(rng.integers(1, 3))
        channels = int(rng.integers(0, 3))
        bits = int(rng.choice([4, 8]))
        freq = int(rng.choice([18900, 37800]))
        trailing = bool(rng.integers(0, 2))
        n_frames = int(rng.integers(1, 40))
        s = strmux.settings(fmt=fmt, codec=codec, width=w, height=h, fps_num=fps[0], fps_den=fps[1], cd_speed=speed, channels=channels,
                            frequency=freq, bits=bits, trailing_audio=trailing)
        try:
            p0 = strmux.plan(s, n_frames)
        except Exception:
            continue                        # frame rate too high for this CD speed: the product refuses, nothing to compare
        if p0.max_frame_size > 60000:
            continue
        sps = p0.audio_samples_per_sector
        n_audio = 0 if not channels else int(rng.choice([0, sps // 3, sps, 3 * sps + 11, (p0.n_audio_sectors + 3) * sps]))
        frames = O.synth_frames(w, h, n_frames, seed=100 + trial, amp=int(rng.integers(2, 10)))
        pcm = np.zeros(n_audio * max(1, channels), np.int16)
        for c in range(channels):
            pcm[c::channels] = O.synth_pcm(trial, c, 0, n_audio, int(rng.integers(0, 3))) if n_audio else 0
        got, p = mux.encode(s, frames, pcm)
        want, qsum, frames_encoded = R.encode_file_str(fmt, codec, w, h, fps[0], fps[1], speed, frames, pcm, channels=channels, freq=freq,
                                                       bits=bits, trailing_audio=trailing)
        ctx = (trial, fmt, codec, w, h, fps, speed, channels, bits, freq, trailing, n_frames, n_audio)
        assert got.shape == want.shape, ctx
        assert np.array_equal(got, want), (ctx, np.nonzero((got != want).any(axis=1))[0][:5].tolist())
        assert (p.quant_scale_sum, p.n_frames_encoded) == (qsum, frames_encoded), ctx
        done += 1
    assert done >= 25
    mux.close()


def test_per_call_harness_builds_and_runs():
    """examples/percall_bench.c: plain C over the three drop-in calls at the reference's own granularity (one launch per call)"""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-s", "-C", os.path.join(root, "examples")], check=True)
    r = subprocess.run([os.path.join(root, "examples", "percall_bench"), "300", "40", "40"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("psx_audio_spu_encode_28_samples", "psx_audio_xa_encode_sector", "encode_frame_bs_320x240_v2"):
        assert d[k]["us_per_call_median"] > 0
    assert d["encode_frame_bs_320x240_v2"]["quant_scale_sum"] > 0
