"""The readers' plan module (psxavenc_amd/csrc/reader_plan.cpp) on the CPU, without HIP and under the host sanitizers, the way
tests/test_str_plan_cpu.py checks the STR muxer's: g++ builds reader_plan.cpp, str_plan.cpp and the driver
(tests/cpu/reader_plan_check.cpp, which brings the error sink) and nothing else.  The driver is handed this file's table of calls and
prints what the plans derive; the expectations are restatements in Python over the constants the driver prints.  Every case is
arithmetic only: counts may be huge and addresses are made up.

tests/golden/reader_plan_parent.json holds what the library answered before the plan module existed: (rc, psxhip_last_error()) for
REFUSALS, a table of calls of the seven entry points the module plans.  It was recorded on a machine without a device, where every
refusal that precedes the device check answers as it does beside a GPU and an accepted call answers "no device", with

    L = bind(ctypes.CDLL(path_of_that_libpsxav_hip_so))
    json.dump([dict(kind=k, settings=s, args=a, rc=rc, error=text) for (k, s, a), (rc, text) in zip(REFUSALS, library_answers(L, REFUSALS))], f)

The plan module and the library as it is built now both have to reproduce the file exactly.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE = -1, -2
P = 0x100000           # the checks look at values only: made-up addresses, never dereferenced
Q = P + (1 << 24)
CHUNK = 2016


def settings(fmt=7, codec=0, width=48, height=32, fps_num=15, fps_den=1, speed=2, video_id=0x8001, trailing=0, ch=2, freq=37800, bits=4,
             xa_file=1, xa_channel=0, tail=0, options=1):
    """the 16 words of psxhip_str_settings_t"""
    return (fmt, codec, width, height, fps_num, fps_den, speed, video_id, trailing, ch, freq, bits, xa_file, xa_channel, tail, options)


def settings8(**kw):
    return settings(**dict(dict(fmt=8, freq=44100, tail=1), **kw))


def pick(defaults, kw):
    assert set(kw) <= set(defaults), kw
    return [dict(defaults, **kw)[name] for name in defaults]


# ------------------------------------------------------------------------------------------------ the calls, arguments in the entry points' order
def demux(s=settings(), **kw):
    return ("demux", s, pick(dict(S=1, d_sectors=P, in_stride=2352 * 4, n=4, first=-1, mf=2, d_bs=P, bs_stride=4032, bs_stream=8064, d_sizes=P, d_info=P,
                                  d_xa=P, cap=4, xa_stream=2352 * 4, d_table=0, d_summary=P), kw))


def strspu(s=settings8(), **kw):
    return ("strspu", s, pick(dict(S=1, d_sectors=P, in_stride=2048 * 4, n=4, first=-1, mf=2, d_bs=P, bs_stride=4032, bs_stream=8064, d_sizes=P, d_info=P,
                                   d_units=P, cap=4, units_stream=4 * 126 * 16, d_chunk=P, d_table=0, d_summary=P, d_asum=P), kw))


def deint(**kw):
    return ("deint", None, pick(dict(d_in=P, n=4, chunk_stride=2048, lane_offset=0x20, lane_bytes=1008, channels=2, src=0, streams=1, in_stride=4 * 2048,
                                     d_units=Q, units_stream=4 * 126 * 16), kw))


def read(s=settings(), **kw):
    return ("read", s, pick(dict(sectors=P, n=4, first=-1, mf=2, frames=0, info=P, decoded=P, pcm=0, pcm_capacity=0, status=0, summary=P), kw))


def readspu(s=settings8(), **kw):
    return ("readspu", s, pick(dict(sectors=P, n=4, first=-1, mf=2, frames=0, info=P, decoded=P, pcm=0, pcm_capacity=0, chunk_info=0, summary=P, asum=0), kw))


def spustreams(**kw):
    return ("spustreams", None, pick(dict(blocks=P, S=2, in_stride=160, n_blocks=10, states=P, samples=P, out_stride=280), kw))


def xastreams(**kw):
    return ("xastreams", None, pick(dict(format=1, stereo=1, frequency=37800, bits=4, sectors=P, S=2, in_stride=2352 * 3, n_sectors=3, states=P, samples=P,
                                         out_stride=4032 * 3, status=0), kw))


UNKNOWN_BIT = settings8(options=1 | 1 << 18)
REFUSALS = [
    # ---- psxhip_str_demux_device: the settings; NULL and counts; alignment; stream strides; what it accepts
    demux(s=None), demux(s=settings(fmt=8)), demux(s=settings(fmt=0)),
    demux(S=0), demux(S=65536), demux(n=-1), demux(mf=-1), demux(cap=-1), demux(first=-2), demux(first=1 << 32), demux(d_summary=0),
    demux(d_sectors=0), demux(d_bs=0), demux(d_sizes=0), demux(d_info=0), demux(d_xa=0),
    demux(d_sectors=P + 2), demux(d_bs=P + 1), demux(d_sizes=P + 2), demux(d_info=P + 2), demux(d_xa=P + 3), demux(d_table=P + 1), demux(d_summary=P + 2),
    demux(in_stride=2352 * 4 + 2), demux(bs_stride=4034), demux(bs_stream=8066), demux(xa_stream=2352 * 4 + 1), demux(bs_stride=2012),
    demux(S=2, in_stride=2352 * 3), demux(S=2, bs_stream=4032), demux(S=2, xa_stream=2352),
    demux(d_summary=0, d_bs=P + 1), demux(s=settings(fmt=8), n=-1), demux(S=2, in_stride=2352 * 3, d_xa=P + 3),          # precedence
    demux(), demux(S=2), demux(n=0, d_sectors=0), demux(mf=0, d_bs=0, d_sizes=0, d_info=0), demux(cap=0, d_xa=0), demux(first=0xFFFFFFFF),
    demux(d_table=P), demux(s=settings(fmt=6), in_stride=2336 * 4, xa_stream=2336 * 4), demux(s=settings(fmt=9)),
    # ---- psxhip_strspu_demux_device: the audio half's refusals, then the video half's
    strspu(s=None), strspu(s=settings(fmt=9)), strspu(s=settings8(ch=3)), strspu(s=settings8(ch=-1)), strspu(s=UNKNOWN_BIT),
    strspu(s=settings8(video_id=-1)), strspu(s=settings8(options=0x8001)),
    strspu(S=0), strspu(S=65536), strspu(cap=-1), strspu(cap=(2 ** 31 - 1) // 126 + 1), strspu(d_asum=0), strspu(d_units=0), strspu(d_chunk=0),
    strspu(d_units=P + 4), strspu(d_units=P + 8), strspu(units_stream=4 * 126 * 16 + 4), strspu(d_chunk=P + 2), strspu(d_asum=P + 1),
    strspu(S=2, units_stream=4 * 126 * 16 - 16),
    strspu(d_sectors=P + 2), strspu(bs_stride=2012), strspu(d_summary=0), strspu(n=-1), strspu(first=-2), strspu(d_table=P + 1),
    strspu(S=2, in_stride=2048 * 3), strspu(S=2, bs_stream=4032),
    strspu(s=UNKNOWN_BIT, cap=-1), strspu(d_asum=0, d_units=P + 4), strspu(d_chunk=P + 2, d_summary=0),                   # precedence
    strspu(), strspu(S=2), strspu(s=settings8(ch=0), cap=0, d_units=0, d_chunk=0), strspu(s=settings8(ch=0, video_id=-1)),
    strspu(cap=(2 ** 31 - 1) // 126, units_stream=0),
    # ---- psxhip_spu_deinterleave_device
    deint(n=-1), deint(streams=0), deint(streams=65536), deint(channels=0), deint(lane_bytes=0), deint(lane_bytes=24), deint(lane_bytes=1000),
    deint(d_in=0), deint(d_units=0),
    deint(d_in=P + 2), deint(src=P + 2), deint(chunk_stride=2050), deint(lane_offset=0x22), deint(in_stride=4 * 2048 + 2), deint(d_units=Q + 4),
    deint(units_stream=4 * 126 * 16 + 8),
    deint(lane_offset=0x1000), deint(lane_offset=0x40), deint(channels=3), deint(chunk_stride=2016), deint(n=(1 << 31) // 126 + 1),
    deint(streams=2, units_stream=4 * 126 * 16 - 16), deint(streams=2, in_stride=3 * 2048),
    deint(d_in=0, d_units=Q + 4), deint(channels=3, d_in=P + 2), deint(streams=2, in_stride=3 * 2048, channels=3),     # precedence
    deint(), deint(streams=2), deint(streams=2, in_stride=0, src=P), deint(n=0, d_in=0, d_units=0),
    deint(lane_offset=0, lane_bytes=16, channels=3, chunk_stride=48, units_stream=4 * 3 * 16), deint(d_in=P + 4),
    # ---- psxhip_str_read_host
    read(s=None), read(s=settings(fmt=5)), read(s=settings(fmt=8)),
    read(n=-1), read(mf=-1), read(pcm_capacity=-1), read(summary=0), read(sectors=0), read(info=0), read(decoded=0),
    read(s=settings(codec=-1)), read(s=settings(codec=3)), read(s=settings(fps_num=0)), read(s=settings(fps_den=0)), read(s=settings(speed=3)),
    read(s=settings(speed=0)), read(s=settings(ch=-1)), read(s=settings(ch=3)), read(s=settings(freq=44100)), read(s=settings(bits=5)),
    read(s=settings(fps_num=1, fps_den=1000)), read(s=settings(fps_num=1, fps_den=300)),
    read(s=settings(fmt=5), n=-1), read(s=settings(fps_num=1, fps_den=1000), mf=-1),                                       # precedence
    read(), read(s=settings(ch=0, bits=5, freq=1)), read(n=0, sectors=0), read(mf=0, info=0, decoded=0), read(pcm=P, pcm_capacity=10 ** 6, status=P),
    # ---- psxhip_strspu_read_host
    readspu(s=None), readspu(s=settings(fmt=7)), readspu(s=settings8(ch=3)), readspu(s=UNKNOWN_BIT), readspu(s=settings8(video_id=-1)),
    readspu(s=settings8(options=0x8001)),
    readspu(n=-1), readspu(mf=-1), readspu(pcm_capacity=-1), readspu(summary=0), readspu(sectors=0), readspu(info=0), readspu(decoded=0),
    readspu(s=settings8(codec=-1)), readspu(s=settings8(codec=3)), readspu(s=settings8(fps_num=0)), readspu(s=settings8(fps_den=0)),
    readspu(s=settings8(speed=3)), readspu(s=settings8(freq=-1)), readspu(s=settings8(fps_num=1, fps_den=1000)),
    readspu(s=UNKNOWN_BIT, n=-1), readspu(s=settings8(fps_num=1, fps_den=1000), summary=0),                               # precedence
    readspu(), readspu(s=settings8(ch=0)), readspu(s=settings8(freq=0)), readspu(pcm=P, pcm_capacity=10 ** 6, chunk_info=P, asum=P),
    # ---- psxhip_spu_decode_streams_host, psxhip_xa_decode_streams_host
    spustreams(S=-1), spustreams(n_blocks=-1), spustreams(blocks=0), spustreams(states=0), spustreams(samples=0),
    spustreams(n_blocks=(2 ** 31 - 1) // 28 + 1, in_stride=1 << 40, out_stride=1 << 40),
    spustreams(in_stride=159), spustreams(out_stride=279), spustreams(in_stride=-160),
    spustreams(S=-1, in_stride=0),                                                                                             # precedence
    spustreams(), spustreams(S=1, in_stride=0, out_stride=0), spustreams(S=0, blocks=0, states=0, samples=0), spustreams(n_blocks=0, blocks=0),
    xastreams(S=-1), xastreams(n_sectors=-1), xastreams(bits=5), xastreams(format=2), xastreams(sectors=0), xastreams(states=0), xastreams(samples=0),
    xastreams(n_sectors=(2 ** 31 - 1) // 4032 + 1, S=1), xastreams(S=4000, n_sectors=4000, in_stride=1 << 40, out_stride=1 << 40),
    xastreams(in_stride=2352 * 3 - 1), xastreams(out_stride=4032 * 3 - 1), xastreams(format=0, in_stride=2336 * 3 - 1),
    xastreams(bits=5, in_stride=0),                                                                                            # precedence
    xastreams(), xastreams(S=1, in_stride=0, out_stride=0), xastreams(S=0), xastreams(n_sectors=0, sectors=0), xastreams(format=0, stereo=0, bits=8),
]


# ------------------------------------------------------------------------------------------------ the library, through ctypes
def bind(L):
    vp, sz, i32, i64 = C.c_void_p, C.c_size_t, C.c_int, C.c_int64
    st = C.c_void_p           # the settings: a pointer to 16 words, or NULL
    L.psxhip_last_error.restype = C.c_char_p
    L.psxhip_str_demux_device.argtypes = [vp, st, i32, vp, sz, i32, i64, i32, vp, sz, sz, vp, vp, vp, i32, sz, vp, vp, vp]
    L.psxhip_strspu_demux_device.argtypes = [vp, st, i32, vp, sz, i32, i64, i32, vp, sz, sz, vp, vp, vp, i32, sz, vp, vp, vp, vp, vp]
    L.psxhip_spu_deinterleave_device.argtypes = [i32, vp, i32, sz, sz, sz, i32, vp, i32, sz, vp, sz, vp]
    L.psxhip_str_read_host.argtypes = [vp, st, vp, i32, i64, i32, vp, vp, vp, vp, i64, vp, vp]
    L.psxhip_strspu_read_host.argtypes = [vp, st, vp, i32, i64, i32, vp, vp, vp, vp, i64, vp, vp, vp]
    L.psxhip_spu_decode_streams_host.argtypes = [i32, vp, i32, i64, i32, vp, vp, i64]
    L.psxhip_xa_decode_streams_host.argtypes = [i32, i32, i32, i32, i32, vp, i32, i64, i32, vp, vp, i64, vp]
    return L


def library_answers(L, calls):
    """(rc, psxhip_last_error()) of every call, with no handle and no stream"""
    out = []
    for kind, s, a in calls:
        words = (C.c_int32 * 16)(*s) if s is not None else None
        sp = C.addressof(words) if s is not None else None
        a = list(a)
        if kind == "demux":
            rc = L.psxhip_str_demux_device(None, sp, *a, None)
        elif kind == "strspu":
            rc = L.psxhip_strspu_demux_device(None, sp, *a, None)
        elif kind == "deint":
            rc = L.psxhip_spu_deinterleave_device(0, *a, None)
        elif kind == "read":
            rc = L.psxhip_str_read_host(None, sp, *a)
        elif kind == "readspu":
            rc = L.psxhip_strspu_read_host(None, sp, *a)
        elif kind == "spustreams":
            rc = L.psxhip_spu_decode_streams_host(0, *a)
        else:
            rc = L.psxhip_xa_decode_streams_host(0, *a)
        out.append((rc, L.psxhip_last_error().decode()))
    return out


@pytest.fixture(scope="module")
def gold():
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "reader_plan_parent.json")))
    assert [(r["kind"], tuple(r["settings"]) if r["settings"] is not None else None, r["args"]) for r in rows] == [(k, s, list(a)) for k, s, a in REFUSALS]
    return [(r["rc"], r["error"]) for r in rows]


# ------------------------------------------------------------------------------------------------ the driver
def run_driver(exe, tmp, calls):
    """the driver's constants, and (rc, error text or list of numbers) per call"""
    src = os.path.join(tmp, "calls.txt")
    with open(src, "w") as f:
        for kind, s, a in calls:
            f.write(" ".join(map(str, [kind, int(s is not None)] + list(s if s is not None else [0] * 16) + [len(a)] + list(a))) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), "the sanitizer build reported:\n" + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[0].startswith("const ") and len(lines) == len(calls) + 1
    out = []
    for (kind, _, _), line in zip(calls, lines[1:]):
        head, rest = line.split(" : ", 1)
        rc, text = rest.split(" |", 1)
        assert head == kind
        out.append((int(rc), text.strip() if int(rc) else text))
    return [int(v) for v in lines[0].split()[1:]], out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build psxavenc_amd/csrc/reader_plan.cpp and tests/cpu/reader_plan_check.cpp")
    tmp = str(tmp_path_factory.mktemp("reader_plan"))
    exe = os.path.join(tmp, "reader_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe,
                    os.path.join(ROOT, "psxavenc_amd/csrc/reader_plan.cpp"), os.path.join(ROOT, "psxavenc_amd/csrc/str_plan.cpp"),
                    os.path.join(ROOT, "tests/cpu/reader_plan_check.cpp")], check=True)
    return lambda calls: run_driver(exe, tmp, calls)


class K:
    """the constants, as the driver prints them"""

    def __init__(self, v):
        (self.scan_block, self.max_chunks, self.sector_rec, self.frame_info, self.decoded, self.summary, self.audio_summary, self.chunk_info, self.state) = v


def ints(text):
    return [int(v) for v in text.split()]


def up(x):
    return (x + 255) // 256 * 256


def placed(offsets, sizes, end):
    """the parts in their order, each 256-byte placed and as long as its kernel indexes, none reaching the next; `end` behind the last"""
    for i, (o, size) in enumerate(zip(offsets, sizes)):
        nxt = offsets[i + 1] if i + 1 < len(offsets) else end
        assert o % 256 == 0 and o + size <= nxt, (i, offsets, sizes, end)
    assert offsets[0] == 0


# ------------------------------------------------------------------------------------------------ refusals
def test_the_plan_refuses_what_the_parent_library_refused(driver, gold):
    """every clause of every refusal with its text, the pairs that fix the precedence, and what is accepted next to them: the plan
    functions, called in the entry points' order, answer as the recorded library did (an accepted call went on to "no device")"""
    _, got = driver(REFUSALS)
    for call, (rc, text), (want_rc, want_text) in zip(REFUSALS, got, gold):
        if want_rc == EINVAL:
            assert (rc, text) == (EINVAL, want_text), call
        else:
            assert rc == 0 and want_rc == EDEVICE, (call, rc, text, want_rc, want_text)
    refused = [g for g in gold if g[0] == EINVAL]
    assert len({t for _, t in refused}) >= 25 and len(refused) < len(gold)


def test_the_library_answers_as_its_parent_did(gold):
    """the built library through ctypes, unsanitized: the same table.  Beside a GPU only the refused calls are made (an accepted one
    would go on to the device with the made-up addresses)"""
    import torch
    from psxavenc_amd import _lib
    L = bind(C.CDLL(_lib.lib()._name))
    pairs = [(c, g) for c, g in zip(REFUSALS, gold) if g[0] == EINVAL or not torch.cuda.is_available()]
    got = library_answers(L, [c for c, _ in pairs])
    for (call, want), answer in zip(pairs, got):
        assert answer == want, call


# ------------------------------------------------------------------------------------------------ the demux workspace
GEOMETRY = {6: (2336, 0, 0x08), 7: (2352, 0x10, 0x18), 9: (2048, -1, 0)}


def test_demux_workspace_parts_hold_what_the_kernels_index(driver):
    """section 13's five steps: the scan records, the table, the block sums, owner / lead / min (one fill with ones), the status words"""
    cases = [(fmt, S, n, mf, bs) for fmt in (6, 7, 9) for S in (1, 2) for n in (0, 1, 256, 257) for mf in (0, 1, 65)
             for bs in (CHUNK, 2 * CHUNK + 100, 65537 * CHUNK)]
    calls = [demux(s=settings(fmt=fmt), S=S, n=n, mf=mf, bs_stride=bs, in_stride=GEOMETRY[fmt][0] * n, bs_stream=bs * mf, cap=n,
                   xa_stream=GEOMETRY[fmt][0] * n) for fmt, S, n, mf, bs in cases]
    consts, got = driver(calls)
    k = K(consts)
    assert k.scan_block == 256 and k.sector_rec == 16
    clamped = 0
    for (fmt, S, n, mf, bs), (rc, text) in zip(cases, got):
        assert rc == 0, (fmt, S, n, mf, bs, text)
        ssz, sub_at, hdr_at, cap, n_blocks, o_rec, o_table, o_blocks, o_owner, o_lead, o_min, o_status, total = ints(text)
        assert (ssz, sub_at, hdr_at) == GEOMETRY[fmt]
        assert cap == min(bs // CHUNK, 65536) and n_blocks == -(-n // k.scan_block)
        clamped += cap < bs // CHUNK
        rows = S * mf
        placed([o_rec, o_table, o_blocks, o_owner, o_status], [S * n * 16, S * n * k.sector_rec, S * n_blocks * 4, (rows * cap + rows + S) * 4, rows * 4], total)
        assert o_lead == o_owner + rows * cap * 4 and o_min == o_lead + rows * 4 and o_min + S * 4 <= o_status          # contiguous
        assert total == sum(up(v) for v in (S * n * 16, S * n * k.sector_rec, S * n_blocks * 4, (rows * cap + rows + S) * 4, rows * 4))
    assert clamped == len(cases) // 3


def test_strspu_demux_plans_the_rules_and_the_audio_workspace(driver):
    cases = [(ch, options, freq, S, cap) for ch in (0, 1, 2) for options in (0x0001, 0x0042 | 0x10000, 0x0001 | 0x20000, 0xFFFF | 0x30000)
             for freq in (0, 44100) for S in (1, 3) for cap in (0, 1, 5)]
    calls = [strspu(s=settings8(ch=ch, options=options, freq=freq), S=S, cap=cap, units_stream=cap * 126 * 16, in_stride=2048 * 4, bs_stream=8064)
             for ch, options, freq, S, cap in cases]
    _, got = driver(calls)
    for (ch, options, freq, S, cap), (rc, text) in zip(cases, got):
        assert rc == 0, text
        audio, video = text.split("|")
        assert ints(audio) == [ch, options & 0xFFFF, 0 if options & 0x20000 else 1, int(bool(options & 0x10000)), freq, S * cap, 2 * S * cap * 4]
        assert ints(video)[:3] == list(GEOMETRY[9])          # the video half is the stream as format 9


def test_deinterleave_plans_blocks_records_and_the_vector_form(driver):
    cases = [(d_in, off, stride, lane, ch, n, S, in_stride) for d_in in (P, P + 4) for off in (0x20, 0x24) for stride in (2064, 2068)
             for lane, ch in ((1008, 2), (2016, 1), (16, 3)) for n in (0, 4) for S, in_stride in ((1, 4), (2, 4 * 2068), (2, 4 * 2068 + 8))]
    calls = [deint(d_in=d_in, lane_offset=off, chunk_stride=stride, lane_bytes=lane, channels=ch, n=n, streams=S, in_stride=in_stride,
                   units_stream=n * ch * lane) for d_in, off, stride, lane, ch, n, S, in_stride in cases]
    _, got = driver(calls)
    forms = set()
    for (d_in, off, stride, lane, ch, n, S, in_stride), (rc, text) in zip(cases, got):
        assert rc == 0, text
        vec16 = (d_in + off) % 16 == 0 and stride % 16 == 0 and (S == 1 or in_stride % 16 == 0)
        assert ints(text) == [lane // 16, n * ch * (lane // 16), int(vec16)]
        forms.add(vec16)
    assert forms == {True, False}


# ------------------------------------------------------------------------------------------------ the _host readers' staging buffer
def parse_read(text):
    parts = text.split("|")
    return ints(parts[0]), ints(parts[1]), [ints(p) for p in parts[2:]]


def check_staging(k, head, offsets, s, n, mf, frames, cap, items):
    """the plan's numbers against the settings, and the parts of the staging buffer"""
    spu, got_n, got_mf, ssz, chunks, bs_stride, frame_bytes, w, h, dc_wrap, got_cap = head[:11]
    fmt, codec, width, height, fps_num, fps_den, speed, ch = s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[9]
    assert (spu, got_n, got_mf, ssz) == (int(fmt == 8), n, mf, 2048 if fmt == 8 else GEOMETRY[fmt][0])
    # the widest frame the rate allows; an STRSPU stream's as the stream's without audio
    interleave = (2 if ch == 2 else 4) * (37800 // s[10]) * (8 // s[11]) * speed if ch and fmt != 8 else 1
    base, den = 75 * speed * max(interleave - 1, 1) * fps_den, interleave * fps_num
    assert chunks == -(-base // den) and bs_stride == chunks * CHUNK
    assert frame_bytes == width * height * 3 // 2 and (w, h, dc_wrap) == (width, height, int(codec == 2))
    assert got_cap == cap and head[14:18] == list(items)
    o_sum, o_asum, o_src, o_units, o_px, reserve = offsets[5], offsets[6], offsets[7], offsets[8], offsets[12], offsets[13]
    src_item, unit_item, info_item, pcm_item = items
    order = offsets[:6] + offsets[7:13]
    sizes = [n * ssz, mf * bs_stride, mf * 4, mf * k.frame_info, mf * k.decoded, k.summary + k.audio_summary, cap * src_item, cap * unit_item,
             cap * info_item, 2 * k.state, cap * pcm_item, 0]
    placed(order, sizes, o_px)
    assert o_units % 16 == 0
    assert o_asum == o_sum + k.summary and o_asum + k.audio_summary <= o_src                # adjacent: one read-back takes both
    assert reserve == o_px + (mf * frame_bytes if frames else 0) + 256 and o_px == sum(up(v) for v in sizes)


def test_read_host_stages_every_xa_layout_and_returns_by_the_rule(driver):
    n, mf = 5, 2
    cases = []
    for fmt in (6, 7):
        for ch in (1, 2):
            for bits in (4, 8):
                sps = 18 * (8 if bits == 4 else 4) * 28
                cases += [(fmt, ch, bits, P, c, P, mf) for c in (sps - 1, sps, 2 * sps + 9, (n + 3) * sps + 5)]
                cases += [(fmt, ch, bits, 0, 10 ** 6, P, mf), (fmt, ch, bits, P, 3 * sps, 0, mf), (fmt, ch, bits, P, 3 * sps, P, 0)]
    cases += [(9, 2, 4, P, 10 ** 6, P, mf), (7, 0, 4, P, 10 ** 6, P, mf), (9, 0, 4, 0, 0, 0, 0)]        # no subheader; no channels
    calls = [read(s=settings(fmt=fmt, ch=ch, bits=bits, width=64, height=48, codec=2 if bits == 8 else 0), n=n, mf=mf_, frames=frames, pcm=pcm,
                  pcm_capacity=c, info=P if mf_ else 0, decoded=P if mf_ else 0) for fmt, ch, bits, pcm, c, frames, mf_ in cases]
    consts, got = driver(calls)
    k = K(consts)
    caps = set()
    for (fmt, ch, bits, pcm, c, frames, mf_), call, (rc, text) in zip(cases, calls, got):
        assert rc == 0, text
        head, offsets, rules = parse_read(text)
        sps = 18 * (8 if bits == 4 else 4) * 28                     # int16 of a sector, all channels together
        cap = min(c // sps, n) if pcm and ch and fmt != 9 else 0
        record = 16 if bits == 4 else 32
        check_staging(k, head, offsets, call[1], n, mf_, bool(frames), cap, (GEOMETRY[fmt][0], sps // 28 * record, 4, sps * 2))
        assert head[11] == ch
        assert [r[0] for r in rules] == [v for v in (0, cap - 1, cap, cap + 1, cap + 7) if v >= 0]          # below, at and above the capacity
        for count, taken, value in rules:
            assert taken == min(count, cap) and value == (taken * sps // ch if ch else 0), (fmt, ch, bits, c, count)
        caps.add(cap)
    assert caps == {0, 1, 2, 3, n}


def test_strspu_read_host_stages_by_the_capacity_rule_and_builds_the_chains(driver):
    kmax = (2 ** 31 - 1) // 126 // 28
    cases = []
    for ch in (1, 2):
        for d in (0, 1):
            B = 126 // ch
            x = 28 * (2 * B - d) * ch
            cases += [(ch, d, 6, P, c, P, 2) for c in (x - 1, x, x + 5, 0, 28 * (B - d) * ch, 10 ** 9)]
            cases += [(ch, d, 700000, P, 28 * ((kmax + 1) * B - d) * ch, P, 2), (ch, d, 700000, P, 28 * (kmax * B - d) * ch - 1, P, 2)]
            cases += [(ch, d, 6, 0, 10 ** 6, P, 2), (ch, d, 6, P, x, 0, 2), (ch, d, 6, P, x, P, 0)]
    cases += [(0, d, 6, P, c, P, 2) for d in (0, 1) for c in (0, 100)]
    calls = [readspu(s=settings8(ch=ch, options=1 | (0 if d else 0x20000), width=64, height=48), n=n, mf=mf, frames=frames, pcm=pcm, pcm_capacity=c,
                     info=P if mf else 0, decoded=P if mf else 0) for ch, d, n, pcm, c, frames, mf in cases]
    consts, got = driver(calls)
    k = K(consts)
    assert k.max_chunks == (2 ** 31 - 1) // 126
    caps = set()
    for (ch, d, n, pcm, c, frames, mf), call, (rc, text) in zip(cases, calls, got):
        assert rc == 0, text
        head, offsets, rules = parse_read(text)
        cap, B = head[10], 126 // ch if ch else 0
        limit = min(n, kmax)
        if not pcm or not ch:
            assert cap == 0
        else:          # the largest nK within the limit with 28 (nK B - d) ch <= pcm_capacity
            assert 0 <= cap <= limit and (cap == 0 or 28 * (cap * B - d) * ch <= c) and (cap == limit or 28 * ((cap + 1) * B - d) * ch > c), (ch, d, n, c, cap)
        check_staging(k, head, offsets, call[1], n, mf, bool(frames), cap, (0, 126 * 16, k.chunk_info, 126 * 28 * 2))
        assert head[11:14] == [ch, d, B]
        for r in rules:
            count, taken, value = r[:3]
            units = max(taken * B - d, 0) if taken else 0
            assert taken == min(count, cap) and value == 28 * units, (ch, d, c, r)
            assert value * ch <= c or not units
            assert r[3:] == ([v for ci in range(ch) for v in (ci, ch, 28 * units, units, ch, d * ch + ci)] if units else []), (ch, d, c, r)
        caps.add(cap if cap < 10 else "max" if cap == kmax else "big")
    assert caps == {0, 1, 2, 6, "max", "big"}


# ------------------------------------------------------------------------------------------------ the ADPCM decoder's host conveniences
def test_streams_host_shapes(driver):
    spu = [(S, nb, in_stride, out_stride) for S in (0, 1, 2, 5) for nb in (0, 1, 10) for in_stride, out_stride in ((16 * nb, 28 * nb), (16 * nb + 48, 28 * nb + 3))]
    xa = [(fmt, stereo, bits, S, n, pad) for fmt in (0, 1) for stereo in (0, 1) for bits in (4, 8) for S in (0, 1, 3) for n in (0, 1, 4) for pad in (0, 100)]
    calls = [spustreams(S=S, n_blocks=nb, in_stride=i, out_stride=o) for S, nb, i, o in spu]
    calls += [xastreams(format=fmt, stereo=stereo, bits=bits, S=S, n_sectors=n, in_stride=(2352 if fmt else 2336) * n + pad,
                        out_stride=18 * (8 if bits == 4 else 4) * 28 * n + pad) for fmt, stereo, bits, S, n, pad in xa]
    consts, got = driver(calls)
    k = K(consts)
    for (S, nb, in_stride, out_stride), (rc, text) in zip(spu, got):
        assert rc == 0, text
        if S == 1:          # one stream ignores the strides
            in_stride, out_stride = 16 * nb, 28 * nb
        assert ints(text) == [1, nb, 28 * nb, 28 * nb, 16 * nb, in_stride, out_stride, S, 0, 16 * nb * S, 16 * nb * S, k.state * S, 2 * 28 * nb * S, 0]
    for (fmt, stereo, bits, S, n, pad), call, (rc, text) in zip(xa, calls[len(spu):], got[len(spu):]):
        assert rc == 0, text
        ch, units, ssz = 1 + stereo, 18 * (8 if bits == 4 else 4) * n, 2352 if fmt else 2336
        per = units // ch * 28 * ch
        in_stride, out_stride = (ssz * n, per) if S == 1 else (call[2][6], call[2][10])
        assert ints(text) == [ch, units, units // ch * 28, per, ssz * n, in_stride, out_stride, S * ch, S * n, ssz * n * S,
                              S * units * (16 if bits == 4 else 32), k.state * S * ch, 2 * per * S, 4 * S * n]
