"""The ADPCM host layer's plan module (psxavenc_amd/csrc/adpcm_plan.cpp) on the CPU, without HIP and under the host sanitizers, the
way tests/test_reader_plan_cpu.py checks the readers': g++ builds adpcm_plan.cpp and the driver (tests/cpu/adpcm_plan_check.cpp,
which brings the error sink) and nothing else.  The driver is handed this file's tables of calls and prints what the plans derive;
the expectations are restatements in Python over the constants the driver prints.  Every case is arithmetic only: addresses are
made up.

tests/golden/adpcm_plan_parent.json holds what the library answered before the plan module existed: (rc, psxhip_last_error()) for
REFUSALS, a table of calls of the entry points the module plans.  It was recorded on a machine without a device, where every refusal
that precedes the device check answers as it does beside a GPU, a call that returns before the device check returns its value, and
an accepted call answers "no device", with

    L = bind(ctypes.CDLL(path_of_that_libpsxav_hip_so))
    json.dump([dict(kind=k, args=a, chains=c, rc=rc, error=text) for (k, a, c), (rc, text) in zip(REFUSALS, library_answers(L, REFUSALS))], f)

The plan module and the library as it is built now both have to reproduce the file exactly.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

from psxavenc_amd import adpcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE = -1, -2
P = 0x100000           # the checks look at values only: made-up addresses, never dereferenced
Q = P + (1 << 24)


def pick(defaults, kw):
    assert set(kw) <= set(defaults), kw
    return [dict(defaults, **kw)[name] for name in defaults]


# ------------------------------------------------------------------------------------------------ the calls, arguments in the entry points' order
def enc(**kw):
    return ("enc", pick(dict(d_samples=P, d_chains=P, d_base=P, n=2, fc=4, bits=4, d_states=P, d_units=Q), kw), None)


def encbeam(**kw):
    return ("encbeam", pick(dict(d_samples=P, d_chains=P, d_base=P, n=2, fc=4, bits=4, beam=2, d_states=P, d_units=Q, d_err=0), kw), None)


def session(**kw):
    return ("session", pick(dict(d_samples=P, chains=P, base=P, lead=0, n=2, fc=4, bits=4, d_units=Q, chunk=64, warm=16), kw), None)


def setbeam(**kw):
    return ("setbeam", pick(dict(session=0, beam=1, speculated=0), kw), None)


def chunked(**kw):
    return ("chunked", pick(dict(d_samples=P, chains=P, base=P, n=2, fc=4, bits=4, d_states=P, d_units=Q, chunk=64, warm=16, passes=0), kw), None)


def chunkedbeam(**kw):
    return ("chunkedbeam", pick(dict(d_samples=P, chains=P, base=P, n=2, fc=4, bits=4, d_states=P, d_units=Q, beam=2, chunk=64, warm=16, passes=0), kw), None)


def pack(**kw):
    return ("pack", pick(dict(d_units=Q, n=4, d_out=P), kw), None)


def scatter(**kw):
    return ("scatter", pick(dict(d_units=Q, n=2, format=1, stereo=1, frequency=37800, bits=4, file=1, channel=0, lba=0, d_eof=0, eof_bits=0, d_out=P,
                                 d_dst=0, S=1, ustride=0, ostride=0), kw), None)


def dec(**kw):
    return ("dec", pick(dict(d_units=Q, d_chains=P, d_base=P, n=2, fc=4, bits=4, d_states=P, d_samples=P, d_flags=0, d_tail=0), kw), None)


def chain(pitch=1, n_units=3, offset=0):
    return [offset, pitch, 28 * n_units, n_units, 1]


def decchunked(chains=(chain(), chain()), **kw):
    """`chains`: the host table the call reads (None: NULL); n defaults to its length"""
    table = [list(c) for c in chains] if chains is not None else None
    d = dict(d_units=Q, chains=P if table is not None else 0, base=P, n=len(table or ()), fc=4, bits=4, d_states=P, d_samples=P, d_flags=0, d_tail=0, chunk=4,
             warm=2, passes=0)
    return ("decchunked", pick(d, kw), table)


def sse(**kw):
    return ("sse", pick(dict(d_a=P, d_a_tail=0, d_b=P, d_chains=P, n=2, d_unit_sse=0, d_unit_base=0, d_sums=P), kw), None)


def dis(**kw):
    return ("dis", pick(dict(d_sectors=P, n=2, format=1, stereo=1, frequency=37800, bits=4, d_units=Q, d_status=0), kw), None)


def spuhost(**kw):
    return ("spuhost", pick(dict(samples=P, S=2, stream_stride=280, pitch=1, n=280, states=P, out=P, out_stride=160), kw), None)


def spuhostbeam(**kw):
    return ("spuhostbeam", pick(dict(samples=P, S=2, stream_stride=280, pitch=1, n=280, states=P, out=P, out_stride=160, beam=2), kw), None)


XA = dict(format=1, stereo=1, frequency=37800, bits=4, file=1, channel=0, samples=P, S=2, stream_stride=4032, n=2016, lbas=0, states=P, out=P,
          out_stride=2352, finalize=1)


def xahost(**kw):
    return ("xahost", pick(XA, kw), None)


def xahostbeam(**kw):
    return ("xahostbeam", pick(dict(XA, beam=2), kw), None)


REFUSALS = [
    # ---- psxhip_adpcm_encode_chains_device, psxhip_adpcm_beam_encode_chains_device
    enc(d_samples=0), enc(d_chains=0), enc(d_base=0), enc(d_states=0), enc(d_units=0), enc(n=-1), enc(fc=3), enc(fc=6), enc(bits=5), enc(d_units=Q + 4),
    enc(bits=8, d_units=Q + 2), enc(d_units=Q + 4, fc=3),
    enc(), enc(bits=8, d_units=Q + 4), enc(fc=5, bits=8), enc(n=0), enc(d_samples=P + 1),
    encbeam(d_samples=0), encbeam(d_chains=0), encbeam(d_base=0), encbeam(d_states=0), encbeam(d_units=0), encbeam(n=-1), encbeam(fc=3), encbeam(bits=5),
    encbeam(beam=0), encbeam(beam=5), encbeam(d_units=Q + 4), encbeam(bits=8, d_units=Q + 2), encbeam(d_err=P + 2), encbeam(beam=0, d_err=P + 2),
    encbeam(), encbeam(beam=1, d_err=P), encbeam(beam=4, bits=8, d_units=Q + 4), encbeam(n=0),
    # ---- psxhip_adpcm_session_create (behind its handle pointer), psxhip_adpcm_session_set_beam without a session
    session(d_samples=0), session(chains=0), session(base=0), session(d_units=0), session(n=-1), session(fc=6), session(bits=16), session(chunk=0),
    session(warm=-1), session(d_units=Q + 8), session(bits=8, d_units=Q + 1), session(chunk=0, d_units=Q + 8),
    session(), session(lead=P), session(n=0), session(bits=8, d_units=Q + 8), session(warm=0, chunk=1),
    setbeam(), setbeam(beam=-1), setbeam(beam=5),
    # ---- psxhip_adpcm_encode_chains_chunked, psxhip_adpcm_beam_encode_chains_chunked: their own refusals, no chains, the session's refusals
    chunked(d_states=0), chunked(d_states=0, n=0), chunked(d_states=0, fc=3), chunked(n=0), chunked(n=0, fc=3, d_units=0), chunked(n=-1), chunked(fc=3),
    chunked(chunk=0), chunked(d_units=Q + 4), chunked(),
    chunkedbeam(beam=0), chunkedbeam(beam=5), chunkedbeam(beam=0, d_states=0), chunkedbeam(d_states=0), chunkedbeam(n=0), chunkedbeam(beam=0, n=0),
    chunkedbeam(n=-1), chunkedbeam(warm=-1), chunkedbeam(), chunkedbeam(beam=4),
    # ---- psxhip_spu_pack_device, psxhip_xa_assemble_scatter
    pack(d_units=0), pack(d_out=0), pack(n=-1), pack(d_out=P + 8), pack(d_units=Q + 8), pack(d_out=0, n=-1), pack(), pack(n=0),
    scatter(d_units=0), scatter(d_out=0), scatter(n=-1), scatter(S=0), scatter(S=65536), scatter(format=2), scatter(bits=5), scatter(d_out=P + 2),
    scatter(ostride=2354), scatter(ustride=18), scatter(S=0, d_out=P + 2),
    scatter(), scatter(n=0), scatter(S=65535, ustride=32, ostride=2352), scatter(format=0, bits=8, stereo=0), scatter(d_units=Q + 4), scatter(d_eof=P + 1, d_dst=P + 1),
    # ---- psxhip_adpcm_decode_chains_device, psxhip_adpcm_decode_chains_chunked with its chains
    dec(n=-1), dec(fc=3), dec(bits=5), dec(fc=5, bits=8), dec(d_units=0), dec(d_chains=0), dec(d_base=0), dec(d_states=0), dec(d_samples=0), dec(d_units=Q + 8),
    dec(d_samples=P + 1), dec(d_tail=P + 2), dec(n=0, d_units=Q + 8), dec(n=-1, fc=3),
    dec(), dec(n=0, d_units=0, d_chains=0, d_base=0, d_states=0, d_samples=0), dec(fc=5), dec(bits=8), dec(d_tail=P + 4, d_flags=P + 1),
    decchunked(n=-1), decchunked(fc=3), decchunked(fc=5, bits=8), decchunked(d_units=0), decchunked(chains=None, n=2), decchunked(base=0), decchunked(d_states=0),
    decchunked(d_samples=0), decchunked(d_units=Q + 8), decchunked(d_samples=P + 1), decchunked(d_tail=P + 2),
    decchunked(chains=(chain(), chain(pitch=0))), decchunked(chains=(chain(n_units=-1), chain(pitch=0))), decchunked(chains=(chain(), chain(), chain(pitch=-2, n_units=-3))),
    decchunked(chains=(chain(pitch=0),), fc=3), decchunked(chains=(chain(pitch=0),), d_tail=P + 2),
    decchunked(), decchunked(chains=()), decchunked(chains=(chain(n_units=0), chain(n_units=0))), decchunked(chunk=0, warm=-1), decchunked(chains=(chain(pitch=2), chain(pitch=2, offset=1))),
    # ---- psxhip_adpcm_sse_device, psxhip_xa_disassemble_device
    sse(n=-1), sse(d_a=0), sse(d_b=0), sse(d_chains=0), sse(d_unit_sse=P), sse(d_a=P + 1), sse(d_b=P + 1), sse(d_a_tail=P + 1), sse(d_unit_sse=P + 4, d_unit_base=P),
    sse(d_sums=P + 4), sse(n=0, d_a=P + 1), sse(n=-1, d_sums=P + 4),
    sse(), sse(n=0, d_a=0, d_b=0, d_chains=0), sse(d_unit_sse=P, d_unit_base=P, d_a_tail=P + 2), sse(d_sums=0), sse(n=0, d_unit_sse=P),
    dis(n=-1), dis(format=2), dis(bits=5), dis(d_sectors=0), dis(d_units=0), dis(d_sectors=P + 2), dis(d_units=Q + 2), dis(d_status=P + 2), dis(n=0, d_units=Q + 2),
    dis(n=-1, format=2), dis(), dis(n=0, d_sectors=0, d_units=0), dis(format=0, bits=8, stereo=0, d_status=P), dis(d_units=Q + 4),
    # ---- psxhip_spu_encode_streams_host, ..._beam: the arguments; nothing to encode; strides (one stream ignores them); zero samples
    spuhost(samples=0), spuhost(states=0), spuhost(out=0), spuhost(S=-1), spuhost(n=-1), spuhost(pitch=0), spuhost(out_stride=159), spuhost(out_stride=-1),
    spuhost(S=-1, out_stride=159), spuhost(S=0, out_stride=0), spuhost(n=0, out_stride=0), spuhost(S=0, n=0), spuhost(S=0, samples=0),
    spuhost(), spuhost(S=1, stream_stride=0, out_stride=0), spuhost(S=1, stream_stride=-5, out_stride=-5), spuhost(n=281, out_stride=176), spuhost(n=281, out_stride=175),
    spuhost(n=1, out_stride=16), spuhost(n=1, out_stride=15), spuhost(pitch=3, stream_stride=1), spuhost(S=5), spuhost(stream_stride=-280),
    spuhostbeam(beam=0), spuhostbeam(beam=5), spuhostbeam(beam=0, samples=0), spuhostbeam(samples=0), spuhostbeam(out_stride=159), spuhostbeam(S=0),
    spuhostbeam(n=0, beam=5), spuhostbeam(n=0), spuhostbeam(), spuhostbeam(S=1, out_stride=0, beam=4),
    # ---- psxhip_xa_encode_streams_host, ..._beam
    xahost(samples=0), xahost(states=0), xahost(out=0), xahost(S=-1), xahost(n=-1), xahost(bits=5), xahost(format=2), xahost(out_stride=2351),
    xahost(format=0, out_stride=2335), xahost(format=2, out_stride=0), xahost(S=0, out_stride=0), xahost(n=0, out_stride=0), xahost(S=0, format=2),
    xahost(), xahost(S=1, stream_stride=0, out_stride=0), xahost(S=1, stream_stride=-1, out_stride=-1), xahost(n=2017, out_stride=2 * 2352), xahost(n=2017, out_stride=2 * 2352 - 1),
    xahost(format=0, stereo=0, bits=8, n=2016, out_stride=2336), xahost(format=0, stereo=0, bits=8, n=2017, out_stride=2336), xahost(n=1), xahost(lbas=P, finalize=0),
    xahostbeam(beam=0), xahostbeam(beam=5), xahostbeam(beam=5, samples=0), xahostbeam(samples=0), xahostbeam(out_stride=2351), xahostbeam(S=0), xahostbeam(n=0, beam=0),
    xahostbeam(n=0), xahostbeam(), xahostbeam(S=1, out_stride=0, beam=1),
]


# ------------------------------------------------------------------------------------------------ the library, through ctypes
CHAIN = C.c_int64 * 3          # psxhip_adpcm_chain_t: an int64 and four int32


def bind(L):
    vp, sz, i32, i64, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_int64, C.c_uint32
    L.psxhip_last_error.restype = C.c_char_p
    L.psxhip_adpcm_encode_chains_device.argtypes = [i32, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    L.psxhip_adpcm_beam_encode_chains_device.argtypes = [i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.psxhip_adpcm_session_create.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, i32, vp, i32, i32, vp]
    L.psxhip_adpcm_session_set_beam.argtypes = [vp, i32]
    L.psxhip_adpcm_encode_chains_chunked.argtypes = [i32, vp, vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, vp]
    L.psxhip_adpcm_beam_encode_chains_chunked.argtypes = [i32, vp, vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp]
    L.psxhip_spu_pack_device.argtypes = [i32, vp, i32, vp, vp]
    L.psxhip_xa_assemble_scatter.argtypes = [i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, u32, vp, vp, i32, sz, sz, vp]
    L.psxhip_adpcm_decode_chains_device.argtypes = [i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.psxhip_adpcm_decode_chains_chunked.argtypes = [i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, i32, i32, vp]
    L.psxhip_adpcm_sse_device.argtypes = [i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.psxhip_xa_disassemble_device.argtypes = [i32, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    L.psxhip_spu_encode_streams_host.argtypes = [i32, vp, i32, i64, i32, i32, vp, vp, i64]
    L.psxhip_spu_encode_streams_host_beam.argtypes = [i32, vp, i32, i64, i32, i32, vp, vp, i64, i32]
    L.psxhip_xa_encode_streams_host.argtypes = [i32, i32, i32, i32, i32, i32, i32, vp, i32, i64, i32, vp, vp, vp, i64, i32]
    L.psxhip_xa_encode_streams_host_beam.argtypes = [i32, i32, i32, i32, i32, i32, i32, vp, i32, i64, i32, vp, vp, vp, i64, i32, i32]
    return L


ENTRY = dict(enc="psxhip_adpcm_encode_chains_device", encbeam="psxhip_adpcm_beam_encode_chains_device", chunked="psxhip_adpcm_encode_chains_chunked",
             chunkedbeam="psxhip_adpcm_beam_encode_chains_chunked", pack="psxhip_spu_pack_device", scatter="psxhip_xa_assemble_scatter",
             dec="psxhip_adpcm_decode_chains_device", decchunked="psxhip_adpcm_decode_chains_chunked", sse="psxhip_adpcm_sse_device",
             dis="psxhip_xa_disassemble_device")
HOST = dict(spuhost="psxhip_spu_encode_streams_host", spuhostbeam="psxhip_spu_encode_streams_host_beam", xahost="psxhip_xa_encode_streams_host",
            xahostbeam="psxhip_xa_encode_streams_host_beam")


def library_answers(L, calls):
    """(rc, psxhip_last_error()) of every call, on device 0 with no stream"""
    out = []
    for kind, a, chains in calls:
        a = list(a)
        if kind == "session":
            handle = C.c_void_p()
            rc = L.psxhip_adpcm_session_create(C.addressof(handle), 0, *a, None)
            assert not handle.value
        elif kind == "setbeam":
            rc = L.psxhip_adpcm_session_set_beam(None, a[1])
        elif kind == "decchunked":
            table = (CHAIN * max(len(chains or ()), 1))()
            for i, (offset, pitch, limit, n_units, stride) in enumerate(chains or ()):
                table[i][:] = [offset, pitch & 0xFFFFFFFF | limit << 32, n_units & 0xFFFFFFFF | stride << 32]
            a[1] = C.addressof(table) if chains is not None else None
            rc = L.psxhip_adpcm_decode_chains_chunked(0, *a, None)
        elif kind in HOST:
            rc = getattr(L, HOST[kind])(0, *a)
        else:
            rc = getattr(L, ENTRY[kind])(0, *a, None)
        out.append((rc, L.psxhip_last_error().decode()))
    return out


@pytest.fixture(scope="module")
def gold():
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "adpcm_plan_parent.json")))
    assert [(r["kind"], r["args"], r["chains"]) for r in rows] == [(k, list(a), c) for k, a, c in REFUSALS]
    return [(r["rc"], r["error"]) for r in rows]


# ------------------------------------------------------------------------------------------------ the driver
def run_driver(exe, tmp, calls):
    """the driver's constants, and (rc, text) per call"""
    src = os.path.join(tmp, "calls.txt")
    with open(src, "w") as f:
        for kind, a, chains in calls:
            a = list(a) + [v for c in chains or () for v in c]
            f.write(" ".join(map(str, [kind, len(a)] + a)) + "\n")
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
        out.append((int(rc), text.strip()))
    return K([int(v) for v in lines[0].split()[1:]]), out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build psxavenc_amd/csrc/adpcm_plan.cpp and tests/cpu/adpcm_plan_check.cpp")
    tmp = str(tmp_path_factory.mktemp("adpcm_plan"))
    exe = os.path.join(tmp, "adpcm_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe,
                    os.path.join(ROOT, "psxavenc_amd/csrc/adpcm_plan.cpp"), os.path.join(ROOT, "tests/cpu/adpcm_plan_check.cpp")], check=True)
    return lambda calls: run_driver(exe, tmp, calls)


class K:
    """the constants, as the driver prints them"""

    def __init__(self, v):
        self.stage_max, self.call_in, self.call_out, self.call_states, self.batch_max, self.chain, self.state, self.record = v


def ask(kind, *a):
    return (kind, list(a), None)


def ints(text):
    return [int(v) for v in text.split()]


def lists(text):
    return [ints(part) for part in text.split("|")]


def up(x):
    return (x + 255) // 256 * 256


def placed(offsets, sizes, end):
    """the parts in their order, each 256-byte placed and as long as its kernel indexes, none reaching the next; `end` behind the last,
    and no larger than the parts' sizes rounded up: the total the block caches saw before"""
    for i, (o, size) in enumerate(zip(offsets, sizes)):
        nxt = offsets[i + 1] if i + 1 < len(offsets) else end
        assert o % 256 == 0 and o + size <= nxt, (i, offsets, sizes, end)
    assert offsets[0] == 0 and end == sum(up(v) for v in sizes)


# ------------------------------------------------------------------------------------------------ refusals
def test_the_plan_refuses_what_the_parent_library_refused(driver, gold):
    """every clause of every refusal with its text, the pairs that fix the precedence, and what is accepted next to them: the plan
    functions, called in the entry points' order, answer as the recorded library did (a call that returned a value before the device
    check returns it here; an accepted call went on to "no device")"""
    _, got = driver(REFUSALS)
    for call, (rc, text), (want_rc, want_text) in zip(REFUSALS, got, gold):
        if want_rc == EINVAL:
            assert (rc, text) == (EINVAL, want_text), call
        elif want_rc == EDEVICE:
            assert (rc, text) == (0, "device"), (call, rc, text, want_text)
        else:
            assert (rc, text) == (0, "early %d" % want_rc), (call, rc, text, want_rc)
    refused = [g for g in gold if g[0] == EINVAL]
    assert len({t for _, t in refused}) >= 20 and any(g[0] == EDEVICE for g in gold) and any(g[0] >= 0 for g in gold)
    assert {k for k, _, _ in REFUSALS} == set(ENTRY) | set(HOST) | {"session", "setbeam"}


def test_the_library_answers_as_its_parent_did(gold):
    """the built library through ctypes, unsanitized: the same table.  Beside a GPU the calls that went on to the device are left out
    (an accepted one would go there with the made-up addresses)"""
    import torch
    from psxavenc_amd import _lib
    L = bind(C.CDLL(_lib.lib()._name))
    pairs = [(c, g) for c, g in zip(REFUSALS, gold) if g[0] != EDEVICE or not torch.cuda.is_available()]
    got = library_answers(L, [c for c, _ in pairs])
    for (call, want), answer in zip(pairs, got):
        assert answer[0] == want[0] and (answer[1] == want[1] or want[0] >= 0), (call, answer, want)


def test_a_session_takes_a_beam_only_while_it_holds_no_records(driver):
    """(a session exists only beside a device: the rule alone)"""
    cases = [(s, beam, spec) for s in (0, 1) for beam in (-1, 0, 1, 4, 5) for spec in (0, 1)]
    _, got = driver([ask("setbeam", *c) for c in cases])
    for (s, beam, spec), (rc, text) in zip(cases, got):
        ok = s and 0 <= beam <= 4 and not spec
        assert rc == (0 if ok else EINVAL) and (ok or text.startswith("adpcm_session_set_beam: bad argument (beam 0 .. 4")), (s, beam, spec)


# ------------------------------------------------------------------------------------------------ route
def test_routes(driver):
    k, _ = driver([])
    assert (k.stage_max, k.call_in, k.call_out, k.call_states, k.batch_max) == (8192, 32768, 16384, 256, 16)
    assert k.call_in >= 2 * k.stage_max and k.call_states >= 4 * k.state          # the block's parts hold what the call kernel stages and leaves
    limits = (k.stage_max, k.call_out)
    stage_units = (k.stage_max - 8) // 28                   # one stream: the last length whose row with its margin is staged whole
    calls = [ask("threshold", 8), ask("threshold", 9), ask("threshold", 1), ask("threshold", 0)]
    calls += [ask("route", u, n) for n, t in ((1, 512), (8, 512), (9, 4096), (1000, 4096)) for u in (t - 1, t)]
    spu = [(0, 4, 1), (0, 5, 1), (0, 1, 511), (0, 1, 512), (0, 0, 0)]          # (one stream of 511 units is past the staging limit already)
    # the staging limit with the threshold out of the way: two streams of 146 units are the last that fit (2 x (28 x 146 + 8) = 8192)
    spu += [(0, 2, 146), (0, 2, 147), (0, 1, stage_units), (0, 1, stage_units + 1), (0, 4, 72), (0, 4, 73)]
    spu += [(beam, S, u) for beam in (1, 4) for S, u in ((1, 1), (4, 1), (1, 511), (2, 146))]
    calls += [ask("spufast", beam, S, u, *limits) for beam, S, u in spu]
    # the output part, with a staging limit that does not bind: 4 x 256 units x 16 bytes fill it exactly; and the route's threshold
    # for one stream with neither limit binding
    out_cases = [(0, 4, 256, 1 << 20, k.call_out), (0, 4, 257, 1 << 20, k.call_out), (0, 1, 511, 1 << 20, 511 * 16), (0, 1, 511, 1 << 20, 511 * 16 - 1),
                 (0, 1, 511, 1 << 20, 1 << 20), (0, 1, 512, 1 << 20, 1 << 20), (1, 1, 511, 1 << 20, 1 << 20)]
    calls += [ask("spufast", *c) for c in out_cases]
    xa = [(0, 1, 6, 4032, 2352), (0, 1, 7, 4032, 2352), (0, 2, 1, 4032, 2352), (0, 1, 1, 4032, 2352), (1, 1, 1, 4032, 2352), (4, 1, 6, 4032, 2352),
          (0, 1, 2, k.stage_max, 2 * 2352), (0, 1, 2, k.stage_max - 7, 2 * 2352), (0, 1, 3, k.stage_max + 1, 3 * 2352), (0, 1, 6, 8064, k.call_out),
          (0, 1, 6, 8064, k.call_out + 1)]
    calls += [ask("xafast", *c, *limits) for c in xa]
    _, got = driver(calls)
    values = [int(text) for rc, text in got]
    assert all(rc == 0 for rc, _ in got)
    assert values[:4] == [512, 4096, 512, 512]
    assert values[4:12] == [0, 1] * 4
    at = 12
    want_spu = [1, 0, 0, 0, 1] + [1, 0, 1, 0, 1, 0] + [0] * 8
    assert stage_units < 512 and 28 * stage_units + 8 <= k.stage_max < 28 * (stage_units + 1) + 8
    assert values[at:at + len(spu)] == want_spu
    at += len(spu)
    assert values[at:at + 7] == [1, 0, 1, 0, 1, 0, 0]
    at += 7
    assert values[at:] == [1, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0]


# ------------------------------------------------------------------------------------------------ chunking
def chunking_totals(rows, n_cu):
    """totals around every branch point of the rule"""
    per_round = 32 * n_cu * rows
    out = {0, 1}
    for fill in (1023, 1024):                                      # `fill` is ceil(total / per_round)
        out |= {per_round * fill - 1, per_round * fill, per_round * fill + 1, per_round * (fill - 1) + 1}
    for rounds in (1, 2, 3):                                       # ceil(fill / 4096) steps behind fill = 4096 x rounds
        out |= {per_round * 4096 * rounds + d for d in (-1, 0, 1)}
    for p in (64, 128, 256, 512, 1024):                            # total // 8192 around twice each power of two
        out |= {8192 * 2 * p + d for d in (-1, 0, 1)} | {8192 * p + d for d in (-1, 0, 1)}
    return sorted(out)


def test_chunking_is_the_python_mirror_s(driver):
    """psxavenc_amd.adpcm.pick_chunking (bench.py and the tools call it) and the plan's rule are one rule"""
    cases = [(t, rows, n_cu) for rows in (4, 5, 64) for n_cu in (1, 64, 256, 304) for t in chunking_totals(rows, n_cu)]
    _, got = driver([ask("chunking", *c) for c in cases])
    seen = set()
    for (t, rows, n_cu), (rc, text) in zip(cases, got):
        assert rc == 0 and tuple(ints(text)) == tuple(adpcm.pick_chunking(t, rows, n_cu)), (t, rows, n_cu, text)
        seen.add(tuple(ints(text)))
    assert {w for _, w in seen} == {16, 32, 64} and {c for c, w in seen if w != 64} == {64, 128, 256, 512, 1024}


def test_the_decoder_chunks_by_its_own_rule_on_top(driver):
    """the encoder's rule for wavefronts of 64 chunks, and at most max(256, total / (4 rounds x 8 wavefronts x 64 chunks x CUs))"""
    cases = [(t, n_cu) for n_cu in (1, 4, 256, 304) for t in chunking_totals(64, n_cu) + [2048 * n_cu * m + d for m in (255, 256, 257, 1023, 1024, 1025) for d in (-1, 0)]]
    _, got = driver([ask("decchunking", *c) for c in cases])
    capped = 0
    for (t, n_cu), (rc, text) in zip(cases, got):
        own = adpcm.pick_chunking(t, 64, n_cu)[0]
        want = min(own, max(256, t // (4 * 8 * 64 * n_cu)))
        assert rc == 0 and int(text) == want, (t, n_cu, text)
        capped += want < own
    assert 0 < capped < len(cases)


# ------------------------------------------------------------------------------------------------ chunk tables and layouts
def unit_counts(c):
    return [0, 1, c - 1, c, c + 1, 2 * c + 1]


def test_session_tables_and_block(driver):
    cases = []
    for c in (1, 2, 7, 64):
        lengths = unit_counts(c)
        for nc in (0, 1, 3, 5):
            for shift in range(len(lengths) if nc else 1):
                n_units = [lengths[(shift + i) % len(lengths)] for i in range(nc)]
                for lead in (None, [(-3, 0, 5, -1, 2)[i] for i in range(nc)]):
                    cases.append((c, n_units, lead))
    calls = [ask("sessionplan", c, int(lead is not None), *[v for u, ld in zip(n_units, lead or [0] * len(n_units)) for v in (u, ld)]) for c, n_units, lead in cases]
    k, got = driver(calls)
    for (c, n_units, lead), (rc, text) in zip(cases, got):
        assert rc == 0
        head, offsets, state_base, chunk_chain, chunk_first, got_lead = lists(text)
        nc, total = len(n_units), sum(n_units)
        want_chain = [i for i, u in enumerate(n_units) for _ in range(0, u, c)]
        want_first = [f for u in n_units for f in range(0, u, c)]
        assert head == [total, len(want_chain)] and chunk_chain == want_chain and chunk_first == want_first
        assert state_base == [sum(n_units[:i]) for i in range(nc)]
        assert got_lead == [max(v, 0) for v in (lead or [0] * nc)]
        nk = len(want_chain)
        sizes = [k.chain * nc, 4 * nc, 8 * nc, 4 * nc, k.state * nc, k.state * nc, nc, 4 * k.batch_max, 4 * nk, 4 * nk, k.state * nk, k.state * total]
        placed(offsets[:-1], sizes, offsets[-1])


def pairs_of(chains):
    """the pair rule as the decoder's kernel needs it: two neighbouring chains of pitch 2, the second one sample behind the first,
    equally long and not empty"""
    out, c = [], 0
    while c < len(chains):
        (o0, p0, u0), (o1, p1, u1) = chains[c], chains[c + 1] if c + 1 < len(chains) else (None, None, None)
        pair = p0 == 2 and p1 == 2 and u0 > 0 and o1 == o0 + 1 and u1 == u0
        out.append((c, 2 if pair else 1))
        c += 2 if pair else 1
    return out


def test_decode_tables_and_workspace(driver):
    L = 9
    shapes = {
        "a true pair": [(0, 2, L), (1, 2, L)],
        "unequal lengths": [(0, 2, L), (1, 2, L - 1)],
        "no units": [(0, 2, 0), (1, 2, 0)],
        "offsets not adjacent": [(0, 2, L), (2, 2, L)],
        "pitch 2 without a partner": [(0, 2, L)],
        "a partner of pitch 1": [(0, 2, L), (1, 1, L)],
        "a pair, then a lone chain": [(0, 2, L), (1, 2, L), (100, 1, 4)],
        "three pitch-2 chains in a row": [(0, 2, L), (1, 2, L), (2, 2, L)],
        "four: two pairs": [(0, 2, L), (1, 2, L), (40, 2, 3), (41, 2, 3)],
        "no chains": [],
    }
    cases = [(name, c, chains) for name, chains in shapes.items() for c in (1, 2, 7, 64)]
    cases += [("lengths", c, [(100 * i, 1, u) for i, u in enumerate(unit_counts(c))][:nc]) for c in (1, 2, 7, 64) for nc in (1, 3, 5)]
    cases += [("pair lengths", c, [(0, 2, u), (1, 2, u)]) for c in (1, 2, 7, 64) for u in unit_counts(c)]
    k, got = driver([ask("decodeplan", c, *[v for ch in chains for v in ch]) for _, c, chains in cases])
    spans = set()
    for (name, c, chains), (rc, text) in zip(cases, got):
        assert rc == 0, (name, text)
        head, offsets, cc, cf, cp, last = lists(text)
        want_cc, want_cf, want_cp, want_last = [], [], [], [-1] * len(chains)
        for first, span in pairs_of(chains):
            spans.add((name, span))
            for f in range(0, chains[first][2], c):
                for j in range(span):
                    want_last[first + j] = len(want_cc)
                    want_cp.append(len(want_cc) - span if f else -1)
                    want_cc.append(first + j)
                    want_cf.append(f)
        assert (cc, cf, cp, last) == (want_cc, want_cf, want_cp, want_last), (name, c)
        nc, nk = len(chains), len(want_cc)
        assert head == [nk]
        placed(offsets[:-1], [k.chain * nc, 4 * nc, 4 * nk, 4 * nk, 4 * nk, 4 * nc, 8 * nk, 8 * nk, 4 * k.batch_max], offsets[-1])
        # every chunk's predecessor is the chunk in front of it in its chain
        for i, pred in enumerate(cp):
            assert pred == -1 and cf[i] == 0 or (cc[pred] == cc[i] and cf[pred] == cf[i] - c)
    assert {s for n, s in spans if n == "a true pair"} == {2} and {s for n, s in spans if n == "three pitch-2 chains in a row"} == {1, 2}
    for name in ("unequal lengths", "no units", "offsets not adjacent", "pitch 2 without a partner", "a partner of pitch 1"):
        assert {s for n, s in spans if n == name} == {1}, name


# ------------------------------------------------------------------------------------------------ the host-buffer encoders' shapes
SAMPLES = (0, 1, 27, 28, 29, 28 * 512)


def test_spu_encode_shapes(driver):
    cases = [(S, n, pitch, pad) for S in (0, 1, 2, 5) for n in SAMPLES for pitch in (1, 2, 3) for pad in (0, 7)]
    calls = [ask("spushape", S, n * pitch + pad, pitch, n, -(-n // 28) * 16 + pad) for S, n, pitch, pad in cases]
    k, got = driver(calls)
    for (S, n, pitch, pad), call, (rc, text) in zip(cases, calls, got):
        assert rc == 0, text
        units = -(-n // 28)
        v = ints(text)
        assert v[:3] == [units, 16 * units, int(S == 0 or units == 0)]
        if v[2]:
            continue
        readable = (n - 1) * pitch + 1
        strides = [readable, 16 * units] if S == 1 else [call[1][1], call[1][4]]          # one stream ignores the strides
        row = -(-28 * units // 8) * 8
        assert v[3:] == strides + [n * pitch, readable, row, 2 * n * pitch * S, k.chain * S, 4 * S, k.state * S, S * units * k.record, S * units * 16]
        assert row >= 28 * units >= n and row % 8 == 0


def test_xa_encode_shapes_and_eof_tables(driver):
    cases = []
    for fmt in (0, 1):
        for stereo in (0, 1):
            for bits in (4, 8):
                ch, group = 1 + stereo, (8 if bits == 4 else 4) * 28
                # per channel: the table's lengths, and totals that end exactly on a group, on a sector, and one sample past each
                lengths = list(SAMPLES) + [group // ch, group // ch + 1, 18 * group // ch, 18 * group // ch + 1, 3 * 18 * group // ch]
                for n in lengths:
                    for S in (0, 1, 3):
                        cases.append((fmt, stereo, bits, S, n, 0, None))
                for S, n in ((1, 18 * group // ch + 1), (3, 18 * group // ch + 1)):
                    sectors = 2
                    cases.append((fmt, stereo, bits, S, n, 1, None))
                    cases.append((fmt, stereo, bits, S, n, 1, [(3 * i + 1) % 4 for i in range(S * sectors)]))
                    cases.append((fmt, stereo, bits, S, n, 0, [0] * (S * sectors)))
    calls = []
    for fmt, stereo, bits, S, n, finalize, flags in cases:
        ch, ssz = 1 + stereo, 2352 if fmt else 2336
        sectors = -(-(-(-n * ch // ((8 if bits == 4 else 4) * 28))) // 18)
        calls.append(ask("xashape", fmt, stereo, bits, S, n * ch + 5, n, sectors * ssz + 3, finalize, int(flags is not None), *(flags or [])))
    k, got = driver(calls)
    for (fmt, stereo, bits, S, n, finalize, flags), call, (rc, text) in zip(cases, calls, got):
        assert rc == 0, text
        ch, ssz, upg = 1 + stereo, 2352 if fmt else 2336, 8 if bits == 4 else 4
        groups = -(-n * ch // (upg * 28))
        sectors = -(-groups // 18)
        parts = lists(text)
        v = parts[0]
        assert v[:5] == [ch, groups, sectors, sectors * ssz, int(S == 0 or sectors == 0)]
        if v[4]:
            assert len(parts) == 1
            continue
        ups = sectors * 18 * upg
        per = n * ch
        strides = [per, sectors * ssz] if S == 1 else [call[1][4], call[1][6]]
        assert v[5:] == [ups, ups // ch] + strides + [per, -(-per // 8) * 8, S * ch, 2 * per * S, k.chain * S * ch, 4 * S * ch, k.state * S * ch, S * ups * k.record,
                                                      S * sectors * ssz, S * sectors]
        want = [int(f) for f in flags] if flags is not None else [int(bool(finalize) and s == sectors - 1) for _ in range(S) for s in range(sectors)]
        assert parts[2] == want
        assert parts[1] == [sum(1 << s for s in range(min(sectors, 32)) if want[s])]          # the fast path's: the first stream's, as bits
