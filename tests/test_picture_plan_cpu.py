"""The picture front ends' plan module (psxavenc_amd/csrc/picture_plan.cpp: scaler, ingest, display) on the CPU, without HIP and under
the host sanitizers, the way tests/test_adpcm_plan_cpu.py checks the ADPCM layer's: g++ builds picture_plan.cpp and the driver
(tests/cpu/picture_plan_check.cpp, which brings the error sink) and nothing else.  The driver is handed this file's tables of calls
and prints what the plans derive; the expectations are restatements in Python over the constants the driver prints.  Every case is
arithmetic only: addresses are made up.

tests/golden/picture_plan_parent.json holds what the library answered before the plan module existed.

"refusals": (rc, psxhip_last_error()) for REFUSALS, recorded through ctypes on a machine without a device, where every refusal that
precedes the device check answers as it does beside a GPU and an accepted call answers "no device" (psxhip_ingest_create and the
three planners need no device at all: their values are recorded).  For the scaler's host convert only the return code is held: it had
no text then.

    [[k, a, rc, text, v] for (k, a), (rc, text, v) in zip(REFUSALS, library_answers(L, REFUSALS))]

"tiles" and "segments": the scaler's decisions sit behind the device check, so they were recorded from the parent's own text: its
psxhip_scaler.cpp compiled by g++ against a stub hip/hip_runtime.h of a few lines (hipMalloc is malloc, hipGetDeviceProperties
answers the case's LDS size and CU count) and a psxhip_scaler_launch that prints the job's tile fields, lds_bytes, vsegs and the
launch's frames and hashes the tables the job points to, driven over TILE_CASES and segment_calls() below (the `gold` fixture
says how the rows are laid out).  That recorder is not part
of the tree.  The plan module has to reproduce the file exactly.
"""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import scaler_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE = -1, -2
P = 0x100000           # made-up addresses, never dereferenced
Q = P + (1 << 26)
RGB, YUV = 0, 1


def pick(defaults, kw):
    assert set(kw) <= set(defaults), kw
    return [dict(defaults, **kw)[name] for name in defaults]


# ------------------------------------------------------------------------------------------------ the calls, arguments in the entry points' order
def screate(**kw):
    return ("screate", pick(dict(fmt=RGB, sw=640, sh=480, full=1, dw=320, dh=240), kw))


def sconvdev(**kw):
    """(no handle exists without a device: handle=1 cases are the plan's alone, see test_the_scaler_converts_refuse)"""
    return ("sconvdev", pick(dict(handle=0, src=P, dst=Q, n=1, sstride=1 << 20, fstride=1 << 20, src_bytes=0, dw=0, dh=0), kw))


def sconvhost(**kw):
    return ("sconvhost", pick(dict(handle=0, src=P, dst=Q, n=1, sstride=0, fstride=0, src_bytes=0, dw=0, dh=0), kw))


def tight_planes(fmt, w, h):
    """(offset, pitch) of a source's planes back to back: YUV420P, YUV420P10, RGB24"""
    b = 2 if fmt == 7 else 1
    if fmt == 12:
        return [(0, 3 * w)]
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return [(0, w * b), (w * h * b, cw * b), (w * h * b + cw * ch * b, cw * b)]


def icreate(planes=None, **kw):
    d = dict(out=1, fmt=0, w=64, h=48, have_planes=1, n_planes=3, matrix=0, full=1, out_format=0, options=0)
    a = pick(d, kw)
    planes = tight_planes(a[1], a[2], a[3]) if planes is None else planes
    return ("icreate", a + [v for p in planes for v in p])


def iconv(kind, **kw):
    d = dict(fmt=0, w=64, h=48, out_format=0, src=P, sstride=64 * 48 * 3 // 2, n_src=2, index=0, n_out=2, dst=Q, ostride=64 * 48 * 3)
    return (kind, pick(d, kw))


def iconvdev(**kw):
    return iconv("iconvdev", **kw)


def iconvhost(**kw):
    return iconv("iconvhost", **kw)


def dconvdev(**kw):
    return ("dconvdev", pick(dict(frames=P, fstride=64 * 48 * 3 // 2, w=64, h=48, n=2, decoded=0, out_format=0, options=0, dst=Q, pitch=192, dstride=192 * 48), kw))


def dconvhost(**kw):
    return ("dconvhost", pick(dict(frames=P, w=64, h=48, n=2, out_format=0, options=0, dst=Q), kw))


def fit(**kw):
    return ("fit", pick(dict(sw=640, sh=480, mw=320, mh=240, ignore=0, out=1), kw))


def recommend(**kw):
    return ("recommend", pick(dict(fmt=0, matrix=0, w=64, h=48), kw))


def pace(pts=(0, 1, 2, 3), **kw):
    return ("pace", pick(dict(have_pts=1, tb_num=1, tb_den=30, fps_num=15, fps_den=1, have_out=1, cap=16), kw) + list(pts))


FRAME = 64 * 48 * 3 // 2
REFUSALS = [
    # ---- psxhip_scaler_create: every clause of the geometry rule; accepted ones go on to the device
    screate(fmt=2), screate(fmt=-1), screate(sw=1), screate(sh=1), screate(sw=16385), screate(sh=16385), screate(dw=8), screate(dh=0), screate(dw=330),
    screate(dh=250), screate(dw=1040), screate(dh=1040), screate(fmt=YUV, sw=641), screate(fmt=YUV, sh=479), screate(fmt=2, dw=8),
    screate(), screate(fmt=YUV), screate(sw=641, sh=479), screate(sw=2, sh=2, dw=1024, dh=1024), screate(sw=16384, sh=16384, dw=16, dh=16), screate(full=0, fmt=YUV),
    # ---- psxhip_scaler_convert_device, _host without a handle
    sconvdev(), sconvdev(src=0), sconvdev(n=0), sconvhost(), sconvhost(n=-1), sconvhost(n=0),
    # ---- psxhip_ingest_create (it needs no device: an accepted call's sizes and matrix are recorded)
    icreate(out=0), icreate(have_planes=0), icreate(out=0, have_planes=0), icreate(fmt=16), icreate(fmt=-1), icreate(n_planes=2), icreate(fmt=12, n_planes=3, planes=[(0, 192)]),
    icreate(w=0), icreate(h=0), icreate(w=16385), icreate(h=16385), icreate(fmt=5, n_planes=1, w=63, planes=[(0, 128)]), icreate(options=2), icreate(options=3),
    icreate(matrix=5), icreate(matrix=-1), icreate(fmt=12, n_planes=1, matrix=9), icreate(out_format=2), icreate(out_format=-1),
    icreate(fmt=12, n_planes=1, out_format=1), icreate(matrix=1, out_format=1), icreate(w=63, out_format=1), icreate(h=47, out_format=1),
    icreate(planes=[(0, 63), (3072, 32), (3840, 32)]), icreate(planes=[(1 << 31, 64), (3072, 32), (3840, 32)]), icreate(planes=[(0, 1 << 31), (3072, 32), (3840, 32)]),
    icreate(fmt=7, planes=[(1, 128), (6144, 64), (7680, 64)]), icreate(fmt=7, planes=[(0, 129), (6400, 64), (8000, 64)]),
    icreate(planes=[(0, 64), (3071, 32), (3840, 32)]), icreate(planes=[(0, 64), (3072, 32), (3072 + 767, 32)]), icreate(planes=[(4608, 64), (0, 32), (16, 32)]),
    icreate(fmt=16, w=0), icreate(n_planes=2, w=0), icreate(w=0, options=2),
    icreate(), icreate(out_format=1), icreate(fmt=12, n_planes=1), icreate(fmt=7), icreate(fmt=7, full=0, matrix=4), icreate(matrix=1, full=0), icreate(matrix=2), icreate(matrix=3),
    icreate(options=1), icreate(w=63, h=47), icreate(planes=[(4608, 64), (0, 32), (768, 32)]), icreate(planes=[(0, 100), (4800, 50), (7200, 50)]),
    # ---- psxhip_ingest_convert_device, _host
    iconvdev(fmt=-1), iconvdev(n_src=-1), iconvdev(n_out=-1), iconvdev(n_out=0), iconvdev(n_out=0, src=0), iconvdev(src=0), iconvdev(dst=0), iconvdev(n_src=0),
    iconvdev(sstride=FRAME - 1), iconvdev(ostride=64 * 48 * 3 - 1), iconvdev(fmt=7, sstride=2 * FRAME + 1), iconvdev(fmt=7, sstride=2 * FRAME, src=P + 1),
    iconvdev(dst=P + FRAME), iconvdev(dst=P + 2 * FRAME - 1), iconvdev(src=Q + 2 * 64 * 48 * 3 - 1), iconvdev(fmt=-1, n_src=-1), iconvdev(n_src=-1, n_out=0),
    iconvdev(), iconvdev(dst=P + 2 * FRAME), iconvdev(fmt=7, sstride=2 * FRAME), iconvdev(index=P), iconvdev(fmt=12, sstride=64 * 48 * 3), iconvdev(out_format=1, ostride=FRAME),
    iconvhost(fmt=-1), iconvhost(n_src=-1), iconvhost(n_out=-1), iconvhost(n_out=0), iconvhost(src=0), iconvhost(dst=0), iconvhost(n_src=0), iconvhost(sstride=FRAME - 1),
    iconvhost(ostride=64 * 48 * 3 - 1), iconvhost(fmt=7, sstride=2 * FRAME + 1), iconvhost(),
    # ---- psxhip_display_convert_device, _host
    dconvdev(n=-1), dconvdev(frames=0), dconvdev(dst=0), dconvdev(w=8), dconvdev(h=1040), dconvdev(w=72, pitch=216, dstride=216 * 48), dconvdev(h=50), dconvdev(out_format=3),
    dconvdev(out_format=-1), dconvdev(options=8), dconvdev(options=2), dconvdev(options=4, out_format=1, pitch=256, dstride=256 * 48), dconvdev(frames=P + 2), dconvdev(fstride=FRAME + 2),
    dconvdev(fstride=FRAME - 4), dconvdev(dst=Q + 1), dconvdev(pitch=194), dconvdev(dstride=192 * 48 + 2), dconvdev(pitch=188), dconvdev(dstride=192 * 48 - 4),
    dconvdev(dst=P + FRAME), dconvdev(dst=P + 2 * FRAME - 4), dconvdev(n=-1, w=8), dconvdev(w=8, out_format=3), dconvdev(out_format=3, options=8),
    dconvdev(), dconvdev(n=0), dconvdev(n=0, frames=0, dst=0), dconvdev(dst=P + 2 * FRAME), dconvdev(out_format=2, options=7, pitch=128, dstride=128 * 48), dconvdev(decoded=P),
    dconvdev(out_format=1, options=1, pitch=256, dstride=256 * 48), dconvdev(pitch=196, dstride=196 * 47 + 192),
    dconvhost(n=-1), dconvhost(frames=0), dconvhost(dst=0), dconvhost(w=0), dconvhost(w=-16), dconvhost(h=-16), dconvhost(h=40), dconvhost(out_format=3), dconvhost(options=2),
    dconvhost(options=16, out_format=2), dconvhost(), dconvhost(n=0), dconvhost(frames=P + 1, dst=Q + 3), dconvhost(out_format=2, options=6), dconvhost(w=1024, h=1024),
    # ---- the planners
    fit(out=0), fit(sw=0), fit(sh=0), fit(mw=8), fit(mh=8), fit(mw=1040), fit(mh=1040), fit(mw=328), fit(mh=250), fit(sw=1, sh=10000, mw=16, mh=1024), fit(sw=10000, sh=1),
    fit(sw=10000, sh=1, ignore=1), fit(), fit(sw=1920, sh=1080), fit(sw=1080, sh=1920), fit(sw=4, sh=3, mw=1024, mh=1024), fit(sw=720, sh=576), fit(sw=853, sh=480, mw=320, mh=240),
    fit(sw=33, sh=17, mw=64, mh=64), fit(sw=3, sh=2, mw=336, mh=240),
    recommend(fmt=16), recommend(fmt=-1), recommend(w=0), recommend(h=0), recommend(), recommend(matrix=1), recommend(w=63), recommend(h=47), recommend(fmt=12), recommend(fmt=11),
    recommend(fmt=7), recommend(fmt=10, matrix=4),
    pace(have_pts=0), pace(tb_num=0), pace(tb_den=0), pace(fps_num=0), pace(fps_den=-1), pace(cap=-1), pace(have_out=0), pace(pts=(0, 10 ** 12), tb_den=1),
    pace(pts=()), pace(pts=(), have_pts=0, have_out=0, cap=0), pace(), pace(cap=2), pace(cap=0, have_out=0), pace(pts=(0, 2, 4, 6, 7, 8, 30)), pace(pts=(5, 5, 5, 6, 3, 9)),
    pace(pts=(100, 101, 104, 110), tb_num=1001, tb_den=30000, fps_num=30000, fps_den=1001), pace(pts=(0, 3, 6), fps_num=30), pace(pts=(-4, -2, 0, 2)),
]

# ---- the scaler's decisions: (format, source, full range, target), as scaler_model and the edge tests name them
GEOMETRIES = M.TILE_GEOMETRIES + M.EXTREME_GEOMETRIES + [(RGB, 2560, 1440, True, 320, 240), (RGB, 2561, 1441, True, 320, 240), (RGB, 640, 480, True, 320, 240),
                                                         (YUV, 640, 480, True, 320, 240)]
# ... and a ">16x" refusal per bank: luma horizontal, luma vertical, chroma horizontal, chroma vertical
GEOMETRIES += [(YUV, 5200, 480, True, 320, 240), (YUV, 640, 3900, True, 320, 240), (RGB, 2600, 480, True, 320, 240), (RGB, 640, 1930, True, 320, 240)]
DEVICES = [(163840, 256), (65536, 256)]
FORCED = [-1, 0, 1, 2, 3, 4]
TILE_CASES = [(g, dev, forced) for g in GEOMETRIES for dev in DEVICES for forced in FORCED]


def tile_call(g, dev, forced):
    fmt, sw, sh, full, dw, dh = g
    return ("tile", [fmt, sw, sh, int(full), dw, dh, dev[0], dev[1], forced])


def segment_frames(n_cu, tiles_x):
    edge = 4 * n_cu // tiles_x
    return sorted({1, 2, max(edge, 1), edge + 1, 65535, 65536, 200000})


def segment_calls(n_cu, tiles_x, tiles_y):
    return [("vsegs", [n_cu, tiles_x, tiles_y, n, -1]) for n in segment_frames(n_cu, tiles_x)] + [("vsegs", [n_cu, tiles_x, tiles_y, 1, o]) for o in (0, 1, tiles_y + 5)]


# ------------------------------------------------------------------------------------------------ the library, through ctypes
class Plane(C.Structure):
    _fields_ = [("offset", C.c_size_t), ("pitch", C.c_size_t)]


def bind(L):
    vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    L.psxhip_last_error.restype = C.c_char_p
    L.psxhip_scaler_create.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32]
    L.psxhip_scaler_convert_device.argtypes = [vp, vp, sz, i32, vp, sz, vp]
    L.psxhip_scaler_convert_host.argtypes = [vp, vp, i32, vp]
    L.psxhip_ingest_create.argtypes = [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, u32]
    L.psxhip_ingest_destroy.argtypes = [vp]
    L.psxhip_ingest_destroy.restype = None
    L.psxhip_ingest_output_bytes.argtypes = L.psxhip_ingest_source_bytes.argtypes = [vp]
    L.psxhip_ingest_output_bytes.restype = L.psxhip_ingest_source_bytes.restype = sz
    L.psxhip_ingest_matrix.argtypes = [vp, vp]
    L.psxhip_ingest_convert_device.argtypes = [vp, vp, sz, i32, vp, i32, vp, sz, vp]
    L.psxhip_ingest_convert_host.argtypes = [vp, vp, sz, i32, vp, i32, vp, sz]
    L.psxhip_display_convert_device.argtypes = [i32, vp, sz, i32, i32, i32, vp, i32, u32, vp, sz, sz, vp]
    L.psxhip_display_convert_host.argtypes = [i32, vp, i32, i32, i32, i32, u32, vp]
    L.psxhip_ingest_fit.argtypes = [i32, i32, i32, i32, i32, vp, vp]
    L.psxhip_ingest_recommend.argtypes = [i32, i32, i32, i32]
    L.psxhip_ingest_pace.argtypes = [vp, i32, i32, i32, i32, i32, vp, i32]
    return L


def plane_table(pairs):
    t = (Plane * max(len(pairs), 1))()
    for i, (o, p) in enumerate(pairs):
        t[i].offset, t[i].pitch = o, p
    return t


def library_answers(L, calls):
    """(rc, psxhip_last_error(), values) of every call, on device 0 with no stream"""
    out = []
    for kind, a in calls:
        values = None
        if kind == "screate":
            handle = C.c_void_p()
            rc = L.psxhip_scaler_create(C.addressof(handle), 0, *a)
            assert not handle.value
        elif kind == "sconvdev":
            assert not a[0]
            rc = L.psxhip_scaler_convert_device(None, a[1], a[4], a[3], a[2], a[5], None)
        elif kind == "sconvhost":
            assert not a[0]
            rc = L.psxhip_scaler_convert_host(None, a[1], a[3], a[2])
        elif kind == "icreate":
            handle = C.c_void_p()
            t = plane_table(list(zip(a[10::2], a[11::2])))
            rc = L.psxhip_ingest_create(C.addressof(handle) if a[0] else None, 0, a[1], a[2], a[3], C.addressof(t) if a[4] else None, *a[5:10])
            if rc == 0:
                m = (C.c_int32 * 7)()
                assert L.psxhip_ingest_matrix(handle, m) == 0
                values = [L.psxhip_ingest_source_bytes(handle), L.psxhip_ingest_output_bytes(handle)] + list(m)
                L.psxhip_ingest_destroy(handle)
        elif kind in ("iconvdev", "iconvhost"):
            handle = C.c_void_p()
            if a[0] >= 0:
                planes = tight_planes(a[0], a[1], a[2])
                t = plane_table(planes)
                assert L.psxhip_ingest_create(C.addressof(handle), 0, a[0], a[1], a[2], C.addressof(t), len(planes), 0, 1, a[3], 0) == 0
            tail = [None] if kind == "iconvdev" else []
            rc = getattr(L, "psxhip_ingest_convert_device" if kind == "iconvdev" else "psxhip_ingest_convert_host")(handle, *a[4:], *tail)
            L.psxhip_ingest_destroy(handle)
        elif kind == "dconvdev":
            rc = L.psxhip_display_convert_device(0, *a, None)
        elif kind == "dconvhost":
            rc = L.psxhip_display_convert_host(0, *a)
        elif kind == "fit":
            w, h = C.c_int(-1), C.c_int(-1)
            rc = L.psxhip_ingest_fit(*a[:5], C.addressof(w) if a[5] else None, C.addressof(h) if a[5] else None)
            values = [w.value, h.value] if rc == 0 else None
        elif kind == "recommend":
            rc = L.psxhip_ingest_recommend(*a)
            values = [rc] if rc >= 0 else None
        else:
            assert kind == "pace"
            pts = (C.c_int64 * max(len(a) - 7, 1))(*a[7:])
            idx = (C.c_int32 * (max(a[6], 0) + 1))()
            rc = L.psxhip_ingest_pace(C.addressof(pts) if a[0] else None, len(a) - 7, *a[1:5], C.addressof(idx) if a[5] else None, a[6])
            values = [rc] + list(idx)[:min(rc, a[6])] if rc >= 0 else None
        out.append((rc, L.psxhip_last_error().decode(), values))
    return out


@pytest.fixture(scope="module")
def gold():
    """the file, a row a line, as the rows the tests compare with: "refusals" [kind, args, rc, error, values]; "banks" [geometry, taps, SHA-256]
    (a geometry's banks are the same on every device and with every tile); "tiles" [case, rc, tile fields or error]; "segments" [[CUs,
    tiles_x, tiles_y], [[n_frames, override, vsegs, launches], ...]]"""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "picture_plan_parent.json")))
    banks = {tuple(geometry): (taps, sha) for geometry, taps, sha in g["banks"]}
    tiles = [dict(case=case, rc=rc, error=v) if rc else dict(case=case, rc=0, fields=v, taps=banks[tuple(case[:6])][0], sha256=banks[tuple(case[:6])][1])
             for case, rc, v in g["tiles"]]
    segments = [dict(case=shape + [n, o], vsegs=v, launches=launches) for shape, rows in g["segments"] for n, o, v, launches in rows]
    return dict(refusals=[dict(kind=k, args=a, rc=rc, error=e, values=v) for k, a, rc, e, v in g["refusals"]], tiles=tiles, segments=segments)


@pytest.fixture(scope="module")
def gold_refusals(gold):
    rows = gold["refusals"]
    assert [(r["kind"], r["args"]) for r in rows] == [(k, list(a)) for k, a in REFUSALS]
    return [(r["rc"], r["error"], r["values"]) for r in rows]


# ------------------------------------------------------------------------------------------------ the driver
def build_driver(tmp, flags):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build psxavenc_amd/csrc/picture_plan.cpp and tests/cpu/picture_plan_check.cpp")
    exe = os.path.join(tmp, "picture_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, "-o", exe, os.path.join(ROOT, "psxavenc_amd/csrc/picture_plan.cpp"),
                    os.path.join(ROOT, "tests/cpu/picture_plan_check.cpp")], check=True)
    return exe


def run_driver(exe, tmp, calls):
    """the driver's constants, (rc, text) per call, and the blob of bank tables"""
    src, blob = os.path.join(tmp, "calls.txt"), os.path.join(tmp, "banks.bin")
    with open(src, "w") as f:
        for kind, a in calls:
            f.write(" ".join(map(str, [kind, len(a)] + list(a))) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, blob], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), "the driver reported:\n" + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[0].startswith("const ") and len(lines) == len(calls) + 1
    out = []
    for (kind, _), line in zip(calls, lines[1:]):
        head, rest = line.split(" : ", 1)
        rc, text = rest.split(" |", 1)
        assert head == kind
        out.append((int(rc), text.strip()))
    return K([int(v) for v in lines[0].split()[1:]]), out, open(blob, "rb").read()


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("picture_plan"))
    exe = build_driver(tmp, SANITIZE)
    return lambda calls: run_driver(exe, tmp, calls)


class K:
    """the constants, as the driver prints them"""

    def __init__(self, v):
        self.plane_pad, self.slack, self.tile_row_bytes, self.launch_frames = v[:4]
        self.shapes = list(zip(v[4::2], v[5::2]))


def ints(text):
    return [int(v) for v in text.split()]


def lists(text):
    return [ints(part) for part in text.split("|")]


class Tile:
    """an accepted "tile" answer"""
    REGIONS = ("p0", "p1", "p2", "tmp_l", "tmp_c", "g_lh", "g_ch", "l_lh", "l_ch", "v_tab", "t_rows")

    def __init__(self, text, blob):
        head, lds, banks = lists(text)
        self.TW, self.TH, self.reg_rows, self.reg_cols, self.creg_rows, self.creg_cols, self.tiles_x, self.tiles_y, self.lds_bytes = head
        self.plane_bytes, self.cplane_bytes, self.ring_l, self.ring_c, self.v_words = lds[:5]
        self.offsets = dict(zip(self.REGIONS, lds[5:16]))
        self.total = lds[16]
        self.banks = []
        for i in range(4):
            taps, taps4, at, nl, nc, nd = banks[6 * i:6 * i + 6]
            self.banks.append(dict(taps=taps, taps4=taps4, left=np.frombuffer(blob, "<i4", nl // 4, at), coef=np.frombuffer(blob, "<i2", nc // 2, at + nl).reshape(-1, taps),
                                   digits=np.frombuffer(blob, "<u4", nd // 4, at + nl + nc), sha=hashlib.sha256(blob[at:at + nl + nc + nd]).hexdigest()))

    def fields(self):
        return [self.TW, self.TH, self.reg_rows, self.reg_cols, self.creg_rows, self.creg_cols, self.tiles_x, self.tiles_y, self.lds_bytes]


# ------------------------------------------------------------------------------------------------ refusals
def compare(call, got, want):
    (rc, text), (want_rc, want_text, values) = got, want
    if want_rc == EDEVICE:
        assert (rc, text) == (0, "device"), (call, got, want)
    elif want_rc < 0:
        assert rc == want_rc and (text == want_text or call[0] == "sconvhost"), (call, got, want)
    elif values is not None:
        flat = [int(v) for v in text.replace("|", " ").split()]
        assert rc == 0 and flat == values, (call, got, want)
    else:
        assert (rc, text) == (0, "early %d" % want_rc), (call, got, want)


def test_the_plan_refuses_what_the_parent_library_refused(driver, gold_refusals):
    """every clause of every refusal with its text, pairs that fix the precedence, and what is accepted next to them"""
    _, got, _ = driver(REFUSALS)
    for call, g, want in zip(REFUSALS, got, gold_refusals):
        compare(call, g, want)
    refused = [g for g in gold_refusals if g[0] == EINVAL]
    assert len({t for _, t, _ in refused}) >= 50 and any(g[0] == EDEVICE for g in gold_refusals) and any(g[2] for g in gold_refusals)
    assert {k for k, _ in REFUSALS} == {"screate", "sconvdev", "sconvhost", "icreate", "iconvdev", "iconvhost", "dconvdev", "dconvhost", "fit", "recommend", "pace"}
    # the one text this layer gained: the scaler's host convert names itself like the device entry does
    host = [g for c, g in zip(REFUSALS, got) if c[0] == "sconvhost" and g[0]]
    assert host and all(text == "psxhip_scaler_convert_host: NULL argument" for _, text in host)


def test_the_library_answers_as_its_parent_did(gold_refusals):
    """the built library through ctypes, unsanitized: the same table.  Beside a GPU the calls that went on to the device are left out
    (an accepted one would go there with the made-up addresses)"""
    import torch
    from psxavenc_amd import _lib
    L = bind(C.CDLL(_lib.lib()._name))
    pairs = [(c, g) for c, g in zip(REFUSALS, gold_refusals) if g[0] != EDEVICE or not torch.cuda.is_available()]
    got = library_answers(L, [c for c, _ in pairs])
    for (call, want), answer in zip(pairs, got):
        assert answer[0] == want[0] and answer[2] == want[2] and (answer[1] == want[1] or want[0] >= 0 or call[0] == "sconvhost"), (call, answer, want)


def test_the_scaler_converts_refuse(driver):
    """with a handle (one exists only beside a device: the rule alone).  A 640x480 RGB source to 320x240"""
    sb, fb = 640 * 480 * 3, 320 * 240 * 3 // 2
    h = dict(handle=1, src_bytes=sb, dw=320, dh=240)
    dev = [dict(), dict(src=0), dict(dst=0), dict(n=-1), dict(n=0), dict(n=0, sstride=0), dict(sstride=sb - 1), dict(fstride=fb - 4), dict(fstride=fb + 2), dict(dst=Q + 2),
           dict(sstride=sb, fstride=fb), dict(n=70000, sstride=sb, fstride=fb)]
    host = [dict(), dict(src=0), dict(dst=0), dict(n=-1), dict(n=0), dict(dst=Q + 1)]
    _, got, _ = driver([sconvdev(**dict(h, **kw)) for kw in dev] + [sconvhost(handle=1, **kw) for kw in host])
    null = "psxhip_scaler_convert_%s: NULL argument"
    strides = "psxhip_scaler_convert_device: strides too small, or the output not 4-byte aligned"
    want = [(0, "device"), (EINVAL, null % "device"), (EINVAL, null % "device"), (EINVAL, null % "device"), (0, "early 0"), (0, "early 0"), (EINVAL, strides), (EINVAL, strides),
            (EINVAL, strides), (EINVAL, strides), (0, "device"), (0, "device")]
    want += [(0, "device"), (EINVAL, null % "host"), (EINVAL, null % "host"), (EINVAL, null % "host"), (0, "early 0"), (0, "device")]
    assert got == want


# ------------------------------------------------------------------------------------------------ the scaler's decisions
@pytest.fixture(scope="module")
def tiles(driver):
    k, got, blob = driver([tile_call(*c) for c in TILE_CASES])
    return k, [(rc, text, Tile(text, blob) if rc == 0 else None) for rc, text in got]


def test_tiles_are_the_parent_s(tiles, gold):
    """tile fields, lds_bytes, the banks' taps and the tables' hashes, or the refusal with its text"""
    _, got = tiles
    rows = gold["tiles"]
    assert [r["case"] for r in rows] == [list(tile_call(*c)[1]) for c in TILE_CASES]
    kinds = set()
    for c, (rc, text, t), r in zip(TILE_CASES, got, rows):
        if r["rc"]:
            assert (rc, text) == (r["rc"], r["error"]), c
            kinds.add(r["error"].split(":")[1][:24])
        else:
            assert rc == 0 and t.fields() == r["fields"] and [b["taps"] for b in t.banks] == r["taps"] and [b["sha"] for b in t.banks] == r["sha256"], (c, text, r)
    # all of: bad PSXHIP_SCALER_TILE, each bank's ">16x", a forced tile that does not fit, no tile fits
    assert len(kinds) >= 7, kinds
    chosen = {(c[1][0], t.TW, t.TH) for c, (rc, _, t) in zip(TILE_CASES, got) if rc == 0 and c[2] == -1}
    assert len({s[1:] for s in chosen if s[0] == 65536}) >= 3, chosen          # the smaller device makes the smaller tiles the natural choice


def test_the_lds_total_is_the_sum_of_its_regions(tiles):
    """scaler_layout.h's carve, region by region, from the job's fields alone"""
    k, got = tiles
    assert (k.plane_pad, k.slack, k.tile_row_bytes) == (8, 16, 16)
    for c, (rc, _, t) in zip(TILE_CASES, got):
        if rc:
            continue
        yuv = c[0][0] == YUV
        up16 = lambda v: (v + 15) // 16 * 16
        plane = up16(t.reg_rows * t.reg_cols + k.plane_pad)
        cplane = up16(t.creg_rows * t.creg_cols + k.plane_pad) if yuv else plane
        ring_c = t.creg_rows if yuv else t.reg_rows
        lv, cv, lh, ch = t.banks[1]["taps"], t.banks[3]["taps"], t.banks[0]["taps4"], t.banks[2]["taps4"]
        v_words = t.TH + t.TH // 2 + (t.TH * lv + t.TH // 2 * cv + 1) // 2
        sizes = [plane, cplane, cplane, 2 * t.reg_rows * t.TW, 2 * 2 * ring_c * (t.TW // 2), 4 * t.TW * 2 * lh, 4 * (t.TW // 2) * 2 * ch, 4 * t.TW, 4 * (t.TW // 2),
                 4 * 2 * v_words, k.tile_row_bytes * t.tiles_y]
        at = 0
        for name, size in zip(Tile.REGIONS, sizes):
            assert t.offsets[name] == at and at % 4 == 0, (c, name)
            at += size
        assert t.total == at + k.slack == t.lds_bytes, c
        assert (t.plane_bytes, t.cplane_bytes, t.ring_l, t.ring_c, t.v_words) == (plane, cplane, t.reg_rows, ring_c, v_words)
        assert (t.tiles_x, t.tiles_y) == (-(-c[0][4] // t.TW), -(-c[0][5] // t.TH))


def reach(b, c, n, tile, align):
    best = 0
    for a in range(0, n, tile):
        e = min(a + tile, n) - 1
        lo, hi = int(b["left"][a]), int(b["left"][e]) + b["taps"]
        if c is not None:
            lo, hi = min(lo, int(c["left"][a // 2])), max(hi, int(c["left"][e // 2]) + c["taps"])
        best = max(best, -(-hi // align) * align - lo // align * align)
    return best


def test_the_tile_is_the_first_that_fits_twice(tiles):
    """... else the last or the forced one if it fits once; the regions' capacities are the banks' reach"""
    k, got = tiles
    assert k.shapes == [(64, 16), (32, 16), (32, 8), (16, 8)]
    by_case = {(c[0], c[1], c[2]): g for c, g in zip(TILE_CASES, got)}
    for g in GEOMETRIES:
        for dev in DEVICES:
            forced = [by_case[(g, dev, f)] for f in (0, 1, 2, 3)]
            if all(rc and "shrinks by more than 16x" in text for rc, text, _ in forced):
                continue
            need = []
            for f, (rc, text, t) in enumerate(forced):          # a forced tile is taken when it fits once: its need either way
                need.append(t.lds_bytes if rc == 0 else int(text.split(" needs ")[1].split()[0]))
                assert (rc == 0) == (need[f] <= dev[0]) and (rc or (t.TW, t.TH) == k.shapes[f]), (g, dev, f)
            rc, text, t = by_case[(g, dev, -1)]
            first = next((f for f in range(4) if 2 * need[f] <= dev[0]), 3 if need[3] <= dev[0] else None)
            if first is None:
                assert rc == EINVAL and text == "psxhip_scaler_create: the filters' reach (%d bytes of LDS per tile) does not fit a compute unit" % need[3], (g, dev)
            else:
                assert rc == 0 and (t.TW, t.TH) == k.shapes[first] and t.fields() == forced[first][2].fields(), (g, dev)
            assert by_case[(g, dev, 4)][:2] == (EINVAL, "psxhip_scaler_create: PSXHIP_SCALER_TILE=4 is not a tile shape (0..3)")
            for rc, _, t in forced:
                if rc:
                    continue
                lh, lv, ch, cv = t.banks
                dw, dh = g[4], g[5]
                if g[0] == YUV:
                    want = [reach(lv, None, dh, t.TH, 1), reach(lh, None, dw, t.TW, 16), reach(cv, None, dh // 2, t.TH // 2, 1), reach(ch, None, dw // 2, t.TW // 2, 16)]
                else:
                    want = [reach(lv, cv, dh, t.TH, 1), reach(lh, ch, dw, t.TW, 4)] * 2
                assert [t.reg_rows, t.reg_cols, t.creg_rows, t.creg_cols] == want, (g, dev, t.TW, t.TH)


def test_the_banks_are_the_model_s(tiles):
    """where tests/scaler_model.py is exact: the number of taps and every output's first source position; beside them every row of
    taps sums to 16384 and the digits restate the taps (the weights themselves are held by the hashes of the recording)"""
    _, got = tiles
    seen = set()
    for c, (rc, _, t) in zip(TILE_CASES, got):
        g = c[0]
        if rc or g in seen:
            continue
        seen.add(g)
        fmt, sw, sh, _, dw, dh = g
        csw, csh = (sw // 2, sh // 2) if fmt == YUV else (sw, sh)
        for b, (src, dst) in zip(t.banks, [(sw, dw), (sh, dh), (csw, dw // 2), (csh, dh // 2)]):
            xi = M.xinc(src, dst)
            scale = max(xi, M.ONE)
            centre = np.arange(dst, dtype=np.int64) * xi + ((xi - M.ONE) >> 1)
            assert b["taps"] == -(-4 * scale // M.ONE) and b["taps4"] == -(-b["taps"] // 4)
            assert (b["left"] == (centre - 2 * scale) // M.ONE + 1).all() and len(b["left"]) == dst
            coef = b["coef"].astype(np.int64)
            assert (coef.sum(axis=1) == 16384).all()
            lo = ((coef + 128) & 255) - 128
            hi = (coef - lo) >> 8
            d = b["digits"].reshape(dst, 2, b["taps4"]).view(np.uint8).reshape(dst, 2, 4 * b["taps4"]).view(np.int8)
            assert (d[:, 0, :b["taps"]] == lo).all() and (d[:, 1, :b["taps"]] == hi).all() and not d[:, :, b["taps"]:].any()
    assert len(seen) >= 8


def test_segments_and_launches_are_the_parent_s(driver, tiles, gold):
    """vsegs for n_frames around the point where the chip is full, the overrides, and the cut of long calls; with the restatement:
    enough segments for four workgroups per CU, within 1 .. tiles_y"""
    k, got = tiles
    shapes = sorted({(dev[1], t.tiles_x, t.tiles_y) for (g, dev, f), (rc, _, t) in zip(TILE_CASES, got) if rc == 0})
    calls = [c for s in shapes for c in segment_calls(*s)]
    _, answers, _ = driver(calls)
    rows = gold["segments"]
    assert [r["case"] for r in rows] == [list(a) for _, a in calls]
    seen = set()
    for (_, (n_cu, tx, ty, n, override)), (rc, text), r in zip(calls, answers, rows):
        (vsegs,), launches = lists(text)
        assert rc == 0 and vsegs == r["vsegs"] and launches == r["launches"], (n_cu, tx, ty, n, override)
        want = override if override >= 0 else -(-4 * n_cu // (tx * n))
        assert vsegs == min(max(want, 1), ty)
        assert sum(launches) == n and all(v == k.launch_frames for v in launches[:-1]) and 0 < launches[-1] <= k.launch_frames
        seen.add(len(launches))
    assert seen == {1, 2, 4}
