"""The MDEC encoder's plan module (psxavenc_amd/csrc/mdec_plan.cpp) on the CPU, without HIP and under the host sanitizers, the way
tests/test_str_plan_cpu.py checks the STR muxer's: g++ builds mdec_plan.cpp and the driver (tests/cpu/mdec_plan_check.cpp, which brings
the error sink) and nothing else; the driver prints what the module derives, and the expectations are restatements in Python -- over
the layout constants the driver prints, so that a changed constant is a changed working set here too.

tests/golden/mdec_plan_parent.json holds what the library computed before the plan module existed (psxhip_mdec_pass_table and
psxhip_mdec_split_geometry run without a device); the module has to reproduce it exactly.  It was recorded from that library with

    L = ctypes.CDLL(path_of_that_libpsxav_hip_so)
    for (w, h) in SIZES, large in (0, 1):       # SIZES: the sizes of the file's "pass_table" entries
        n = L.psxhip_mdec_pass_table(w, h, large, None, 0); buf = (c_uint32 * (2 * (n + 1)))()
        L.psxhip_mdec_pass_table(w, h, large, buf, n + 1)  ->  n, sha256(bytes(buf))
    for args in CASES:                          # the "args" of the file's "split_geometry" entries
        g = Geo()                               # psxhip_mdec_split_geo_t: 3 x int, 6 x size_t
        rc = L.psxhip_mdec_split_geometry(*args, byref(g))  ->  rc, the nine fields of g in their order
"""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
SIZES = (16, 48, 160, 320, 640, 1024)
BUDGETS = (8, 512, 8192, 20000, 80000, 131072, 262140)
MID = -999999          # how the driver prints "mid"


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build psxavenc_amd/csrc/mdec_plan.cpp and tests/cpu/mdec_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("mdec_plan") / "mdec_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe,
                    os.path.join(ROOT, "psxavenc_amd/csrc/mdec_plan.cpp"), os.path.join(ROOT, "tests/cpu/mdec_plan_check.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("PSXHIP_MDEC_SPLIT_M", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), "the sanitizer build reported:\n" + r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        out.setdefault(kind, []).append(rest)
    return out


def ints(text):
    return [int(v) for v in text.split()]


def pairs(rows):
    """"a b c : x y z" -> ([a, b, c], [x, y, z])"""
    for line in rows:
        head, rest = line.split(" : ")
        yield ints(head), ints(rest)


def up(x, a):
    return (x + a - 1) // a * a


class K:
    """the layout constants, as the driver prints them"""

    def __init__(self, lines):
        (self.waves_small, self.waves_large, self.tile_stride, self.z_stride, self.pilot_max, self.max_tiles, self.no_mb, self.s_count, self.wave_tile_bytes,
         self.lut, self.split_waves, self.split_round, self.split_rounds, self.split_wbuf_words) = ints(lines["const"][0])

    def waves(self, large):
        return self.waves_large if large else self.waves_small

    def lds_bytes(self, nmb, out_words, stg_words, large):
        """the frame kernel's working set: what is sized at compile time first, then the arrays sized by the geometry"""
        b = self.s_count * 4 + self.lut * 2
        b = up(b, 4) + self.lut * 4 + 32
        b = up(b, 16) + 2 * 64 * 16 + 2 * 64 + self.waves(large) * self.wave_tile_bytes
        b = up(b, 16) + out_words * 4 + stg_words * 4 + nmb * 4 + nmb * 4
        b += (2 * ((nmb + 63) >> 6) + ((4 * nmb + 63) >> 6)) * 16 + nmb * 6 * 2
        return up(b, 16)

    def split_lds_bytes(self, codec, M, nmb):
        b = 96 * 4 + up(self.lut * 2, 16) + up(self.lut * 4, 16) + M * 6 * 64 * 2 + M * self.split_round * 4 + M * 8 * 2
        b += self.split_waves * self.split_wbuf_words * 4
        if codec:
            b += up(nmb * 6 * 2, 16) + (2 * ((nmb + 511) >> 9) + ((4 * nmb + 511) >> 9)) * 16
        return up(b, 16)


@pytest.fixture(scope="module")
def k(lines):
    return K(lines)


def test_layout_constants_are_consistent(lines, k):
    assert k.wave_tile_bytes == up(6 * k.tile_stride * 2 + 6 * k.z_stride * 2, 16) >= 384 * 4
    assert k.s_count == 26 + 14 + 2 * k.pilot_max + k.max_tiles + 1 + 16          # per-frame scalars, MdecSearch, the pilot's, the tiles', the kept ones
    assert ints(lines["threads"][0]) == [64 * k.waves_small, 64 * k.waves_large] and k.no_mb == 0xFFFF and k.max_tiles == 16
    assert ints(lines["args"][0]) == [1, 1, 0, 0, 0, 0, 0, 0, 1]


def geometry(k, w, h, budget, lds_cu):
    """(fits, large, out_words, stg_words, lds_bytes): the first (shape, tile) that fits, two small groups before one large group,
    the whole image before 2048, 1024, 512 dwords"""
    nmb, image = (w // 16) * (h // 16), (budget + 3) // 4
    sw = image + nmb + 2
    if sw > 0xFFFF:
        return None
    for shape in (0, 1):
        for tile in (image, 2048, 1024, 512):
            t = min(tile, image)
            if -(-image // t) <= 16 and (1 if shape else 2) * k.lds_bytes(nmb, t + 2, sw, shape) <= lds_cu:
                return 1, shape, t + 2, sw, k.lds_bytes(nmb, t + 2, sw, shape)
    ow = min(image, 512) + 2
    return 0, 1, ow, sw, k.lds_bytes(nmb, ow, sw, 1)


def test_geometry_takes_the_first_shape_and_tile_that_fit(lines, k):
    seen, shapes = set(), set()
    for (w, h, budget, lds_cu), got in pairs(lines["geo"]):
        want = geometry(k, w, h, budget, lds_cu)
        if want is None:
            assert got[0] == 0, (w, h, budget, lds_cu)
        else:
            assert got == list(want), (w, h, budget, lds_cu, got, want)
            fits, large, ow, sw, need = want
            assert sw <= 0xFFFF
            if fits:
                assert -(-((budget + 3) // 4) // (ow - 2)) <= 16 and (1 if large else 2) * need <= lds_cu
                shapes.add((large, ow - 2 == (budget + 3) // 4))
        seen.add((w, h, budget, lds_cu))
    assert seen == {(w, h, b, l) for w in SIZES for h in SIZES for b in BUDGETS for l in (65536, 163840)}
    assert shapes == {(0, True), (0, False), (1, True), (1, False)}          # both shapes, whole images and tiles


def test_largest_budget_fits_and_the_next_eight_do_not(lines, k):
    seen = set()
    for (w, h, lds_cu), got in pairs(lines["maxb"]):
        limit, at, above = got[0], got[1], got[2:]
        fits = lambda b: (geometry(k, w, h, b, lds_cu) or (0,))[0]
        if limit:
            assert at == 1 and fits(limit) == 1 and limit >= 8, (w, h, lds_cu)
        else:
            assert fits(8) == 0, (w, h, lds_cu)
        assert above == [0] * 8 and not any(fits(limit + d) for d in range(1, 9)), (w, h, lds_cu, got)
        seen.add((w, h, lds_cu))
    assert len(seen) == 72 and any(g[0] == 0 for _, g in pairs(lines["maxb"])) and any(g[0] > 100000 for _, g in pairs(lines["maxb"]))


def pass_order(lines, w, h, large, cap):
    for line in lines["order"]:
        head, rest = line.split(" : ")
        if ints(head) == [w, h, large, cap]:
            n, words = rest.split(" |")
            return int(n), np.array([int(v, 16) for v in words.split()], np.uint32)
    raise KeyError((w, h, large, cap))


@pytest.mark.parametrize("w,h", [(16, 16), (48, 32), (320, 240), (640, 480)])
@pytest.mark.parametrize("large", [0, 1])
def test_pass_order_visits_every_macroblock_once_and_spreads_the_first_quarter(lines, k, w, h, large):
    """what tests/test_mdec_search.py asserts through the library, on the module itself"""
    waves = k.waves(large)
    nx, ny = w // 16, h // 16
    nmb = nx * ny
    n_want = -(-nmb // waves) * waves
    n, o = pass_order(lines, w, h, large, n_want)
    assert n == n_want and o.size == n
    assert ints([l for l in lines["trips"] if l.startswith("%d %d %d :" % (w, h, large))][0].split(" : ")[1])[0] == n // waves
    valid = o != 0xFFFF
    assert valid.sum() == nmb
    fx, fy = o[valid] & 0xFF, o[valid] >> 8
    assert fx.max() < nx and fy.max() < ny
    assert len(set((fy * nx + fx).tolist())) == nmb
    if n // waves >= 8:
        q = o[:(n // waves // 4) * waves]
        q = q[q != 0xFFFF]
        bands = np.bincount(((q >> 8) * 4 // ny).astype(np.int64), minlength=4)
        rounds = n // waves // 4
        if rounds >= 8:
            assert bands.min() * 3 >= bands.max(), bands
        else:
            assert (bands > 0).sum() >= min(rounds, 3), bands
        rest = o[(n // waves // 4) * waves:]
        first_of_round = rest[::waves]
        first_of_round = first_of_round[first_of_round != 0xFFFF].astype(np.int64)
        raster = (first_of_round >> 8) * nx + (first_of_round & 0xFF)
        assert (np.diff(raster) > 0).all()
    # a cap short of the end: the same entries, and nothing written behind them (the driver's buffer ends there)
    n7, o7 = pass_order(lines, w, h, large, 7)
    assert n7 == n and np.array_equal(o7, o[:7])


def test_pass_table_is_the_order_entry_by_entry(lines, k):
    seen = set()
    for line in lines["table"]:
        head, rest = line.split(" : ")
        w, h, large, cap = ints(head)
        ns, words = rest.split(" |")
        t = np.array([int(v, 16) for v in words.split()], np.uint32).reshape(-1, 2)
        n, o = pass_order(lines, w, h, large, -(-(w // 16) * (h // 16) // k.waves(large)) * k.waves(large))
        assert ints(ns) == [n, n] and t.shape[0] == cap
        ny = h // 16
        want = np.zeros((cap, 2), np.uint32)
        for i in range(min(cap, n)):
            if o[i] != 0xFFFF:
                fx, fy = int(o[i]) & 0xFF, int(o[i]) >> 8
                want[i] = (fy * 8 * w | 0x80000000, fx * 16 | ((fx * ny + fy) * 4 << 16))
        assert np.array_equal(t, want), (w, h, large, cap)          # cap = n + 1: the all-zero entry behind the tickets
        seen.add((w, h, large, cap - n if cap >= n else cap))
    assert seen == {(w, h, l, c) for (w, h) in ((16, 16), (48, 32), (320, 240), (640, 480)) for l in (0, 1) for c in (1, 0, 7)}


def split_geometry(k, codec, w, h, budget, n_frames, n_cu):
    nmb = (w // 16) * (h // 16)
    if nmb <= 0 or n_frames <= 0 or n_cu <= 0:
        return [0] * 10
    M = 2
    while M < 16 and -(-nmb // M) * n_frames > n_cu:
        M *= 2
    segs = -(-nmb // M)
    if segs > n_cu:
        return [0] * 10
    img = (budget + 3) // 4 + 2
    slots = 64
    dcq = slots + k.split_rounds * nmb * k.split_round * 8
    image = dcq + up(nmb * 3 * 4, 16)
    done = image + up(img * 4, 16)
    stride = up(done + up(nmb * 4, 16), 128)
    lds = k.split_lds_bytes(codec, M, nmb)
    return [1 if lds <= 65536 else 0, M, segs, img, stride, slots, dcq, image, done, lds]


def test_split_geometry(lines, k):
    seen, layout = set(), {}
    for (codec, w, h, budget, n_frames, n_cu), got in pairs(lines["split"]):
        want = split_geometry(k, codec, w, h, budget, n_frames, n_cu)
        assert got == want, (codec, w, h, budget, n_frames, n_cu, got, want)
        seen.add((w, h, n_frames, n_cu))
        if got[0]:
            ok, M, segs, img, stride, slots, dcq, image, done, lds = got
            nmb = (w // 16) * (h // 16)
            assert M in (2, 4, 8, 16) and segs <= n_cu and (M == 2 or M == 16 or (segs * n_frames <= n_cu and -(-nmb // (M // 2)) * n_frames > n_cu))
            # the parts: ordered, disjoint, inside the stride; the stride 128-byte aligned
            ends = [slots + k.split_rounds * nmb * k.split_round * 8, dcq + nmb * 3 * 4, image + img * 4, done + nmb * 4]
            assert 64 <= slots and ends[0] <= dcq and ends[1] <= image and ends[2] <= done and ends[3] <= stride
            assert stride % 128 == 0
            # offsets and stride depend on the size and the largest budget only: the context sizes the workspace by the one-frame
            # geometry and uses it for every launch, whatever its number of frames and M
            assert layout.setdefault((w, h, budget), got[3:9]) == got[3:9]
    assert seen >= {(w, h, n, c) for w in SIZES for h in SIZES for n in list(range(1, 13)) + [64] for c in (256, 8, 1)}
    by_m = {}
    for (codec, w, h, budget, n_frames, n_cu), got in pairs(lines["split"]):
        if got[0]:
            by_m.setdefault((w, h, budget), set()).add(got[1])
    assert any(len(v) > 1 for v in by_m.values())          # ... and M did vary under one layout
    assert any(got[0] == 0 and split_geometry(k, *args)[1] == 0 and args[4] > 0 and args[5] > 0 for args, got in pairs(lines["split"]))   # segs > n_cu


def test_split_workspace_parts_are_16_byte_aligned(lines):
    """every part of the workspace starts on a 16-byte boundary.  The done words did not before the plan module existed: they followed
    the image's (budget + 3) // 4 + 2 words directly (8192 bytes: 2050 words = 8200 bytes, ws_done = 8920 at 16x16, 8920 % 16 = 8); the
    image's part is rounded up to 16 bytes now.  The kernel reads and writes the done words one 32-bit word at a time, so either layout
    works; the padding is never written and stays zero."""
    for (codec, w, h, budget, n_frames, n_cu), got in pairs(lines["split"]):
        if got[0]:
            assert all(v % 16 == 0 for v in got[5:9]), (w, h, budget, got[5:9])


def test_the_parents_tables_and_split_geometries_are_reproduced(lines):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "mdec_plan_parent.json")))
    tables = {}
    for line in lines["gtable"]:
        head, rest = line.split(" : ")
        n, words = rest.split(" |")
        tables[tuple(ints(head))] = (int(n), hashlib.sha256(np.array([int(v, 16) for v in words.split()], "<u4").tobytes()).hexdigest())
    assert len(gold["pass_table"]) == 14 and len(gold["split_geometry"]) == 9
    for e in gold["pass_table"]:
        assert tables[(e["width"], e["height"], e["large"])] == (e["n"], e["sha256"]), e
    splits = {tuple(a): g for a, g in pairs(lines["split"])}
    for e in gold["split_geometry"]:
        got = splits[tuple(e["args"])]
        want = list(e["geo"])
        if e["rc"]:
            # The one place where the module departs from that library, on purpose (test_split_workspace_parts_are_16_byte_aligned): the
            # done words start on the next 16-byte boundary behind the image, and the stride follows from that.  What the recorded
            # figures become is worked out here from the recorded figures alone, and compared exactly like the rest.
            nmb = (e["args"][1] // 16) * (e["args"][2] // 16)
            ws_img, img_words, ws_done = want[6], want[2], want[7]
            assert ws_done == ws_img + img_words * 4 and want[3] == up(ws_done + up(nmb * 4, 16), 128)       # (the recorded layout, as it was)
            want[7] = up(ws_done, 16)
            want[3] = up(want[7] + up(nmb * 4, 16), 128)
        assert got[0] == e["rc"] and (not e["rc"] or got[1:] == want), e


def test_launch_policy_at_every_threshold(lines, k):
    seen = set()
    for line in lines["policy"]:
        consts, rest = line.split(" | ")
        call, got = rest.split(" : ")
        codec, w, h, budget, n_cu, groups_max, large, split_max, retry_cap, order_large = ints(consts)
        nb, n, stats, no_split = ints(call)
        geo = split_geometry(k, codec, w, h, budget, n, n_cu)
        if nb == 1 and n <= split_max and not stats and not no_split and geo[0]:
            want = [1, geo[1], geo[2], 0, 0, 0, 0, 0, 0]
        else:
            small = int(bool(order_large) and n <= n_cu)
            shape = int(large or small)
            trips = -(-(w // 16) * (h // 16) // k.waves(shape))
            grid = min(n, groups_max)
            queue = int(retry_cap > 0 and grid < n <= 8 * grid and n < retry_cap)
            want = [0, 0, 0, small, shape, trips, None, grid, queue]
            step = ints(got)[6]
            assert 1 <= step < max(trips, 2) and np.gcd(step, trips) == 1 and abs(step - 0.382 * trips) <= 2, (trips, step)
            want[6] = step
        assert ints(got) == want, line
        seen.add((split_max, retry_cap, large, order_large, nb, n, stats, no_split))
    for split_max, retry_cap, large, order_large, groups_max in ((12, 65536, 0, 0, 512), (12, 65536, 0, 1, 512), (12, 1000, 0, 1, 512), (12, 0, 0, 0, 512),
                                                              (12, 65536, 1, 0, 256), (0, 65536, 0, 1, 512)):
        for t in (split_max, 256, groups_max, 8 * groups_max, retry_cap):
            for n in (t - 1, t, t + 1):
                for nb in (1, 2):
                    if n >= nb:
                        assert {(split_max, retry_cap, large, order_large, nb, n, s, x) for s in (0, 1) for x in (0, 1)} <= seen, (t, n, nb)
    # the rules did decide: each outcome appears
    outcomes = {tuple(ints(l.split(" : ")[1])[i] for i in (0, 3, 4, 8)) for l in lines["policy"]}
    assert {(1, 0, 0, 0), (0, 1, 1, 0), (0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 1)} <= outcomes


def test_host_call_checks_every_refusal_with_its_text(lines):
    want = [
        (0, 8, 8, None), (0, 4096, 4096, None),
        (EINVAL, 0, 0, "encode_frames_host: frame_max_size 7 outside [8, 4096]"),
        (EINVAL, 0, 0, "encode_frames_host: frame_max_size 4097 outside [8, 4096]"),
        (EINVAL, 0, 0, "encode_frames_host: out_stride 1000 smaller than the largest budget 1001"),
        (0, 1001, 1004, None), (0, 4096, 4096, None),
        (EINVAL, 0, 0, "encode_frames_host: frame 1 budget 7 outside [8, 4096]"),
        (EINVAL, 0, 0, "encode_frames_host: frame 2 budget 4097 outside [8, 4096]"),
        (EINVAL, 0, 0, "encode_frames_host: out_stride 776 smaller than the largest budget 777"),
        (0, 777, 780, None), (0, 777, 780, None),
        (EINVAL, 0, 0, "encode_frames_host: row width 776 outside [777, 4096]"),
        (0, 4096, 4096, None),
        (EINVAL, 0, 0, "encode_frames_host: row width 4097 outside [777, 4096]"),
        (EINVAL, 0, 0, "encode_frames_host: out_stride 2047 smaller than the largest budget 2048"),
        (0, 2048, 2048, None),
        (EINVAL, 0, 0, "encode_frames_host: row width 511 outside [512, 4096]"),
    ]
    assert len(lines["check"]) == len(want)
    for line, (rc, max_size, dstride, text) in zip(lines["check"], want):
        head, rest = line.split(" : ")
        got_rc, sizes, got_text = (p.strip() for p in rest.split("|", 2))
        assert int(got_rc) == rc, line
        if rc == 0:
            assert ints(sizes) == [max_size, dstride] and got_text == "", line
            assert dstride == up(max_size, 4)
        else:
            assert got_text == text and ints(sizes) == [-1, 0], line          # (nothing is written for a refused call)


def test_withhold_switch_is_parsed_and_resolved(lines):
    want = {"0:mid": (0, MID, 1, 0), "1:-1:2:1": (1, -1, 2, 1), "2:1000": (2, 1000, 1, 0), "3:4:5": (3, 4, 5, 0), "0:0:1:7": (0, 0, 1, 1),
            "4:mid:3:0": (4, MID, 3, 0)}
    off = ["", "mid", "0", "x:1", "-1:0", "0:1:0", "0:1:-2", "0::1"]          # malformed, or nothing to withhold: reads as off
    got = {}
    for line in lines["withhold"]:
        spec, rest = line.split(" : ")
        got[spec[1:-1]] = tuple(ints(rest))
    assert set(got) == set(want) | set(off)
    for spec, w in want.items():
        assert got[spec] == w, spec
    for spec in off:
        assert got[spec][2] == 0, spec
    seen = set()
    for (seg, segs), (resolved,) in pairs(lines["whseg"]):
        want_seg = segs // 2 if seg == MID else (max(segs + seg, 0) if seg < 0 else min(seg, segs - 1))
        assert resolved == want_seg and 0 <= resolved < segs, (seg, segs)
        seen.add((seg, segs))
    assert {(MID, 7), (-1, 150), (1000, 150), (-1000, 7), (0, 1)} <= seen


def test_chunk_size_at_its_three_bounds(lines):
    bounds = set()
    for (groups_max, frame_bytes, n), (chunk,) in pairs(lines["chunk"]):
        by_grid, by_staging = groups_max * 3 // 4, (96 << 20) // frame_bytes
        want = min(max(min(by_grid, by_staging), 1), n)
        assert chunk == want >= 1, (groups_max, frame_bytes, n)
        bounds.add("frames" if want == n else "one" if want == 1 else "grid" if want == by_grid else "staging")
    assert bounds == {"frames", "one", "grid", "staging"}
