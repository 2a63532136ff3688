"""The MDEC decoder's kernel file (psxavenc_amd/csrc/mdec_decode_kernels.hip) and its host layer (psxhip_decode.cpp), their own text,
on the CPU under the host sanitizers: tests/cpu/mdec_decode_lanes.cpp behind the stand-in's wavefront model
(tests/cpu/hip_lanes/hip_lanes_waves.h), against the oracle's reader (tests/mdec_decode_corpus.py: status, levels, quant scale,
version, bits consumed), "psxhip MDEC reconstruct v1" (tests/mdec_recon_ref.py) and numpy sums of squared errors.

The parse core (mdec_parse.h) already runs on the CPU; what runs here for the first time is what stands round it: the staging of
the tables in LDS, the clamp of a frame's size to bs_stride, the header loads, the readlane walk over a window, the stores of
blocks, the reconstruct kernel's early returns in front of 96 shuffles, the SSE kernel's reduction.  The bitstream block of a device
call ends with the last byte of the frame's size, so a read past a frame's size -- which on the device finds the next row, or
guard bytes that merely change a status -- is a report.  Three orders of workgroups, wavefronts and lanes must give equal bytes.
The last test reads gcov: every line of the kernel file ran."""
import numpy as np
import pytest

import lanes_cpu as L
import mdec_decode_corpus as DC
import mdec_recon_ref as R
import oracle_lib as O

FILL = 0x3D
KERNEL_FILE = "mdec_decode_kernels.hip"
NOT_REACHED = {}


def decode_record(kind, w, h, wrap, rows, sizes=None, uniform=0, levels=True, frames=True, frame_pad=0):
    """rows: (n, bs_stride) uint8; sizes: per frame, or None for `uniform`"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n, stride = rows.shape
    head = np.array([kind, w, h, int(wrap), n, stride, int(sizes is not None), uniform, int(levels), int(frames), frame_pad, FILL, 0, 0, 0, 0], np.int32)
    src = head.tobytes() + (np.asarray(sizes, np.int32).tobytes() if sizes is not None else b"") + rows.tobytes()
    eff = [min(max(int(s), 0), stride) for s in (sizes if sizes is not None else [uniform] * n)]
    return dict(kind=kind, w=w, h=h, wrap=wrap, rows=rows, eff=eff, levels=levels, frames=frames, frame_pad=frame_pad, src=src)


def check_decode(r, raw, at, where):
    """one decode record's output against the oracle and the reconstruction's statement; returns the next offset and the statuses"""
    w, h, n = r["w"], r["h"], len(r["eff"])
    nblk, fb = (w // 16) * (h // 16) * 6, w * h * 3 // 2
    dec = np.frombuffer(raw, np.int32, 4 * n, at).reshape(n, 4)
    at += 16 * n
    lv = px = None
    if r["levels"]:
        lv = np.frombuffer(raw, np.int16, n * nblk * 64, at).reshape(n, nblk, 64)
        at += n * nblk * 128
    if r["frames"]:
        stride = fb + (r["frame_pad"] if r["kind"] == 0 else 0)
        size = (n - 1) * stride + fb
        flat = np.frombuffer(raw, np.uint8, size, at)
        at += size
        px = [flat[i * stride:i * stride + fb] for i in range(n)]
        for i in range(n - 1):
            assert (flat[i * stride + fb:(i + 1) * stride] == FILL).all(), (where, i, "bytes between the frames changed")
    statuses = []
    for i in range(n):
        rc, want, q, v, nbits = DC.oracle_decode(DC.Case("", w, h, r["wrap"], r["rows"][i], r["eff"][i]))
        statuses.append(int(rc))
        assert dec[i, 0] == rc, (where, i, dec[i].tolist(), rc)
        if rc == 0:
            assert tuple(dec[i]) == (0, q, v, nbits), (where, i, dec[i].tolist(), (q, v, nbits))
            if lv is not None:
                assert np.array_equal(lv[i], want), (where, i, "levels")
            if px is not None:
                assert np.array_equal(px[i], R.reconstruct(w, h, want, q).reshape(-1)), (where, i, "pixels")
        else:
            assert dec[i, 3] == 0, (where, i)
            if px is not None:
                assert (px[i] == FILL).all(), (where, i, "a frame that does not parse leaves its pixels alone")
    return at, statuses


def sse_record(w, h, a, b, pad):
    n, fb = a.shape[0], w * h * 3 // 2
    head = np.array([2, w, h, 0, n, fb + pad, 0, 0, 0, 0, 0, FILL, 0, 0, 0, 0], np.int32)
    return dict(kind=2, src=head.tobytes() + a.tobytes() + b.tobytes(), want=R.sse(w, h, a, b).astype(np.uint64).tobytes())


# ---- the corpus
def _clean(codec, w, h, n, budget, amp=8):
    fr = O.synth_frames(w, h, n, seed=60 + codec, amp=amp, first=1)
    rows, res, rc = O.mdec_encode(codec, w, h, fr, budget)
    assert rc == 0 and (res[:, 0] <= 63).all()
    return rows[:, :budget], np.minimum(res[:, 1], budget).astype(np.int32)


def shape_records():
    """16x16 and 48x32, v2 (codec 0), v3 (1) and v3 with the DC wrap (2); per-frame sizes and a uniform size; sizes of 0, 7, 8, one
    byte short of the frame's last code and above bs_stride; levels only, pixels only (through the context's workspace) and neither;
    both entry points, the host one with a row stride that is no multiple of 4; a failed frame between two good ones; a quant scale
    past the reconstruction's saturation bound"""
    out = []
    for codec in (0, 1, 2):
        for (w, h, budget) in ((16, 16, 1024), (48, 32, 2048)):
            rows, used = _clean(codec, w, h, 3, budget)
            wrap = codec == 2
            out.append(decode_record(0, w, h, wrap, rows, used, frame_pad=8))
            out.append(decode_record(0, w, h, wrap, rows, None, budget, levels=False))
            out.append(decode_record(0, w, h, wrap, rows, None, budget, frames=False))
            out.append(decode_record(0, w, h, wrap, rows, used, levels=False, frames=False))
            wide = np.full((3, budget + 1), 0xEE, np.uint8)
            wide[:, :budget] = rows
            out.append(decode_record(1, w, h, wrap, wide, used))
            out.append(decode_record(1, w, h, wrap, rows, None, budget, levels=False, frames=False))
            u = int(used[0])
            for size in (0, 7, 8, u - 1, u - 4, budget + 100):
                out.append(decode_record(0, w, h, wrap, rows[:1], [size]))
            # a size above bs_stride on a row that ends in the middle of the frame's codes: the parser comes to the row's last byte
            # and asks for more, and only the clamp of the size to bs_stride keeps it inside the block
            short = (u - 8) & ~3
            out.append(decode_record(0, w, h, wrap, rows[:1, :short], [short + 100]))
            out.append(decode_record(0, w, h, wrap, rows[:1, :short], [0x7FFFFFFF], levels=False))
            bad = rows.copy()
            bad[1, 3] = 0x39                                       # wrong magic: the middle frame fails
            out.append(decode_record(0, w, h, wrap, bad, [int(used[0]), int(used[1]), int(used[2])], frame_pad=4))
            big = rows[:1].copy()
            big[0, 4], big[0, 5] = 0x05, 0x40                      # quant scale 0x4005 > 2^14
            out.append(decode_record(0, w, h, wrap, big, [u]))
    return out


def _thinned(cases, keep=2):
    """of every class of the corrupted corpus (a case's name without its running number) `keep` cases, evenly spaced, of every
    truncation series eight; every class stays, a run of the program stays short"""
    groups = {}
    for c in cases:
        groups.setdefault(c.name.rstrip("0123456789"), []).append(c)
    out = []
    for name, g in groups.items():
        k = 8 if name.endswith("cut at ") else keep
        at = sorted({int(round(i * (len(g) - 1) / max(k - 1, 1))) for i in range(min(k, len(g)))})
        out += [g[i] for i in at]
    return out


def corrupted_records():
    """the corrupted corpus, thinned, one frame to a call, so that each frame's bitstream block ends with its own size (the row stride
    is the size rounded up to 4; the program's block does not hold the bytes behind the size)"""
    out = []
    for k, c in enumerate(_thinned(DC.corrupted_cases())):
        row = np.full((1, max((c.size + 3) & ~3, 4)), 0xEE, np.uint8)
        row[0, :c.size] = c.data[:c.size]
        out.append(decode_record(0, c.w, c.h, c.wrap, row, [c.size], levels=k % 2 == 0, frames=k % 3 != 1))
    return out


def sse_records():
    """16x16 (96 dwords) and 48x32 (576): neither a multiple of the workgroup's 256; extremes and noise; a padded stride"""
    out = []
    for (w, h, n) in ((16, 16, 3), (48, 32, 2)):
        fb = w * h * 3 // 2
        rng = np.random.default_rng(w)
        out.append(sse_record(w, h, np.zeros((n, fb), np.uint8), np.full((n, fb), 255, np.uint8), 36))
        out.append(sse_record(w, h, rng.integers(0, 256, (n, fb), dtype=np.uint8), rng.integers(0, 256, (n, fb), dtype=np.uint8), 0))
    return out


def _run(folder, exe, records):
    src, dst = str(folder / "in.bin"), str(folder / "out.bin")
    with open(src, "wb") as f:
        for r in records:
            f.write(r["src"])
    raw, at, seen = L.run_orders(exe, src, dst, fibers=True), 0, []
    for k, r in enumerate(records):
        if r["kind"] == 2:
            assert raw[at:at + len(r["want"])] == r["want"], ("record %d" % k, "sums of squared errors")
            at += len(r["want"])
        else:
            at, statuses = check_decode(r, raw, at, "record %d" % k)
            seen += statuses
    assert at == len(raw), (at, len(raw))
    return seen


@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    d = tmp_path_factory.mktemp("mdec_decode_lanes")
    return d, L.build(d, "mdec_decode_lanes", L.SANITIZE)


def test_shapes_sizes_outputs_and_entry_points(oracle, lanes):
    seen = _run(*lanes, shape_records())
    assert 0 in seen and any(s != 0 for s in seen)


def test_corrupted_corpus_one_frame_to_a_block(oracle, lanes):
    seen = _run(*lanes, corrupted_records())
    assert set(seen) == DC.REACHABLE[2] | DC.REACHABLE[3]


def test_sse_kernel_is_exact(oracle, lanes):
    _run(*lanes, sse_records())


def test_the_records_reach_every_line(oracle, tmp_path):
    exe = L.build(tmp_path, "mdec_decode_lanes", L.COVERAGE)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        for r in shape_records() + corrupted_records()[::3] + sse_records():
            f.write(r["src"])
    L.run(exe, src, dst, sanitized=False)
    cov = L.Coverage(tmp_path, "mdec_decode_lanes", KERNEL_FILE)
    unvisited = cov.unvisited()
    print("lines that hold code and did not run:", unvisited)
    assert not [x for x in unvisited if x[1] not in NOT_REACHED], [x for x in unvisited if x[1] not in NOT_REACHED]
    assert len(cov.lines) > 80
