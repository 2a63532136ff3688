"""The picture ingest's arithmetic of one sample (psxavenc_amd/csrc/ingest_core.h: ingest_pixel()) on the CPU, under the host
sanitizers, against the statement (tests/ingest_ref.py) byte for byte: every format, both outputs, both chroma modes, three
matrices, both ranges, over the corpus the kernels are shown (tests/ingest_corpus.py) -- padded pitches and shifted planes
included.  The kernel calls the same functions; it sees the corpus only after this has passed (tests/test_gpu_ingest.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ingest_corpus as K
import ingest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpu/ingest_sim.cpp")
    d = tmp_path_factory.mktemp("ingest_sim")
    exe = str(d / "ingest_sim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe,
                    os.path.join(ROOT, "tests/cpu/ingest_sim.cpp")], check=True)

    def run(records):
        """records: dicts of fmt, w, h, planes, size, matrix, full, out, options, src (n, stride) -> the output pictures of each"""
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        with open(src, "wb") as f:
            for r in records:
                planes = list(r["planes"]) + [(0, 0)] * (3 - len(r["planes"]))
                coef = R.coefficients(r["matrix"], r["full"], R.depth(r["fmt"])) if R.is_yuv(r["fmt"]) else (0,) * 7
                head = [r["fmt"], r["w"], r["h"]] + [v for p in planes for v in p] + list(coef) + \
                       [r["out"], r["options"], r["src"].shape[0], r["src"].shape[1], r["size"]]
                f.write(np.array(head, np.int32).tobytes())
                f.write(np.ascontiguousarray(r["src"]).tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=900)
        assert p.returncode == 0 and not p.stderr.strip(), "the sanitizer build reported (exit %d):\n%s" % (p.returncode, p.stderr[-4000:])
        raw, out, at = np.fromfile(dst, np.uint8), [], 0
        for r in records:
            n, size = r["src"].shape[0], R.output_bytes(r["out"], r["w"], r["h"])
            out.append(raw[at:at + n * size].reshape(n, size))
            at += n * size
        assert at == raw.size
        return out
    return run


def _record(fmt, w, h, matrix, full, out, options, pad=0, first=0, gap=0, seed=5):
    unit = 2 if fmt in R.TEN_BIT else 1
    planes, size = R.layout(fmt, w, h, pad * unit, first * unit, gap * unit)
    src, _ = K.pictures(fmt, w, h, planes, size + 2 * unit, seed)
    return dict(fmt=fmt, w=w, h=h, planes=planes, size=size, matrix=matrix, full=full, out=out, options=options, src=src)


def _check(sim, records):
    for r, got in zip(records, sim(records)):
        want = R.convert(r["src"], r["fmt"], r["w"], r["h"], r["planes"], r["matrix"], r["full"], r["out"], r["options"])
        bad = np.nonzero(got != want)
        assert not bad[0].size, (R.NAMES[r["fmt"]], r["w"], r["h"], r["matrix"], r["full"], r["out"], r["options"], r["planes"],
                                 "%d bytes differ, the first in picture %d at %d" % (bad[0].size, bad[0][0], bad[1][0]))


@pytest.mark.parametrize("fmt", R.ALL_FORMATS, ids=R.NAMES)
def test_every_setting_converts_as_the_statement_says(sim, fmt):
    sizes = {R.OUT_RGB24: [(2, 2), (6, 4), (18, 2), (16, 4), (1, 1), (3, 3), (5, 7), (33, 1)], R.OUT_YUV420P: [(2, 2), (6, 4), (18, 2), (16, 4)]}
    records = [_record(fmt, w, h, m, full, out, opt) for m, full, out, opt in K.settings_for(fmt) for w, h in sizes[out]
               if not (fmt in R.PACKED and w % 2)]
    assert len(records) >= 8
    _check(sim, records)


@pytest.mark.parametrize("fmt", R.ALL_FORMATS, ids=R.NAMES)
def test_padded_pitches_and_shifted_planes(sim, fmt):
    records = []
    for out in (R.OUT_RGB24, R.OUT_YUV420P):
        if out == R.OUT_YUV420P and not R.is_yuv(fmt):
            continue
        for pad in K.PADS:
            for first in K.OFFSETS:
                records.append(_record(fmt, 18, 4, R.BT601, False, out, R.CHROMA_BILINEAR if first & 1 else 0, pad, first, gap=first ^ 1))
    _check(sim, records)


def test_the_noise_of_the_corpus_hits_every_clamp():
    """each of the six clamps of the matrix fires in the statement's answer for the noise pictures, in both chroma modes"""
    for fmt in (R.NV12, R.YUV422P10):
        w, h = 66, 10
        planes, size = R.layout(fmt, w, h)
        src, _ = K.pictures(fmt, w, h, planes, size, 5)
        for bilinear in (False, True):
            below, above = np.zeros(3, bool), np.zeros(3, bool)
            for pic in src[:2]:
                y, cb, cr = R.unpack(pic, fmt, w, h, planes)
                v = R.matrix_sums(y, R.chroma_at_pixels(cb, fmt, w, h, bilinear), R.chroma_at_pixels(cr, fmt, w, h, bilinear),
                                  R.coefficients(R.BT709, False, R.depth(fmt))) >> 16
                below |= (v < 0).reshape(-1, 3).any(axis=0)
                above |= (v > 255).reshape(-1, 3).any(axis=0)
            assert below.all() and above.all(), (fmt, bilinear, below.tolist(), above.tolist())
