"""The display back-end's arithmetic of one pixel (psxavenc_amd/csrc/display_core.h) on the CPU, under the host sanitizers, against
the statement (tests/display_ref.py) byte for byte: every format, both chroma modes, dither and mask bit, over the corpus the kernels
are shown (tests/display_corpus.py) at its small sizes and over seeded noise at a few more.  The kernel runs the same text; it sees
the corpus only after this has passed (tests/test_gpu_display.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import display_corpus as K
import display_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpu/display_sim.cpp")
    d = tmp_path_factory.mktemp("display_sim")
    exe = str(d / "display_sim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe,
                    os.path.join(ROOT, "tests/cpu/display_sim.cpp")], check=True)

    def run(records):
        """records: (w, h, frames (n, w h 3 / 2), out_format, options) -> the pictures (n, h, row bytes) of each"""
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        with open(src, "wb") as f:
            for w, h, frames, fmt, options in records:
                f.write(np.array([w, h, frames.shape[0], fmt, options], np.int32).tobytes())
                f.write(np.ascontiguousarray(frames).tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0 and not r.stderr.strip(), "the sanitizer build reported (exit %d):\n%s" % (r.returncode, r.stderr[-4000:])
        raw, out, at = np.fromfile(dst, np.uint8), [], 0
        for w, h, frames, fmt, options in records:
            size = frames.shape[0] * h * R.row_bytes(fmt, w)
            out.append(raw[at:at + size].reshape(frames.shape[0], h, R.row_bytes(fmt, w)))
            at += size
        assert at == raw.size
        return out
    return run


def _differences(got, want):
    bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
    return "%d of %d bytes differ, the first at %d" % (bad.size, got.size, bad[0]) if bad.size else ""


def test_the_corpus_converts_as_the_statement_says(sim):
    sizes = [s for s in K.SIZES if s[0] * s[1] <= 48 * 32]
    records = [(w, h, K.frames(w, h)[0], fmt, options) for w, h in sizes for fmt, options in R.all_option_sets()]
    assert len(records) == 4 * 12
    for (w, h, _, fmt, options), got in zip(records, sim(records)):
        assert not _differences(got, K.expected(w, h, fmt, options)), (w, h, fmt, options, _differences(got, K.expected(w, h, fmt, options)))


def test_seeded_noise_at_more_sizes(sim):
    rng = np.random.default_rng(181)
    records = []
    for w, h in [(64, 16), (16, 64), (80, 48), (1024, 16), (16, 1024)]:
        frames = rng.integers(0, 256, (2, w * h * 3 // 2)).astype(np.uint8)
        records += [(w, h, frames, fmt, options) for fmt, options in R.all_option_sets()]
    for (w, h, frames, fmt, options), got in zip(records, sim(records)):
        want = R.pictures(frames, w, h, fmt, options)
        assert not _differences(got, want), (w, h, fmt, options, _differences(got, want))


def test_the_dither_offsets_are_the_table(sim):
    """grey pictures of one luma value: R = G = B = Y, so the RGB555 picture with dither shows clamp(Y + D) >> 3 cell by cell"""
    w = h = 16
    values = [0, 3, 4, 7, 8, 124, 127, 128, 248, 251, 252, 255]
    frames = np.stack([np.concatenate([np.full(w * h, v, np.uint8), np.full(w * h // 2, 128, np.uint8)]) for v in values])
    got = sim([(w, h, frames, R.OUT_RGB555, R.DITHER)])[0].view("<u2").astype(np.int64)
    cells = R.D[np.arange(h)[:, None] & 3, np.arange(w)[None, :] & 3]
    for i, v in enumerate(values):
        c5 = np.clip(v + cells, 0, 255) >> 3
        assert np.array_equal(got[i], c5 | (c5 << 5) | (c5 << 10)), v


def test_the_noise_of_the_corpus_hits_every_clamp():
    """each of the six clamps of step 2 fires in the statement's answer for the noise frames, at every size and in both chroma modes"""
    for w, h in K.SIZES:
        frames, kinds = K.frames(w, h)
        noise = frames[[k == "noise" for k in kinds]]
        y, cb, cr = R.planes(noise, w, h)
        for bilinear in (False, True):
            v = R.matrix_sums(y, R.chroma_at_pixels(cb, w, h, bilinear), R.chroma_at_pixels(cr, w, h, bilinear)) >> 16
            below, above = (v < 0).reshape(-1, 3).any(axis=0), (v > 255).reshape(-1, 3).any(axis=0)
            assert below.all() and above.all(), (w, h, bilinear, below.tolist(), above.tolist())
