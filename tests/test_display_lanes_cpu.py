"""The display kernel file's own text (psxavenc_amd/csrc/display_kernels.hip) on the CPU, lane by lane, under the host sanitizers
(tests/cpu/display_lanes.cpp behind the stand-in tests/cpu/hip_lanes/hip/hip_runtime.h), against the statement
(tests/display_ref.py) byte for byte.  tests/test_display_core_cpu.py runs the arithmetic of one pixel; this runs what decides which
addresses a lane touches -- chroma_hmix's dwords left and right of the lane's own, the rows above and below, the last workgroup's
tail -- over heap blocks of exactly the sizes psxhip_display_check accepts, where a read outside is a report even when its value is
dropped.  Every option set over the corpus, the placement cases and the gate of tests/test_gpu_display.py; every lane order --
ascending, descending, shuffled -- must give the same bytes.

The last test measures the coverage of all that: every one of the kernel's instantiations ran, and every line of the file that holds
code, except the lines listed in NOT_REACHED with their reasons."""
import re

import numpy as np
import pytest

import display_corpus as K
import display_ref as R
import lanes_cpu as L

FILL = 0xA5
KERNEL_FILE = "display_kernels.hip"
# lines of display_kernels.hip that hold code and that no valid job reaches: {the line's text: why}.  None may lie in chroma_hmix
# (or in a function of the names the ingest kernel's list bars).
NOT_REACHED = {}                # (empty: the records reach every line)
ADDRESSING = ("fetch", "store", "load_luma", "load_chroma", "chroma_sample", "far_of", "chroma_hmix", "store_rgb")


def _record(w, h, frames, fmt, options, frame_stride=None, pitch=None, stride=None, offset=0, statuses=None):
    row = R.row_bytes(fmt, w)
    pitch = row if pitch is None else pitch
    return dict(w=w, h=h, frames=frames, fmt=fmt, options=options, frame_stride=frames.shape[1] if frame_stride is None else frame_stride,
                pitch=pitch, stride=(h - 1) * pitch + row if stride is None else stride, offset=offset, statuses=statuses)


def _destination_bytes(r):
    return (r["frames"].shape[0] - 1) * r["stride"] + (r["h"] - 1) * r["pitch"] + R.row_bytes(r["fmt"], r["w"])


def _write(path, records):
    with open(path, "wb") as f:
        for r in records:
            n = r["frames"].shape[0]
            assert r["frames"].shape[1] == r["frame_stride"]
            f.write(np.array([r["w"], r["h"], n, r["fmt"], r["options"], r["frame_stride"], r["pitch"], r["stride"], r["offset"],
                              int(r["statuses"] is not None), FILL], np.int32).tobytes())
            if r["statuses"] is not None:
                decoded = np.zeros((n, 4), np.int32)
                decoded[:, 0], decoded[:, 1], decoded[:, 2] = r["statuses"], 7, 2
                f.write(decoded.tobytes())
            f.write(np.ascontiguousarray(r["frames"]).tobytes())


def _want(r, pics=None):
    pics = R.pictures(r["frames"], r["w"], r["h"], r["fmt"], r["options"]) if pics is None else pics
    return R.place(np.full(_destination_bytes(r), FILL, np.uint8), pics, r["pitch"], r["stride"], 0, r["statuses"])


# ---------------------------------------------------------------------------------------------------------------- the records
def corpus_records(w, h):
    """tests/test_gpu_display.py::test_formats_and_options_over_the_corpus: every option set, the frames of a size in one call"""
    return [_record(w, h, K.frames(w, h)[0], fmt, options) for fmt, options in R.all_option_sets()]


def noise_records():
    """the widest and the tallest picture there is, and one row of lanes that is exactly a wavefront"""
    rng, out = np.random.default_rng(181), []
    for w, h in [(256, 16), (1024, 16), (16, 1024)]:
        frames = rng.integers(0, 256, (2, w * h * 3 // 2)).astype(np.uint8)
        out += [_record(w, h, frames, fmt, options) for fmt, options in R.all_option_sets()]
    return out


def placement_records():
    """tests/test_gpu_display.py::test_placement_inside_a_larger_surface"""
    w, h, n, out = 48, 32, 3, []
    fb = w * h * 3 // 2
    for fmt in R.FORMATS:
        row = R.row_bytes(fmt, w)
        padded = np.random.default_rng(40 + fmt).integers(0, 256, (n, fb + 64)).astype(np.uint8)
        extras = (R.DITHER | R.MASK_BIT) if fmt == R.OUT_RGB555 else 0
        for options in (extras, extras | R.CHROMA_BILINEAR):
            for pitch in (row + 4, row + 68):
                for offset in (4, 8, 12):
                    out.append(_record(w, h, padded, fmt, options, pitch=pitch, stride=(h - 1) * pitch + row + 256, offset=offset))
    return out


def gate_records():
    """tests/test_gpu_display.py::test_frames_the_decoder_gave_up_are_skipped"""
    w, h = 32, 16
    frames = np.random.default_rng(50).integers(0, 256, (5, w * h * 3 // 2)).astype(np.uint8)
    return [_record(w, h, frames, fmt, options, statuses=[0, -5, 0, -1, 0]) for fmt, options in R.all_option_sets()]


# ---------------------------------------------------------------------------------------------------------------- the programs
@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    d = tmp_path_factory.mktemp("display_lanes")
    exe = L.build(d, "display_lanes", L.SANITIZE)

    def check(records, wants=None):
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        _write(src, records)
        raw, at = np.frombuffer(L.run_orders(exe, src, dst), np.uint8), 0
        for i, r in enumerate(records):
            size = _destination_bytes(r)
            got, want = raw[at:at + size], _want(r, None if wants is None else wants[i])
            at += size
            bad = np.nonzero(got != want)[0]
            assert not bad.size, (r["w"], r["h"], r["fmt"], r["options"], r["pitch"], r["stride"], r["offset"],
                                  "%d bytes differ from the statement, the first at %d" % (bad.size, bad[0]))
        assert at == raw.size
        return raw
    return check


@pytest.mark.parametrize("w,h", K.SIZES)
def test_formats_and_options_over_the_corpus(lanes, w, h):
    lanes(corpus_records(w, h), [K.expected(w, h, fmt, options) for fmt, options in R.all_option_sets()])


def test_noise_at_the_widest_and_the_tallest_size(lanes):
    lanes(noise_records())


def test_placement_inside_a_larger_surface(lanes):
    lanes(placement_records())


def test_frames_the_decoder_gave_up_are_skipped(lanes):
    records = gate_records()
    raw = lanes(records)
    size = _destination_bytes(records[0])                    # RGB24: pictures 1 and 3 keep the fill
    picture = size // 5
    assert (raw[picture:2 * picture] == FILL).all() and (raw[3 * picture:4 * picture] == FILL).all() and not (raw[:picture] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_the_records_reach_every_instantiation_and_every_line(tmp_path):
    exe = L.build(tmp_path, "display_lanes", L.COVERAGE)
    records = noise_records() + placement_records() + gate_records()
    for w, h in K.SIZES:
        records += corpus_records(w, h)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write(src, records)
    L.run(exe, src, dst, sanitized=False)
    cov = L.Coverage(tmp_path, "display_lanes", KERNEL_FILE)
    # (a) the file's own statement of how many instantiations the kernel has: psxhip_display_launch names six (format, dither, mask
    #     bit) triples, and launch_chroma makes two of each; the specification's option sets are as many
    text = "\n".join(cov.text)
    stated = len(re.findall(r"\blaunch_chroma<DISP_\w+, (?:true|false), (?:true|false)>\(", text)) * len(re.findall(r"\blaunch<FMT, (?:true|false), DITHER, MASK>\(", text))
    seen = cov.instantiations("display_convert_kernel")
    print("instantiations of display_convert_kernel: %d seen, %d stated by the file" % (len(seen), stated))
    assert stated == 12 == len(R.all_option_sets()) and len(seen) == 12
    assert not [n for n, c in seen.items() if c == 0], [n for n, c in seen.items() if c == 0]
    # (b) every line that holds code ran, except the listed ones
    unvisited = cov.unvisited()
    print("lines that hold code and did not run:", unvisited)
    assert not [x for x in unvisited if x[1] not in NOT_REACHED], [x for x in unvisited if x[1] not in NOT_REACHED]
    # (c) none of the listed lines lies in the functions that decide an address
    inside = cov.lines_of(ADDRESSING)
    assert len(inside) >= 10
    listed = [n for n, line in enumerate(cov.text, 1) if line.strip() in NOT_REACHED]
    assert not [n for n in listed if n in inside], [n for n in listed if n in inside]
