"""The ingest kernel file's own text (psxavenc_amd/csrc/ingest_kernels.hip) on the CPU, lane by lane, under the host sanitizers
(tests/cpu/ingest_lanes.cpp behind the stand-in tests/cpu/hip_lanes/hip/hip_runtime.h), against the statement (tests/ingest_ref.py)
byte for byte.  tests/test_ingest_core_cpu.py runs the arithmetic of one sample; this runs what decides which addresses a lane
touches -- fetch<> and store<>, the clamped neighbours of the bilinear mix, the ragged tail of a workgroup -- over heap blocks of
exactly the sizes the entry point's argument rules accept, where a read outside is a report even when its value is masked away, which
no GPU test can see.  It is shown everything tests/test_gpu_ingest.py shows the kernel, the two remaining matrices, and the wide
sizes of more than one wavefront and workgroup; every lane order -- ascending, descending, shuffled -- must give the same bytes.

The last test measures the coverage of all that: every one of the kernel's instantiations ran, and every line of the file that holds
code, except the lines listed in NOT_REACHED with their reasons."""
import re

import numpy as np
import pytest

import ingest_corpus as K
import ingest_ref as R
import lanes_cpu as L

FILL = 0x5A
KERNEL_FILE = "ingest_kernels.hip"
# lines of ingest_kernels.hip that hold code and that no valid job reaches: {the line's text: why}.  None may lie in fetch, store,
# load_luma, load_chroma, chroma_sample, far_of, chroma_hmix or store_rgb.
NOT_REACHED = {}                # (empty: the records reach every line; a failed launch's `return e` shares its line with the test of e)
ADDRESSING = ("fetch", "store", "load_luma", "load_chroma", "chroma_sample", "far_of", "chroma_hmix", "store_rgb")


def _record(fmt, w, h, planes, size, src, matrix, full, out, options, index=None, out_stride=None):
    return dict(fmt=fmt, w=w, h=h, planes=planes, size=size, src=src, matrix=matrix, full=full, out=out, options=options, index=index,
                out_stride=R.output_bytes(out, w, h) if out_stride is None else out_stride)


def _write(path, records):
    with open(path, "wb") as f:
        for r in records:
            planes = list(r["planes"]) + [(0, 0)] * (3 - len(r["planes"]))
            coef = R.coefficients(r["matrix"], r["full"], R.depth(r["fmt"])) if R.is_yuv(r["fmt"]) else (0,) * 7
            n_out = r["src"].shape[0] if r["index"] is None else len(r["index"])
            head = [r["fmt"], r["w"], r["h"]] + [v for p in planes for v in p] + list(coef) + \
                   [r["out"], r["options"], r["src"].shape[0], r["src"].shape[1], r["size"], n_out, r["out_stride"], int(r["index"] is not None), FILL]
            f.write(np.array(head, np.int32).tobytes())
            if r["index"] is not None:
                f.write(np.asarray(r["index"], np.int32).tobytes())
            f.write(np.ascontiguousarray(r["src"]).tobytes())


def _destination_bytes(r):
    n_out = r["src"].shape[0] if r["index"] is None else len(r["index"])
    return n_out, (n_out - 1) * r["out_stride"] + R.output_bytes(r["out"], r["w"], r["h"])


def _want(r):
    """the destination after the call, by the statement: an entry past the sources leaves its picture as a negative one does"""
    n_out, size = _destination_bytes(r)
    index = None if r["index"] is None else [i if i < r["src"].shape[0] else -1 for i in r["index"]]
    before = np.full((n_out, r["out_stride"]), FILL, np.uint8)
    return R.convert(r["src"], r["fmt"], r["w"], r["h"], r["planes"], r["matrix"], r["full"], r["out"], r["options"], index=index,
                     out=before).reshape(-1)[:size]


# ---------------------------------------------------------------------------------------------------------------- the records
def matrix_records(fmt, sizes_for=K.sizes_for, seed=7):
    """tests/test_gpu_ingest.py::test_every_setting_over_the_corpus"""
    unit, out = 2 if fmt in R.TEN_BIT else 1, []
    for out_format in (R.OUT_RGB24, R.OUT_YUV420P):
        settings = [s for s in K.settings_for(fmt) if s[2] == out_format]
        for w, h in sizes_for(fmt, out_format) if settings else []:
            planes, size = R.layout(fmt, w, h)
            src, _ = K.pictures(fmt, w, h, planes, size + 3 * unit, seed=seed)
            out += [_record(fmt, w, h, planes, size, src, m, full, o, opt) for m, full, o, opt in settings]
    return out


def wide_records(fmt):
    """tests/test_gpu_ingest.py::test_every_setting_at_sizes_of_several_wavefronts_and_workgroups"""
    return matrix_records(fmt, K.wide_sizes_for, seed=23)


def placement_records(fmt):
    """tests/test_gpu_ingest.py::test_padded_pitches_shifted_planes_and_untouched_bytes"""
    unit, out = 2 if fmt in R.TEN_BIT else 1, []
    for out_format in (R.OUT_RGB24, R.OUT_YUV420P):
        if out_format == R.OUT_YUV420P and not R.is_yuv(fmt):
            continue
        for w, h in [(18, 4), (16, 4)]:
            for pad in K.PADS:
                for first in K.OFFSETS:
                    planes, size = R.layout(fmt, w, h, pad * unit, first * unit, gap=(first ^ 1) * unit)
                    src, _ = K.pictures(fmt, w, h, planes, size + (5 + first) * unit, seed=11)
                    opt = R.CHROMA_BILINEAR if (first & 1 and out_format == R.OUT_RGB24) else 0
                    out.append(_record(fmt, w, h, planes, size, src, R.BT601, bool(first & 2), out_format, opt,
                                       out_stride=R.output_bytes(out_format, w, h) + 13 - first))
    return out


def selection_records():
    """tests/test_gpu_ingest.py::test_pictures_are_selected_by_index"""
    out = []
    for fmt, out_format, w, h in [(R.NV12, R.OUT_RGB24, 18, 6), (R.YUV422P10, R.OUT_YUV420P, 34, 6), (R.BGRA32, R.OUT_RGB24, 5, 7), (R.UYVY422, R.OUT_YUV420P, 16, 4)]:
        planes, size = R.layout(fmt, w, h, pad=2)
        src, _ = K.pictures(fmt, w, h, planes, size + 6, seed=13)
        m = R.BT709 if out_format == R.OUT_RGB24 else R.BT601
        for index, spare in (([3, 3, -1, 2, 0, 0, -5, 3, 4], 8), ([3, 2, 1, 0], 0)):
            out.append(_record(fmt, w, h, planes, size, src, m, False, out_format, 0, index=index, out_stride=R.output_bytes(out_format, w, h) + spare))
    return out


def cut_records():
    """tests/test_gpu_ingest.py::test_more_outputs_than_a_grid_dimension_holds: 65 537 outputs of 2 x 2, by an index and without"""
    fmt, w, h, n = R.NV21, 2, 2, 65537
    planes, size = R.layout(fmt, w, h)
    src, _ = K.pictures(fmt, w, h, planes, size + 2, seed=17)
    src = src[:3]
    index = (np.arange(n) * 7 + np.arange(n) // 65535) % 4 - 1
    index[-2:] = [2, 0]
    return [_record(fmt, w, h, planes, size, src, R.BT601, True, R.OUT_RGB24, 0, index=index.tolist(), out_stride=16),
            _record(fmt, w, h, planes, size, np.tile(src, (21846, 1))[:n], R.BT601, True, R.OUT_RGB24, 0)]


def other_matrix_records():
    """the two matrices of the five that the corpus leaves out, in both ranges and both chroma modes, for an 8-bit and a 10-bit format"""
    out = []
    for fmt in (R.NV12, R.YUV422P10):
        w, h = 34, 6
        planes, size = R.layout(fmt, w, h)
        src, _ = K.pictures(fmt, w, h, planes, size, seed=29)
        out += [_record(fmt, w, h, planes, size, src, m, full, R.OUT_RGB24, opt) for m in (R.SMPTE240M, R.FCC) for full in (False, True)
                for opt in (0, R.CHROMA_BILINEAR)]
    return out


# ---------------------------------------------------------------------------------------------------------------- the programs
@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    d = tmp_path_factory.mktemp("ingest_lanes")
    exe = L.build(d, "ingest_lanes", L.SANITIZE)

    def check(records):
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        _write(src, records)
        raw, at = np.frombuffer(L.run_orders(exe, src, dst), np.uint8), 0
        for r in records:
            size = _destination_bytes(r)[1]
            got, want = raw[at:at + size], _want(r)
            at += size
            bad = np.nonzero(got != want)[0]
            assert not bad.size, (R.NAMES[r["fmt"]], r["w"], r["h"], r["matrix"], r["full"], r["out"], r["options"], r["planes"],
                                  "%d bytes differ from the statement, the first at %d" % (bad.size, bad[0]))
        assert at == raw.size
    return check


@pytest.mark.parametrize("fmt", R.ALL_FORMATS, ids=R.NAMES)
def test_every_setting_over_the_corpus(lanes, fmt):
    lanes(matrix_records(fmt))


@pytest.mark.parametrize("fmt", R.ALL_FORMATS, ids=R.NAMES)
def test_every_setting_at_sizes_of_several_wavefronts_and_workgroups(lanes, fmt):
    records = wide_records(fmt)
    assert max(K.lanes_of(r["w"], r["h"]) for r in records) > 256
    lanes(records)


@pytest.mark.parametrize("fmt", R.ALL_FORMATS, ids=R.NAMES)
def test_padded_pitches_shifted_planes_and_untouched_bytes(lanes, fmt):
    lanes(placement_records(fmt))


def test_pictures_are_selected_by_index(lanes):
    lanes(selection_records())


def test_more_outputs_than_a_grid_dimension_holds(lanes):
    lanes(cut_records())


def test_the_two_remaining_matrices(lanes):
    lanes(other_matrix_records())


def test_the_wide_sizes_are_what_the_corpus_says():
    assert [K.lanes_of(w, h) for w, h in K.WIDE_SIZES] == [85, 192, 330, 257, 195]
    assert max(K.lanes_of(w, h) for w, h in K.EVEN_SIZES + K.ODD_SIZES + K.WHOLE_SIZES) == 48


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_the_records_reach_every_instantiation_and_every_line(tmp_path):
    exe = L.build(tmp_path, "ingest_lanes", L.COVERAGE)
    records = selection_records() + cut_records() + other_matrix_records()
    for fmt in R.ALL_FORMATS:
        records += matrix_records(fmt) + wide_records(fmt) + placement_records(fmt)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write(src, records)
    L.run(exe, src, dst, sanitized=False)
    cov = L.Coverage(tmp_path, "ingest_lanes", KERNEL_FILE)
    # (a) the file's own statement of how many instantiations the kernel has
    stated = [int(n) for n in re.findall(r"(\d+) instantiations", "\n".join(cov.text))]
    seen = cov.instantiations("ingest_convert_kernel")
    print("instantiations of ingest_convert_kernel: %d seen, %s stated by the file" % (len(seen), stated))
    assert stated == [29] and len(seen) == 29
    assert not [n for n, c in seen.items() if c == 0], [n for n, c in seen.items() if c == 0]
    # (b) every line that holds code ran, except the listed ones
    unvisited = cov.unvisited()
    print("lines that hold code and did not run:", unvisited)
    assert not [x for x in unvisited if x[1] not in NOT_REACHED], [x for x in unvisited if x[1] not in NOT_REACHED]
    # (c) none of the listed lines lies in the functions that decide an address
    inside = cov.lines_of(ADDRESSING)
    assert len(inside) > 60
    listed = [n for n, text in enumerate(cov.text, 1) if text.strip() in NOT_REACHED]
    assert not [n for n in listed if n in inside], [n for n in listed if n in inside]
