"""Records for tests/cpu/str_demux_lanes.cpp and tests/cpu/strspu_demux_lanes.cpp (one text, tests/cpu/str_readers_lanes.inc) and the
statements' bytes for them: tests/str_demux_ref.py for formats 6, 7 and 9, tests/strspu_demux_ref.py for format 8.

Test infrastructure only."""
import types

import numpy as np

import str_demux_ref as D
import strspu_demux_ref as U

FILL = 0x5C
SETTINGS_WORDS = ("format", "video_codec", "video_width", "video_height", "str_fps_num", "str_fps_den", "str_cd_speed", "str_video_id",
                  "trailing_audio", "audio_channels", "audio_frequency", "audio_bit_depth", "audio_xa_file", "audio_xa_channel", "tail_mode",
                  "strspu_options")


def settings(fmt, **over):
    s = dict(format=fmt, video_codec=0, video_width=48, video_height=32, str_fps_num=15, str_fps_den=1, str_cd_speed=2, str_video_id=0x8001,
             trailing_audio=0, audio_channels=2, audio_frequency=37800, audio_bit_depth=4, audio_xa_file=1, audio_xa_channel=0, tail_mode=0,
             strspu_options=0)
    s.update(over)
    return types.SimpleNamespace(**s)


def sector_size(s):
    return 2048 if s.format == 8 else D.GEOMETRY_OF[s.format][0]


def record(s, streams, first_frame, max_frames, bs_stride, capacity, table=True, in_pad=0, bs_pad=0, out_pad=0, in_offset=0):
    """streams: per stream an (n, sector size) uint8 array, all of one n"""
    streams = [np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, sector_size(s)) for x in streams]
    assert len({x.shape[0] for x in streams}) == 1
    return dict(s=s, streams=streams, first_frame=first_frame, max_frames=max_frames, bs_stride=bs_stride, capacity=capacity, table=table,
                in_pad=in_pad, bs_pad=bs_pad, out_pad=out_pad, in_offset=in_offset)


def write(path, records):
    with open(path, "wb") as f:
        for r in records:
            head = [getattr(r["s"], k) for k in SETTINGS_WORDS]
            head += [len(r["streams"]), r["streams"][0].shape[0], r["first_frame"], r["max_frames"], r["bs_stride"], r["capacity"],
                     int(r["table"]), r["in_pad"], r["bs_pad"], r["out_pad"], FILL, r["in_offset"]]
            head += [0] * (32 - len(head))
            f.write(np.array(head, np.int64).astype(np.uint32).tobytes())
            for x in r["streams"]:
                f.write(x.tobytes())


def _strided(parts, stride):
    """the parts (flat uint8 arrays of one size) `stride` bytes apart in a buffer of FILL that ends with the last part"""
    size = parts[0].size
    buf = np.full((len(parts) - 1) * stride + size, FILL, np.uint8)
    for i, p in enumerate(parts):
        buf[i * stride:i * stride + size] = p
    return buf.tobytes()


def want(r):
    """(the statement's bytes for one record in the program's order, the statement's results per stream)"""
    s, mf, cap = r["s"], r["max_frames"], r["capacity"]
    spu = s.format == 8
    unit = 126 * 16 if spu else sector_size(s)
    results, rows, audio = [], [], []
    for x in r["streams"]:
        bs = np.full((mf, r["bs_stride"]), FILL, np.uint8)
        if spu:
            a = np.full((cap * 126, 16), FILL, np.uint8)
            results.append(U.demux(s, x, r["first_frame"], mf, bs, a))
        else:
            a = np.full((cap, unit), FILL, np.uint8)
            results.append(D.demux(s, x, r["first_frame"], mf, bs, a))
        rows.append(bs.reshape(-1))
        audio.append(a.reshape(-1))
    cat = lambda key: b"".join(np.ascontiguousarray(q[key], dtype=np.int32).tobytes() for q in results)
    parts = []
    if mf:
        parts += [("rows", _strided(rows, mf * r["bs_stride"] + r["bs_pad"])), ("sizes", cat("sizes")), ("info", cat("info"))]
    if cap:
        parts.append(("units" if spu else "xa", _strided(audio, cap * unit + r["out_pad"])))
        if spu:
            parts.append(("chunk_info", cat("chunk_info")))
    if r["table"]:
        parts.append(("table", cat("table")))
    parts.append(("summary", cat("summary")))
    if spu:
        parts.append(("audio_summary", cat("audio_summary")))
    return parts, results


def check(L, folder, exe, records, answers=None):
    """the program's bytes in all three orders against the statements'; returns the statements' results per record"""
    src, dst = str(folder / "in.bin"), str(folder / "out.bin")
    write(src, records)
    raw, at = L.run_orders(exe, src, dst, fibers=True), 0
    out = []
    for k, r in enumerate(records):
        parts, results = want(r) if answers is None else answers[k]
        out.append(results)
        for name, part in parts:
            got = raw[at:at + len(part)]
            if got != part:
                first = next(i for i, (a, b) in enumerate(zip(got, part)) if a != b) if len(got) == len(part) else -1
                raise AssertionError("record %d (format %d, %d x %d sectors): %s differs from the statement first at byte %d" % (
                    k, r["s"].format, len(r["streams"]), r["streams"][0].shape[0], name, first))
            at += len(part)
    assert at == len(raw), (at, len(raw))
    return out
