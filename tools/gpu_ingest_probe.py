#!/usr/bin/env python3
"""Times the picture ingest (psxavenc_amd/ingest.py) on 64 pictures of 1920x1080 -- NV12 -> YUV420P, NV12 BT.709 -> RGB24, P010
BT.709 -> RGB24 with bilinear chroma, YUV422P10 -> YUV420P -- each beside a device-to-device copy_ that moves the same number of
bytes (read plus written).

  python tools/gpu_ingest_probe.py --out profiles/<kernel rev>_probe.json

Device events around windows of back-to-back launches, every leg warmed up first, the legs alternated inside one run, median and
spread over the windows reported.  Bytes moved are what the algorithm needs, computed from the shapes: the source's sample bytes
read once, the packed output written once (bilinear chroma reads the same bytes: its neighbours come out of cache lines the kernel
fetches anyway).  Every leg has `--sets` sets of buffers and takes the next one with each launch, so that a launch finds neither its
input nor its output in the 256 MB last-level cache: a batch is 300 .. 800 MB, and the sets of a leg together are a multiple of
that.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--pictures", type=int, default=64)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=200.0, help="target length of a timed window")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "gpu_ingest_probe needs an MI355X"
    from psxavenc_amd import ingest as I

    w, h, n = args.width, args.height, args.pictures
    assert w % 2 == 0 and h % 2 == 0

    def tight(rows_and_bytes):
        planes, at = [], 0
        for rows, row in rows_and_bytes:
            planes.append((at, row))
            at += rows * row
        return planes, at

    variants = [
        ("NV12 -> YUV420P", I.SRC_NV12, tight([(h, w), (h // 2, w)]), I.MATRIX_BT601, I.PIX_YUV420P, 0),
        ("NV12 BT.709 -> RGB24", I.SRC_NV12, tight([(h, w), (h // 2, w)]), I.MATRIX_BT709, I.PIX_RGB24, 0),
        ("P010 BT.709 -> RGB24 bilinear", I.SRC_P010, tight([(h, 2 * w), (h // 2, 2 * w)]), I.MATRIX_BT709, I.PIX_RGB24, I.INGEST_CHROMA_BILINEAR),
        ("YUV422P10 -> YUV420P", I.SRC_YUV422P10, tight([(h, 2 * w), (h, w), (h, w)]), I.MATRIX_BT601, I.PIX_YUV420P, 0),
    ]
    legs, moved, keep = {}, {}, []
    for name, fmt, (planes, size), matrix, out_format, options in variants:
        g = I.Ingest(fmt, w, h, planes, matrix, False, out_format, options)
        srcs = [torch.randint(0, 256, (n, size), dtype=torch.uint8, device="cuda:0") for _ in range(args.sets)]
        outs = [torch.empty((n, g.output_bytes), dtype=torch.uint8, device="cuda:0") for _ in range(args.sets)]
        total = n * (size + g.output_bytes)
        a = [torch.randint(0, 256, (total // 2,), dtype=torch.uint8, device="cuda:0") for _ in range(args.sets)]
        b = [torch.empty_like(t) for t in a]
        keep.append(g)
        turn = {"i": 0}

        def convert(g=g, srcs=srcs, outs=outs, turn=turn):
            k = turn["i"] = (turn["i"] + 1) % args.sets
            g.convert_device(srcs[k], d_out=outs[k])

        def copy(a=a, b=b, turn=turn):
            k = turn["i"] = (turn["i"] + 1) % args.sets
            b[k].copy_(a[k])
        legs[name] = convert
        legs["copy_ of the bytes of " + name] = copy
        moved[name] = moved["copy_ of the bytes of " + name] = total
    torch.cuda.synchronize()

    reps = {}
    for leg, fn in legs.items():                           # warm up and size the window
        for _ in range(2 * args.sets):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(4 * args.sets):
            fn()
        torch.cuda.synchronize()
        reps[leg] = max(2 * args.sets, int(args.window_ms * 1e-3 / ((time.perf_counter() - t0) / (4 * args.sets))))
    times = {leg: [] for leg in legs}
    for _ in range(args.windows):                          # the legs alternate: drift hits all of them alike
        for leg, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps[leg]):
                fn()
            b.record()
            b.synchronize()
            times[leg].append(a.elapsed_time(b) * 1e3 / reps[leg])
    us = {leg: [round(statistics.median(t), 2), round(min(t), 2), round(max(t), 2)] for leg, t in times.items()}
    rate = {leg: round(moved[leg] / (us[leg][0] * 1e-6) / 1e9, 1) for leg in legs}
    record = {
        "kernel_rev": I.kernel_rev(), "device": torch.cuda.get_device_name(0),
        "width": w, "height": h, "pictures": n, "buffer_sets": args.sets, "windows": args.windows,
        "method": "HIP events around windows of back-to-back launches, each on the next of the leg's buffer sets; median [min, max] "
                  "microseconds per launch of the whole batch; bytes moved computed from the shapes (sample bytes in + packed output out; "
                  "the copy_ beside a variant reads half of that and writes half)",
        "microseconds_per_launch": us, "launches_per_window": reps, "bytes_moved_per_launch": moved,
        "gigabytes_moved_per_second": rate,
        "rate_over_the_copys": {name: round(rate[name] / rate["copy_ of the bytes of " + name], 3) for name, *_ in variants},
        "pictures_per_second": {name: round(n / (us[name][0] * 1e-6), 1) for name, *_ in variants},
    }
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
