#!/usr/bin/env python3
"""Times the display back-end (psxavenc_amd/display.py) for each format and chroma mode on the batch bench.py measures
(1000 x 320x240), with the decoder's reconstruct kernel on the same batch alongside.

  python tools/gpu_display_probe.py --out profiles/<kernel rev>_probe.json

Device events around windows of back-to-back launches (each window long enough that the clock's grain does not matter), every shape
warmed up first, the legs alternated inside one run, median and spread over the windows reported.  Bytes moved are what the
algorithm needs, computed from the shapes: 1.5 bytes read and 2, 3 or 4 written per pixel (bilinear chroma reads the same bytes:
its neighbours come out of cache lines the kernel fetches anyway).  The batch (115 MB in, up to 307 MB out) is of the order of the
256 MB last-level cache: the rates are those of this workload, not of HBM alone.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=250.0, help="target length of a timed window")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "gpu_display_probe needs an MI355X"
    from psxavenc_amd import MdecDecoder, decode, display, synth
    from psxavenc_amd.mdec import MdecEncoder

    w, h, budget, n = 320, 240, 8192, args.frames
    px = w * h * n
    d_frames = synth.frames_device(w, h, 1, 0, n, 4, device=0)
    enc, dec = MdecEncoder(0, w, h, max_frame_size=budget, device=0), MdecDecoder(w, h)
    d_out, d_res = enc.encode_frames_device(d_frames, budget)
    d_lv, d_px, d_dec = dec.decode_frames_device(d_out, budget)
    torch.cuda.synchronize()
    assert (d_dec[:, 0] == 0).all()

    names = {display.OUT_RGB24: "RGB24", display.OUT_RGBX32: "RGBX32", display.OUT_RGB555: "RGB555"}
    legs, moved = {}, {}
    for fmt, name in names.items():
        for chroma, cname in ((0, "replicate"), (display.DISPLAY_CHROMA_BILINEAR, "bilinear")):
            for extra, ename in ((0, ""), (display.DISPLAY_DITHER, " dither")) if fmt == display.OUT_RGB555 else ((0, ""),):
                d_dst = display.convert_device(d_px, w, h, fmt, chroma | extra)
                leg = "convert %s %s%s" % (name, cname, ename)
                legs[leg] = (lambda fmt=fmt, o=chroma | extra, d_dst=d_dst: display.convert_device(d_px, w, h, fmt, o, d_dst=d_dst))
                moved[leg] = px * 3 // 2 + n * h * display.row_bytes(fmt, w)
    d_555 = display.convert_device(d_px, w, h, display.OUT_RGB555, 0)
    legs["parse + reconstruct"] = lambda: dec.decode_frames_device(d_out, budget, d_levels=d_lv, d_frames=d_px, d_decoded=d_dec)
    legs["parse (levels out)"] = lambda: dec.decode_frames_device(d_out, budget, frames=False, d_levels=d_lv, d_decoded=d_dec)
    legs["decode_display RGB555 replicate"] = lambda: dec.decode_display_device(d_out, budget, display.OUT_RGB555, 0, d_decoded=d_dec, d_dst=d_555)
    moved["reconstruct (difference)"] = px * 3 // 2 + n * dec.blocks * 128          # levels in, NV21 out
    torch.cuda.synchronize()

    reps = {}
    for leg, fn in legs.items():                           # warm up and size the window
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        reps[leg] = max(20, int(args.window_ms * 1e-3 / ((time.perf_counter() - t0) / 20)))
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
    us["reconstruct (difference)"] = [round(us["parse + reconstruct"][0] - us["parse (levels out)"][0], 2)]
    record = {
        "kernel_rev": display.kernel_rev(), "decode_kernel_rev": decode.kernel_rev(), "device": torch.cuda.get_device_name(0),
        "width": w, "height": h, "frames": n, "windows": args.windows,
        "method": "HIP events around windows of back-to-back launches; median [min, max] microseconds per launch of the whole batch; "
                  "bytes moved computed from the shapes (NV21 in + row bytes out; reconstruct: levels in + NV21 out)",
        "microseconds_per_launch": us, "launches_per_window": reps,
        "bytes_moved_per_launch": moved,
        "gigabytes_moved_per_second": {leg: round(moved[leg] / (us[leg][0] * 1e-6) / 1e9, 1) for leg in moved if us[leg][0] > 0},
        "frames_per_second": {leg: round(n / (v[0] * 1e-6), 1) for leg, v in us.items() if v[0] > 0},
    }
    enc.close()
    dec.close()
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
